// nf4_dequant_cpu.cpp -- the host-CPU NF4 double dequantization of libnf4dq.so
// ("nf4_dequant_ref_cpu(...), thread count as a parameter").
//
// What it replaces: the reference's CPU path, _aggressive_pytorch_t4
// (nf4_triton_dequantization/kernel_optimized.py:208-314), which loops over the
// 64-column blocks in Python (:267) and writes the output column by column
// (:305-312).  Same semantics, bit for bit (the HIP kernels' semantics too):
//
//   s(r, b)   = ((float)absmax_q[(r*bpr + b) mod nb] / 127.0f) * absmax2[(r*G + b/4) mod n2]
//   out[r][c] = RNE(NF4[nib(r, c)] * s(r, c/64)),  high nibble -> even column
//
// (single-quant branch :273-274: s(r, b) = absmax[r*(absmax_len/m) + b]).
//
// Design: every output of a 64-column block is one of only 16 values, so a block
// costs 16 fp32 products + 16 roundings (IEEE, no fused ops) into a 16-entry
// table of output bit patterns, and the 64 outputs are table lookups on the
// nibbles: with AVX2 one vpshufb per output byte plane per 32 outputs
// (the 16-bit outputs split into low-byte and high-byte tables), so the block
// is ~20 vector instructions and the loop runs at memory speed.  Rows are split
// over `threads` std::thread workers (no OpenMP runtime: the library is loaded
// into processes that already carry torch's).  A CPU without AVX2 takes the
// portable scalar table loop (same tables, same results).
#include <float.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include <immintrin.h>

#include "../../include/nf4_dequant.h"
#include "nf4_embed_plan.h"
#include "nf4_quant_plan.h"

namespace {

// The 16 NF4 code points (fp32 bit patterns of kernel_optimized.py:234-239).
constexpr uint32_t kCode[16] = {0xbf800000u, 0xbf3239b1u, 0xbf066b30u, 0xbeca32a0u, 0xbe91a24du, 0xbe3d353fu,
                                0xbdba7871u, 0x00000000u, 0x3da2faffu, 0x3e24cae3u, 0x3e7c04ddu, 0x3ead033au,
                                0x3ee1a4b8u, 0x3f1007abu, 0x3f3913b3u, 0x3f800000u};

enum Mode { kRef, kSingle };

inline float code_f(int i) {
    float f;
    memcpy(&f, &kCode[i], 4);
    return f;
}

inline uint16_t bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN (quiet)
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

inline uint16_t f16_rne(float x) {
    const _Float16 h = (_Float16)x;  // IEEE RNE incl. subnormals and overflow to inf
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}

struct Job {
    const uint8_t* packed;
    int64_t stride;  // packed bytes per row (packed_len / m)
    const uint8_t* a1;
    int64_t nb;
    const float* a2;  // ref: nested absmax; single: fp32 absmax rows
    int64_t n2;       // ref: modulus; single: absmax row stride
    void* out;
    int64_t m, n, bpr, groups;
};

// 16 outputs of one block: products in fp32 (same op order as the kernels and
// the reference: LUT value times block scale), then the output rounding.
template <int DT>
inline void block_table(float s, uint16_t* t16, float* t32) {
    for (int k = 0; k < 16; ++k) {
        const float p = code_f(k) * s;  // one IEEE product (-ffp-contract=off; x86 has no fused multiply-round)
        if constexpr (DT == NF4DQ_F32) t32[k] = p;
        else if constexpr (DT == NF4DQ_BF16) t16[k] = bf16_rne(p);
        else t16[k] = f16_rne(p);
    }
}

// Scalar: any block width (partial last block, odd n).
template <int DT>
inline void block_scalar(const uint8_t* src, void* out, int64_t c0, int64_t cnt, const uint16_t* t16,
                         const float* t32) {
    for (int64_t k = 0; k < cnt; ++k) {
        const int64_t c = c0 + k;
        const uint8_t byte = src[c >> 1];
        const int nib = (c & 1) ? (byte & 15) : (byte >> 4);
        if constexpr (DT == NF4DQ_F32) reinterpret_cast<float*>(out)[c] = t32[nib];
        else reinterpret_cast<uint16_t*>(out)[c] = t16[nib];
    }
}

// AVX2: 32 packed bytes -> 64 16-bit outputs with four vpshufb per 32 outputs.
__attribute__((target("avx2"))) inline void block64_avx2(const uint8_t* src, uint16_t* dst, const uint16_t* t16) {
    alignas(16) uint8_t lo[16], hi[16];
    for (int k = 0; k < 16; ++k) {
        lo[k] = (uint8_t)(t16[k] & 0xFF);
        hi[k] = (uint8_t)(t16[k] >> 8);
    }
    const __m256i tlo = _mm256_broadcastsi128_si256(_mm_load_si128(reinterpret_cast<const __m128i*>(lo)));
    const __m256i thi = _mm256_broadcastsi128_si256(_mm_load_si128(reinterpret_cast<const __m128i*>(hi)));
    const __m256i m4 = _mm256_set1_epi8(0x0F);
    const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src));
    const __m256i nh = _mm256_and_si256(_mm256_srli_epi16(v, 4), m4);
    const __m256i nl = _mm256_and_si256(v, m4);
    // per 128-bit lane: (hi0, lo0, hi1, lo1, ...) = column order of the outputs
    const __m256i i0 = _mm256_unpacklo_epi8(nh, nl);  // lane0: bytes 0-7 (cols 0-15), lane1: bytes 16-23 (32-47)
    const __m256i i1 = _mm256_unpackhi_epi8(nh, nl);  // lane0: bytes 8-15 (16-31), lane1: bytes 24-31 (48-63)
    __m256i* d = reinterpret_cast<__m256i*>(dst);
    {
        const __m256i L = _mm256_shuffle_epi8(tlo, i0), H = _mm256_shuffle_epi8(thi, i0);
        const __m256i w0 = _mm256_unpacklo_epi8(L, H), w1 = _mm256_unpackhi_epi8(L, H);
        _mm256_storeu_si256(d + 0, _mm256_permute2x128_si256(w0, w1, 0x20));
        _mm256_storeu_si256(d + 2, _mm256_permute2x128_si256(w0, w1, 0x31));
    }
    {
        const __m256i L = _mm256_shuffle_epi8(tlo, i1), H = _mm256_shuffle_epi8(thi, i1);
        const __m256i w0 = _mm256_unpacklo_epi8(L, H), w1 = _mm256_unpackhi_epi8(L, H);
        _mm256_storeu_si256(d + 1, _mm256_permute2x128_si256(w0, w1, 0x20));
        _mm256_storeu_si256(d + 3, _mm256_permute2x128_si256(w0, w1, 0x31));
    }
}

template <int DT, int MODE, bool AVX2>
void run_rows(const Job& J, int64_t r0, int64_t r1) {
    const int64_t osz = DT == NF4DQ_F32 ? 4 : 2;
    alignas(32) uint16_t t16[16];
    alignas(32) float t32[16];
    for (int64_t r = r0; r < r1; ++r) {
        const uint8_t* src = J.packed + r * J.stride;
        void* orow = reinterpret_cast<uint8_t*>(J.out) + r * J.n * osz;
        int64_t i1 = 0, i2 = 0;
        if constexpr (MODE == kRef) {
            i1 = (r * J.bpr) % J.nb;        // (r*bpr + b) mod nb, advanced per block
            i2 = (r * J.groups) % J.n2;     // (r*G + b/4) mod n2, advanced every 4 blocks
        }
        for (int64_t b = 0; b < J.bpr; ++b) {
            float s;
            if constexpr (MODE == kRef) {
                s = ((float)J.a1[i1] / 127.0f) * J.a2[i2];  // IEEE division (:45, :270), then fp32 multiply
                if (++i1 == J.nb) i1 = 0;
                if ((b & 3) == 3 && ++i2 == J.n2) i2 = 0;
            } else {
                s = J.a2[r * J.n2 + b];
            }
            block_table<DT>(s, t16, t32);
            const int64_t c0 = b * 64;
            const int64_t cnt = J.n - c0 < 64 ? J.n - c0 : 64;
            if constexpr (AVX2 && DT != NF4DQ_F32) {
                if (cnt == 64) {
                    block64_avx2(src + (c0 >> 1), reinterpret_cast<uint16_t*>(orow) + c0, t16);
                    continue;
                }
            }
            block_scalar<DT>(src, orow, c0, cnt, t16, t32);
        }
    }
}

template <int MODE>
void dispatch_rows(const Job& J, int32_t dtype, int64_t r0, int64_t r1, bool avx2) {
#define NF4_CPU_ROWS(DT_)                                              \
    do {                                                               \
        if (avx2) run_rows<DT_, MODE, true>(J, r0, r1);                \
        else run_rows<DT_, MODE, false>(J, r0, r1);                    \
    } while (0)
    if (dtype == NF4DQ_BF16) NF4_CPU_ROWS(NF4DQ_BF16);
    else if (dtype == NF4DQ_F16) NF4_CPU_ROWS(NF4DQ_F16);
    else NF4_CPU_ROWS(NF4DQ_F32);
#undef NF4_CPU_ROWS
}

template <int MODE>
int run(const Job& J, int32_t dtype, int32_t threads) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    int64_t t = threads > 0 ? threads : (int64_t)std::max(1u, std::thread::hardware_concurrency());
    // at least 16 rows of work per worker (thread start-up is ~tens of us)
    t = std::max<int64_t>(1, std::min<int64_t>(t, (J.m + 15) / 16));
    if (t == 1) {
        dispatch_rows<MODE>(J, dtype, 0, J.m, avx2);
        return NF4DQ_OK;
    }
    std::vector<std::thread> pool;
    pool.reserve((size_t)t - 1);
    const int64_t per = (J.m + t - 1) / t;
    for (int64_t i = 1; i < t; ++i) {
        const int64_t r0 = i * per, r1 = std::min(J.m, r0 + per);
        if (r0 >= r1) break;
        pool.emplace_back([&J, dtype, r0, r1] { dispatch_rows<MODE>(J, dtype, r0, r1, avx2); });
    }
    dispatch_rows<MODE>(J, dtype, 0, std::min(J.m, per), avx2);
    for (auto& th : pool) th.join();
    return NF4DQ_OK;
}

// Same acceptance rules as the device entry points (what .view(m, -1) and the
// slicing of kernel_optimized.py:229, :288-312 accept).
int check(const uint8_t* packed, int64_t packed_len, const void* out, int32_t dtype, int64_t m, int64_t n) {
    if (dtype != NF4DQ_F16 && dtype != NF4DQ_BF16 && dtype != NF4DQ_F32) return NF4DQ_ERR_ARG;
    if (m < 0 || n < 0 || packed_len < 0) return NF4DQ_ERR_ARG;
    if (m == 0 || n == 0) return NF4DQ_OK;
    if (!packed || !out) return NF4DQ_ERR_ARG;
    if (packed_len % m) return NF4DQ_ERR_SHAPE;
    if (packed_len / m < (n + 1) / 2) return NF4DQ_ERR_SHAPE;
    return NF4DQ_OK;
}

}  // namespace

extern "C" {

int nf4_dequant_ref_cpu(const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q, int64_t nb,
                        const float* absmax2, int64_t n2, void* out, int32_t out_dtype, int64_t m, int64_t n,
                        int32_t threads) {
    const int rc = check(packed, packed_len, out, out_dtype, m, n);
    if (rc || m == 0 || n == 0) return rc;
    if (!absmax_q || !absmax2 || nb <= 0 || n2 <= 0) return NF4DQ_ERR_ARG;
    Job J{};
    J.packed = packed;
    J.stride = packed_len / m;
    J.a1 = absmax_q;
    J.nb = nb;
    J.a2 = absmax2;
    J.n2 = n2;
    J.out = out;
    J.m = m;
    J.n = n;
    J.bpr = (n + 63) / 64;
    J.groups = (J.bpr + 3) / 4;
    return run<kRef>(J, out_dtype, threads);
}

int nf4_dequant_single_cpu(const uint8_t* packed, int64_t packed_len, const float* absmax, int64_t absmax_len,
                           void* out, int32_t out_dtype, int64_t m, int64_t n, int32_t threads) {
    const int rc = check(packed, packed_len, out, out_dtype, m, n);
    if (rc || m == 0 || n == 0) return rc;
    if (!absmax || absmax_len < 0) return NF4DQ_ERR_ARG;
    const int64_t bpr = (n + 63) / 64;
    if (absmax_len % m || absmax_len / m < bpr) return NF4DQ_ERR_SHAPE;
    Job J{};
    J.packed = packed;
    J.stride = packed_len / m;
    J.a2 = absmax;
    J.n2 = absmax_len / m;
    J.out = out;
    J.m = m;
    J.n = n;
    J.bpr = bpr;
    return run<kSingle>(J, out_dtype, threads);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Host forms of the NF4 quantizer (nf4_quant.hip): the same arithmetic -- fp32 absmax,
// one IEEE division per element, count of the midpoints below the quotient, fp64 absmax
// sum in the order of nf4_quant_plan.h -- so the same bits.  Blocks are split over threads.
// ---------------------------------------------------------------------------
namespace {

inline float quant_elem(const void* w, int32_t dt, int64_t i) {
    if (dt == NF4DQ_F32) return reinterpret_cast<const float*>(w)[i];
    const uint16_t h = reinterpret_cast<const uint16_t*>(w)[i];
    if (dt == NF4DQ_BF16) {
        const uint32_t u = (uint32_t)h << 16;
        float f;
        memcpy(&f, &u, 4);
        return f;
    }
    _Float16 f;
    memcpy(&f, &h, 2);
    return (float)f;
}

inline float abs_f(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u &= 0x7fffffffu;
    memcpy(&x, &u, 4);
    return x;
}

struct QuantMids {
    float m[15];
    QuantMids() {
        for (int j = 0; j < 15; ++j) m[j] = (code_f(j) + code_f(j + 1)) / 2.0f;
    }
};

inline uint32_t quant_code(float q, const QuantMids& M) {
    uint32_t c = 0;
    for (int j = 0; j < 15; ++j) c += M.m[j] < q ? 1u : 0u;
    return c;
}

void quant_blocks(const void* w, int32_t dt, int64_t numel, int32_t bs, uint8_t* packed, float* absmax, int64_t b0,
                  int64_t b1) {
    static const QuantMids M;
    for (int64_t b = b0; b < b1; ++b) {
        const int64_t e0 = b * bs, e1 = std::min<int64_t>(numel, e0 + bs);
        float amax = 0.0f;
        for (int64_t i = e0; i < e1; ++i) {
            const float a = abs_f(quant_elem(w, dt, i));
            amax = a > amax ? a : amax;
        }
        absmax[b] = amax;
        const float safe = amax > 0.0f ? amax : 1.0f;
        for (int64_t i = e0; i < e1; i += 2) {
            const uint32_t hi = quant_code(quant_elem(w, dt, i) / safe, M);
            const uint32_t lo = i + 1 < numel ? quant_code(quant_elem(w, dt, i + 1) / safe, M) : 7u;  // pad 0 -> code 7
            packed[i >> 1] = (uint8_t)(hi << 4 | lo);
        }
    }
}

// `count` items [0, count) split into contiguous ranges over up to `threads` workers
template <class F>
void split_ranges(int64_t count, int64_t min_per, int32_t threads, F&& fn) {
    int64_t t = threads > 0 ? threads : (int64_t)std::max(1u, std::thread::hardware_concurrency());
    t = std::max<int64_t>(1, std::min<int64_t>(t, (count + min_per - 1) / min_per));
    const int64_t per = (count + t - 1) / t;
    std::vector<std::thread> pool;
    for (int64_t i = 1; i < t; ++i) {
        const int64_t r0 = i * per, r1 = std::min(count, r0 + per);
        if (r0 >= r1) break;
        pool.emplace_back([&fn, r0, r1] { fn(r0, r1); });
    }
    fn(0, std::min(count, per));
    for (auto& th : pool) th.join();
}

// sum_ordered of nf4_quant_plan.h
template <class T>
double sum_ordered(const T* v, int64_t n) {
    double slot[nf4q::kBlock2];
    for (int t = 0; t < nf4q::kBlock2; ++t) {
        double acc = 0.0;
        for (int64_t i = t; i < n; i += nf4q::kBlock2) acc += (double)v[i];
        slot[t] = acc;
    }
    for (int s = nf4q::kBlock2 / 2; s; s >>= 1)
        for (int t = 0; t < s; ++t) slot[t] += slot[t + s];
    return slot[0];
}

int quant_check(const void* w, int32_t dt, int64_t numel, int32_t bs, const void* packed) {
    if (dt != NF4DQ_F16 && dt != NF4DQ_BF16 && dt != NF4DQ_F32) return NF4DQ_ERR_ARG;
    if (numel < 0 || !nf4q::valid_blocksize(bs)) return NF4DQ_ERR_ARG;
    if (numel == 0) return NF4DQ_OK;
    if (!w || !packed) return NF4DQ_ERR_ARG;
    return NF4DQ_OK;
}

}  // namespace

extern "C" {

int nf4_quant_bnb_cpu(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize, void* packed, void* absmax,
                      int32_t threads) {
    const int rc = quant_check(w, in_dtype, numel, blocksize, packed);
    if (rc || numel == 0) return rc;
    if (!absmax) return NF4DQ_ERR_ARG;
    const int64_t nblk = (numel + blocksize - 1) / blocksize;
    uint8_t* p = reinterpret_cast<uint8_t*>(packed);
    float* am = reinterpret_cast<float*>(absmax);
    // at least 64 Ki elements per worker
    split_ranges(nblk, std::max<int64_t>(1, 65536 / blocksize), threads, [=](int64_t b0, int64_t b1) {
        quant_blocks(w, in_dtype, numel, blocksize, p, am, b0, b1);
    });
    return NF4DQ_OK;
}

int nf4_quant_bnb_nested_cpu(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize, const float* code2,
                             int32_t blocksize2, void* packed, void* absmax_q, void* absmax2, void* offset,
                             int32_t threads) {
    int rc = quant_check(w, in_dtype, numel, blocksize, packed);
    if (rc) return rc;
    if (blocksize2 != nf4q::kBlock2) return NF4DQ_ERR_ARG;
    if (numel == 0) return NF4DQ_OK;
    if (!code2 || !absmax_q || !absmax2 || !offset) return NF4DQ_ERR_ARG;
    const int64_t nblk = (numel + blocksize - 1) / blocksize;
    std::vector<float> am((size_t)nblk);
    rc = nf4_quant_bnb_cpu(w, in_dtype, numel, blocksize, packed, am.data(), threads);
    if (rc) return rc;
    const nf4q::SumPlan sp = nf4q::sum_plan(nblk);
    std::vector<double> parts((size_t)sp.parts);
    for (int32_t p = 0; p < sp.parts; ++p) {
        const int64_t b0 = (int64_t)p * sp.chunk;
        parts[(size_t)p] = sum_ordered(am.data() + b0, std::min(nblk - b0, sp.chunk));
    }
    const float off = (float)(sum_ordered(parts.data(), sp.parts) / (double)nblk);
    *reinterpret_cast<float*>(offset) = off;
    float mids[255];
    for (int j = 0; j < 255; ++j) mids[j] = (code2[j] + code2[j + 1]) / 2.0f;
    uint8_t* aq = reinterpret_cast<uint8_t*>(absmax_q);
    float* a2 = reinterpret_cast<float*>(absmax2);
    const int64_t n2 = (nblk + nf4q::kBlock2 - 1) / nf4q::kBlock2;
    const float* amp = am.data();
    split_ranges(n2, 64, threads, [=, &mids](int64_t g0, int64_t g1) {
        for (int64_t g = g0; g < g1; ++g) {
            const int64_t i0 = g * nf4q::kBlock2, i1 = std::min(nblk, i0 + nf4q::kBlock2);
            float m = 0.0f;
            for (int64_t i = i0; i < i1; ++i) {
                const float a = abs_f(amp[i] - off);
                m = a > m ? a : m;
            }
            m = m > FLT_MIN ? m : FLT_MIN;
            a2[g] = m;
            for (int64_t i = i0; i < i1; ++i) {
                const float q = (amp[i] - off) / m;
                aq[i] = (uint8_t)(std::lower_bound(mids, mids + 255, q) - mids);
            }
        }
    });
    return NF4DQ_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Host forms of the embedding gather (nf4_embed.hip): the validation is the device entries'
// (nf4_embed_plan.h), the arithmetic the bitsandbytes-mode kernels' -- fp32 product of the
// nested code and absmax2, then the offset added (two roundings), fp32 product with the NF4
// code, one rounding to the output type -- so the same bits.  A plain loop over the output
// rows, split over threads; an id outside [0, rows) gives a row of zero bits and reads
// nothing from the table.
// ---------------------------------------------------------------------------
namespace {

void embed_rows(const nf4dq::EmbedCall& c, float off, int64_t i0, int64_t i1) {
    const int bsh = (int)nf4dq::embed_log2((uint64_t)c.blocksize);
    const int bsh2 = c.single ? 0 : (int)nf4dq::embed_log2((uint64_t)c.blocksize2);
    const size_t esize = c.out_dtype == NF4DQ_F32 ? 4 : 2;
    for (int64_t i = i0; i < i1; ++i) {
        bool ok;
        int64_t id;
        if (c.ids_dtype == NF4DQ_IDS_I64) {
            id = reinterpret_cast<const int64_t*>(c.ids)[i];
            ok = id >= 0 && id < c.rows;
        } else {
            const int32_t v = reinterpret_cast<const int32_t*>(c.ids)[i];
            id = v;
            ok = v >= 0 && (int64_t)v < c.rows;
        }
        char* row = reinterpret_cast<char*>(c.out) + (size_t)i * (size_t)c.dim * esize;
        if (!ok) {
            memset(row, 0, (size_t)c.dim * esize);
            continue;
        }
        const int64_t e0 = id * c.dim;
        for (int64_t j = 0; j < c.dim; ++j) {
            const int64_t e = e0 + j;
            const uint8_t byte = c.packed[e >> 1];
            const int nib = (e & 1) ? (byte & 15) : (byte >> 4);
            const int64_t b = e >> bsh;
            float s;
            if (c.single) {
                s = c.a2[b];
            } else {
                const float p = c.code2[c.a1[b]] * c.a2[b >> bsh2];  // (-ffp-contract=off: rounded here)
                s = p + off;
            }
            const float x = code_f(nib) * s;
            if (c.out_dtype == NF4DQ_F32) reinterpret_cast<float*>(row)[j] = x;
            else reinterpret_cast<uint16_t*>(row)[j] = c.out_dtype == NF4DQ_BF16 ? bf16_rne(x) : f16_rne(x);
        }
    }
}

int embed_cpu(const nf4dq::EmbedCall& c, int32_t threads) {
    const nf4dq::EmbedPlan P = nf4dq::plan_embed(c);
    if (P.rc != NF4DQ_OK || P.launches == 0) return P.rc;
    const float off = (!c.single && c.offset) ? *c.offset : 0.0f;
    // at least 64 Ki elements per worker
    split_ranges(c.count, std::max<int64_t>(1, 65536 / c.dim), threads,
                 [&c, off](int64_t i0, int64_t i1) { embed_rows(c, off, i0, i1); });
    return NF4DQ_OK;
}

}  // namespace

extern "C" {

int nf4_embedding_bnb_cpu(const void* ids, int32_t ids_dtype, int64_t count, const uint8_t* packed,
                          const uint8_t* absmax_q, int64_t nb, const float* code2, const float* absmax2, int64_t n2,
                          const float* offset, int32_t blocksize, int32_t blocksize2, void* out, int32_t out_dtype,
                          int64_t rows, int64_t dim, int32_t threads) {
    const nf4dq::EmbedCall c{ids, ids_dtype, count, packed, absmax_q, nb, code2, absmax2, n2, offset,
                             blocksize, blocksize2, out, out_dtype, rows, dim, false};
    return embed_cpu(c, threads);
}

int nf4_embedding_bnb_single_cpu(const void* ids, int32_t ids_dtype, int64_t count, const uint8_t* packed,
                                 const float* absmax, int64_t nabs, int32_t blocksize, void* out, int32_t out_dtype,
                                 int64_t rows, int64_t dim, int32_t threads) {
    const nf4dq::EmbedCall c{ids, ids_dtype, count, packed, nullptr, nabs, nullptr, absmax, 0, nullptr,
                             blocksize, 0, out, out_dtype, rows, dim, true};
    return embed_cpu(c, threads);
}

}  // extern "C"
