// nf4_quant.hip -- the producer side of libnf4dq.so: float weights (fp16 / bf16 / fp32,
// a flat element stream) into the bitsandbytes NF4 layout, on gfx950.
//
// The specification is bnb_layout.quantize_nf4 (a chain of torch ops), bit for bit:
//
//   absmax[b] = max |x| over block b (fp32; elements past numel read as 0)
//   safe      = absmax > 0 ? absmax : 1
//   q         = x / safe                      (one correctly rounded IEEE fp32 division)
//   code      = #{ j : mid_j < q },  mid_j = (c_j + c_{j+1}) / 2 in fp32   (a tie -> lower code)
//   packed[i] = code[2i] << 4 | code[2i+1]    (an odd numel is padded with one 0: code 7)
//
// and, for compress_statistics=True, the nested statistics of the fp32 absmax:
//
//   offset      = fp32( (sum of absmax in fp64, fixed order: nf4_quant_plan.h) / nblk )
//   v           = absmax - offset (fp32; elements past nblk read as 0)
//   absmax2[g]  = max(max |v| over 256-block g, FLT_MIN)
//   absmax_q[i] = #{ j : mid2_j < v[i] / absmax2[i / 256] },  mid2_j = (code2_j + code2_{j+1}) / 2
//
// Kernels:
//   nf4_quant_blocks_kernel<DT>          blocksize 64, 16-byte aligned input, 4-byte aligned
//       packed: a wave owns a tile of 512 elements, a lane 8 consecutive ones (one 16-byte
//       non-temporal load for fp16 / bf16, two for fp32); the 8 lanes of a block fold their
//       maxima with three DPP moves; a lane stores its 4 packed bytes as one dword, so a wave
//       writes 256 contiguous bytes.  The weight is read once.
//   nf4_quant_blocks_general_kernel<DT>  every other alignment and block size: a wave per
//       block, two passes over it (the second one hits the cache), one byte per lane and step.
//   nf4_quant_absmax_sum_kernel          per-workgroup fp64 partial sums of absmax
//   nf4_quant_stats_kernel               every workgroup folds the partials in the same fixed
//       order (no float atomics: two runs are bitwise equal), then quantizes one 256-block of
//       absmax - offset against the 255 midpoints of code2, staged in LDS and binary-searched.
#include "nf4_common.h"
#include "nf4_quant_plan.h"

#include <float.h>

namespace {

using nf4dq::kNf4Bits;
using nf4dq::u32x4;

constexpr int kQWg = 256;                     // threads per workgroup
constexpr int kQWaves = kQWg / 64;            // waves per workgroup
constexpr int kQLane = 8;                     // elements per lane (fast form)
constexpr int kQTile = 64 * kQLane;           // elements per wave (fast form)
constexpr int64_t kMaxGrid = 0x7fffffff;

constexpr float code_pt(int j) { return __builtin_bit_cast(float, kNf4Bits[j]); }
// fp32 sum, then an exact halving: torch's (code[1:] + code[:-1]) / 2.0
constexpr float mid_pt(int j) { return (code_pt(j) + code_pt(j + 1)) / 2.0f; }

// #{ j : mid_j < q }: bucketize(q, mids, right=False).
__device__ __forceinline__ uint32_t nf4_code_of(float q) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 15; ++j) c += mid_pt(j) < q ? 1u : 0u;
    return c;
}

// The streaming kernel's form of the same count: one table look-up and one comparison.
// bucket(q) = trunc(clamp(fl(q * 16 + 16), 0, 32)) is monotone in q, so a midpoint in a
// lower bucket than q's is below q, one in a higher bucket is above it, and only a midpoint
// in q's own bucket needs comparing.  Buckets are 1/16 wide and neighbouring midpoints at
// least 0.08 apart (checked below), so a bucket holds at most one: entry b = {that midpoint
// or +inf, the number of midpoints in lower buckets}.  The table is built with the bucket
// function's own rounding (q * 16 + 16 is exact in fp64 for the midpoints, then one rounding
// to fp32: the fma's result), so the count is exact by construction, not by tolerance.
constexpr int kBuckets = 33;
constexpr int bucket_of_mid(int j) { return (int)(float)((double)mid_pt(j) * 16.0 + 16.0); }

struct CodeEntry {
    float thr;
    uint32_t base;
};
struct CodeTable {
    CodeEntry e[kBuckets];
};

constexpr CodeTable make_code_table() {
    CodeTable t{};
    for (int b = 0; b < kBuckets; ++b) {
        t.e[b].thr = __builtin_huge_valf();
        t.e[b].base = 0;
        for (int j = 0; j < 15; ++j) {
            if (bucket_of_mid(j) < b) t.e[b].base += 1;
            if (bucket_of_mid(j) == b) t.e[b].thr = mid_pt(j);
        }
    }
    return t;
}

constexpr bool one_mid_per_bucket() {
    for (int j = 0; j + 1 < 15; ++j)
        if (bucket_of_mid(j) >= bucket_of_mid(j + 1)) return false;
    return bucket_of_mid(0) >= 0 && bucket_of_mid(14) < kBuckets;
}
static_assert(one_mid_per_bucket(), "two NF4 midpoints share a bucket of the code table");

__device__ const CodeTable kCodeTable = make_code_table();

__device__ __forceinline__ uint32_t nf4_code_lut(float q, const CodeEntry* lut) {
    // |q| <= 1 for finite inputs; the clamp keeps a NaN / Inf quotient's index inside the table
    const float f = __builtin_amdgcn_fmed3f(__builtin_fmaf(q, 16.0f, 16.0f), 0.0f, 32.0f);
    const CodeEntry e = lut[(uint32_t)f];
    return e.base + (e.thr < q ? 1u : 0u);
}

template <int DT>
__device__ __forceinline__ float cvt16(uint32_t h) {
    if constexpr (DT == NF4DQ_BF16) {
        return __uint_as_float(h << 16);
    } else {
        return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
    }
}

// Element i of the stream as fp32 (exact for every input dtype).
template <int DT>
__device__ __forceinline__ float load_elem(const void* w, int64_t i) {
    if constexpr (DT == NF4DQ_F32) return reinterpret_cast<const float*>(w)[i];
    else return cvt16<DT>(reinterpret_cast<const uint16_t*>(w)[i]);
}

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// max over the 8 lanes of a 64-element block: lane ^ 1, lane ^ 2 (quad permutes), then the
// other quad of the 8 (half-row mirror: every lane of a quad already holds the quad's max).
__device__ __forceinline__ uint32_t max8(uint32_t m) {
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    m = m > o ? m : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true);           // quad_perm [2,3,0,1]
    m = m > o ? m : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, true);          // row_half_mirror
    return m > o ? m : o;
}

// The eight divisions of a lane share their divisor, so they share its reciprocal.
// `x / a` compiles to v_div_scale (both operands), v_rcp, two fmas refining the reciprocal,
// q0 = n * r, a residual correction e = fma(-d, q, n), q += e * r, a second one whose
// final fma is v_div_fmas, and v_div_fixup.  For a divisor in [2^-32, 2^32] and |x| >= 2^-6 |a| neither
// v_div_scale rescales (their thresholds lie beyond 2^+-64), v_div_fmas is a plain fma and
// v_div_fixup passes a finite non-zero quotient through: the sequence below is that
// expansion instruction for instruction, with the reciprocal's three instructions hoisted,
// so it returns the same correctly rounded quotient.  For |x| < 2^-6 |a| it may differ from it
// (the residuals can underflow) but stays within a few ulp of x / a, below 2^-5: inside
// (mid_6, mid_7) = (-0.0455, 0.0398) like the exact quotient, so the code is 7 either way; a
// zero quotient's sign is not kept, which no threshold sees.  Divisors outside the window
// (subnormal or huge absmax) take the plain division.
struct SharedRcp {
    float d, r;
};

__device__ __forceinline__ bool shared_rcp_ok(float a) {
    return ((__float_as_uint(a) >> 23) & 0xffu) - 95u <= 64u;  // biased exponent 95..159: 2^-32 <= a < 2^33
}

__device__ __forceinline__ SharedRcp make_shared_rcp(float a) {
    const float r0 = __builtin_amdgcn_rcpf(a);
    const float e0 = __builtin_fmaf(-a, r0, 1.0f);
    return SharedRcp{a, __builtin_fmaf(e0, r0, r0)};
}

__device__ __forceinline__ float div_shared(float n, const SharedRcp& s) {
    float q = n * s.r;
    q = __builtin_fmaf(__builtin_fmaf(-s.d, q, n), s.r, q);
    return __builtin_fmaf(__builtin_fmaf(-s.d, q, n), s.r, q);  // the second correction is v_div_fmas' fma
}

template <int DT>
__global__ __launch_bounds__(kQWg) void nf4_quant_blocks_kernel(const void* __restrict__ w, int64_t numel,
                                                                uint8_t* __restrict__ packed,
                                                                float* __restrict__ absmax) {
    __shared__ CodeEntry lut[kBuckets];
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t tile = (int64_t)blockIdx.x * kQWaves + (threadIdx.x >> 6);
    const int64_t t0 = tile * kQTile;
    const int64_t base = t0 + (int64_t)lane * kQLane;
    float x[kQLane];
    // (a wave whose tile starts past numel loads nothing, passes the barrier and leaves whole:
    // every lane of a live wave stays active for the DPP moves)
    if (base + kQLane <= numel) {
        if constexpr (DT == NF4DQ_F32) {
            const u32x4* p = reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(w) + base);
            const u32x4 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k] = __uint_as_float(a[k]);
                x[4 + k] = __uint_as_float(b[k]);
            }
        } else {
            const u32x4 a =
                __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(w) + base));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[2 * k] = cvt16<DT>(a[k] & 0xffffu);
                x[2 * k + 1] = cvt16<DT>(a[k] >> 16);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < kQLane; ++k) x[k] = base + k < numel ? load_elem<DT>(w, base + k) : 0.0f;
    }
    // the code table into LDS behind the weight loads (its own load returns after them)
    if (threadIdx.x < kBuckets) lut[threadIdx.x] = kCodeTable.e[threadIdx.x];
    __syncthreads();
    if (t0 >= numel) return;
    uint32_t m = abs_bits(x[0]);
#pragma unroll
    for (int k = 1; k < kQLane; ++k) {
        const uint32_t a = abs_bits(x[k]);
        m = m > a ? m : a;
    }
    m = max8(m);
    const float amax = __uint_as_float(m);
    const float safe = amax > 0.0f ? amax : 1.0f;
    uint32_t word = 0;
    if (shared_rcp_ok(safe)) {
        const SharedRcp d = make_shared_rcp(safe);
#pragma unroll
        for (int k = 0; k < kQLane; ++k) {
            const uint32_t c = nf4_code_lut(div_shared(x[k], d), lut);
            word |= c << (8 * (k >> 1) + ((k & 1) ? 0 : 4));  // high nibble first; byte k/2 of the dword
        }
    } else {
#pragma unroll
        for (int k = 0; k < kQLane; ++k) {
            const uint32_t c = nf4_code_lut(x[k] / safe, lut);
            word |= c << (8 * (k >> 1) + ((k & 1) ? 0 : 4));
        }
    }
    const int64_t plen = (numel + 1) >> 1;
    const int64_t pb = base >> 1;
    if (pb + 4 <= plen) {
        __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(packed + pb));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (pb + k < plen) packed[pb + k] = (uint8_t)(word >> (8 * k));
    }
    if ((lane & 7u) == 0 && base < numel) absmax[base >> 6] = amax;
}

struct GeneralArgs {
    const void* w;
    int64_t numel;
    int64_t nblk;
    uint8_t* packed;
    float* absmax;
    int32_t bs_shift;
};

template <int DT>
__global__ __launch_bounds__(kQWg) void nf4_quant_blocks_general_kernel(GeneralArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t blk = (int64_t)blockIdx.x * kQWaves + (threadIdx.x >> 6);
    if (blk >= A.nblk) return;
    const int64_t e0 = blk << A.bs_shift;
    const uint32_t pairs = 1u << (A.bs_shift - 1);
    uint32_t m = 0;
    for (uint32_t p = lane; p < pairs; p += 64) {
        const int64_t i = e0 + 2 * (int64_t)p;
        const uint32_t a = i < A.numel ? abs_bits(load_elem<DT>(A.w, i)) : 0u;
        const uint32_t b = i + 1 < A.numel ? abs_bits(load_elem<DT>(A.w, i + 1)) : 0u;
        m = m > a ? m : a;
        m = m > b ? m : b;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t r = (uint32_t)__shfl_xor((int)m, o);
        m = m > r ? m : r;
    }
    const float amax = __uint_as_float(m);
    const float safe = amax > 0.0f ? amax : 1.0f;
    for (uint32_t p = lane; p < pairs; p += 64) {
        const int64_t i = e0 + 2 * (int64_t)p;
        if (i >= A.numel) break;
        const float a = load_elem<DT>(A.w, i);
        const float b = i + 1 < A.numel ? load_elem<DT>(A.w, i + 1) : 0.0f;
        A.packed[i >> 1] = (uint8_t)(nf4_code_of(a / safe) << 4 | nf4_code_of(b / safe));
    }
    if (lane == 0) A.absmax[blk] = amax;
}

// slot[0] = the slots folded pairwise in a fixed order (nf4_quant_plan.h); all threads return it
__device__ __forceinline__ double fold256(double* slot, double mine) {
    const uint32_t t = threadIdx.x;
    slot[t] = mine;
    __syncthreads();
#pragma unroll
    for (uint32_t s = nf4q::kBlock2 / 2; s; s >>= 1) {
        if (t < s) slot[t] += slot[t + s];
        __syncthreads();
    }
    return slot[0];
}

__global__ __launch_bounds__(nf4q::kBlock2) void nf4_quant_absmax_sum_kernel(const float* __restrict__ absmax,
                                                                           int64_t nblk, int64_t chunk,
                                                                           double* __restrict__ parts) {
    __shared__ double slot[nf4q::kBlock2];
    const int64_t b0 = (int64_t)blockIdx.x * chunk;
    const int64_t b1 = b0 + chunk < nblk ? b0 + chunk : nblk;
    double acc = 0.0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += nf4q::kBlock2) acc += (double)absmax[i];
    const double s = fold256(slot, acc);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

__global__ __launch_bounds__(nf4q::kBlock2) void nf4_quant_stats_kernel(const float* __restrict__ absmax, int64_t nblk,
                                                                      const double* __restrict__ parts, int32_t nparts,
                                                                      const float* __restrict__ code2,
                                                                      uint8_t* __restrict__ absmax_q,
                                                                      float* __restrict__ absmax2,
                                                                      float* __restrict__ offset) {
    __shared__ double slot[nf4q::kBlock2];
    __shared__ float mids[nf4q::kBlock2];
    __shared__ uint32_t wmax[nf4q::kBlock2 / 64];
    const uint32_t t = threadIdx.x;
    // the 255 decision thresholds of the code book; slot 255 is never below a quotient
    mids[t] = t < 255 ? (code2[t] + code2[t + 1]) / 2.0f : __uint_as_float(0x7f800000u);
    double acc = 0.0;
    for (int32_t i = (int32_t)t; i < nparts; i += nf4q::kBlock2) acc += parts[i];
    const double total = fold256(slot, acc);  // its barriers also publish mids
    const float off = (float)(total / (double)nblk);
    if (blockIdx.x == 0 && t == 0) *offset = off;
    const int64_t i = (int64_t)blockIdx.x * nf4q::kBlock2 + t;
    const float v = i < nblk ? absmax[i] - off : 0.0f;
    uint32_t m = abs_bits(v);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t r = (uint32_t)__shfl_xor((int)m, o);
        m = m > r ? m : r;
    }
    if ((t & 63u) == 0) wmax[t >> 6] = m;
    __syncthreads();
    m = wmax[0];
#pragma unroll
    for (int k = 1; k < nf4q::kBlock2 / 64; ++k) m = m > wmax[k] ? m : wmax[k];
    float amax2 = __uint_as_float(m);
    amax2 = amax2 > FLT_MIN ? amax2 : FLT_MIN;
    const float q = v / amax2;
    uint32_t c = 0;  // #{ j : mids[j] < q } of the sorted thresholds
#pragma unroll
    for (uint32_t s = 128; s; s >>= 1)
        if (mids[c + s - 1] < q) c += s;
    if (i < nblk) absmax_q[i] = (uint8_t)c;
    if (t == 0) absmax2[blockIdx.x] = amax2;
}

inline int hip_rc(hipError_t e) { return e == hipSuccess ? NF4DQ_OK : NF4DQ_ERR_HIP_BASE + (int)e; }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int ilog2(uint32_t v) {
    int s = 0;
    while ((1u << s) < v) ++s;
    return s;
}

// Shared argument rules of the four entries (the host forms apply the same ones).
int check_common(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize, const void* packed) {
    if (in_dtype != NF4DQ_F16 && in_dtype != NF4DQ_BF16 && in_dtype != NF4DQ_F32) return NF4DQ_ERR_ARG;
    if (numel < 0 || !nf4q::valid_blocksize(blocksize)) return NF4DQ_ERR_ARG;
    if (numel == 0) return NF4DQ_OK;
    if (!w || !packed) return NF4DQ_ERR_ARG;
    return NF4DQ_OK;
}

int launch_blocks(const void* w, int32_t dt, int64_t numel, int32_t blocksize, uint8_t* packed, float* absmax,
                  hipStream_t st) {
    const int64_t esz = dt == NF4DQ_F32 ? 4 : 2;
    if (!aligned(w, (uintptr_t)esz) || !aligned(absmax, 4)) return NF4DQ_ERR_ARG;
    if (blocksize == 64 && aligned(w, 16) && aligned(packed, 4)) {
        const int64_t g = ((numel + kQTile - 1) / kQTile + kQWaves - 1) / kQWaves;
        if (g > kMaxGrid) return NF4DQ_ERR_TOO_LARGE;
        if (dt == NF4DQ_BF16)
            hipLaunchKernelGGL((nf4_quant_blocks_kernel<NF4DQ_BF16>), dim3((unsigned)g), dim3(kQWg), 0, st, w, numel,
                               packed, absmax);
        else if (dt == NF4DQ_F16)
            hipLaunchKernelGGL((nf4_quant_blocks_kernel<NF4DQ_F16>), dim3((unsigned)g), dim3(kQWg), 0, st, w, numel,
                               packed, absmax);
        else
            hipLaunchKernelGGL((nf4_quant_blocks_kernel<NF4DQ_F32>), dim3((unsigned)g), dim3(kQWg), 0, st, w, numel,
                               packed, absmax);
        return hip_rc(hipGetLastError());
    }
    GeneralArgs A{};
    A.w = w;
    A.numel = numel;
    A.nblk = (numel + blocksize - 1) / blocksize;
    A.packed = packed;
    A.absmax = absmax;
    A.bs_shift = ilog2((uint32_t)blocksize);
    const int64_t g = (A.nblk + kQWaves - 1) / kQWaves;
    if (g > kMaxGrid) return NF4DQ_ERR_TOO_LARGE;
    if (dt == NF4DQ_BF16)
        hipLaunchKernelGGL((nf4_quant_blocks_general_kernel<NF4DQ_BF16>), dim3((unsigned)g), dim3(kQWg), 0, st, A);
    else if (dt == NF4DQ_F16)
        hipLaunchKernelGGL((nf4_quant_blocks_general_kernel<NF4DQ_F16>), dim3((unsigned)g), dim3(kQWg), 0, st, A);
    else
        hipLaunchKernelGGL((nf4_quant_blocks_general_kernel<NF4DQ_F32>), dim3((unsigned)g), dim3(kQWg), 0, st, A);
    return hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

size_t nf4_quant_workspace_bytes(int64_t numel, int32_t blocksize) {
    if (numel <= 0 || !nf4q::valid_blocksize(blocksize)) return 0;
    return (size_t)nf4q::ws_bytes((numel + blocksize - 1) / blocksize);
}

int nf4_quant_bnb(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize, void* packed, void* absmax,
                  void* hip_stream) {
    const int rc = check_common(w, in_dtype, numel, blocksize, packed);
    if (rc || numel == 0) return rc;
    if (!absmax) return NF4DQ_ERR_ARG;
    return launch_blocks(w, in_dtype, numel, blocksize, reinterpret_cast<uint8_t*>(packed),
                         reinterpret_cast<float*>(absmax), reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_quant_bnb_nested(const void* w, int32_t in_dtype, int64_t numel, int32_t blocksize, const float* code2,
                         int32_t blocksize2, void* packed, void* absmax_q, void* absmax2, void* offset,
                         void* workspace, size_t workspace_bytes, void* hip_stream) {
    int rc = check_common(w, in_dtype, numel, blocksize, packed);
    if (rc) return rc;
    if (blocksize2 != nf4q::kBlock2) return NF4DQ_ERR_ARG;
    if (numel == 0) return NF4DQ_OK;
    if (!code2 || !absmax_q || !absmax2 || !offset || !workspace) return NF4DQ_ERR_ARG;
    if (!aligned(workspace, 8) || !aligned(absmax2, 4) || !aligned(offset, 4) || !aligned(code2, 4))
        return NF4DQ_ERR_ARG;
    const int64_t nblk = (numel + blocksize - 1) / blocksize;
    if (workspace_bytes < (size_t)nf4q::ws_bytes(nblk)) return NF4DQ_ERR_ARG;
    const int64_t n2 = (nblk + nf4q::kBlock2 - 1) / nf4q::kBlock2;
    if (n2 > kMaxGrid) return NF4DQ_ERR_TOO_LARGE;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    float* am = reinterpret_cast<float*>(workspace);
    double* parts = reinterpret_cast<double*>(reinterpret_cast<uint8_t*>(workspace) + nf4q::ws_absmax_bytes(nblk));
    rc = launch_blocks(w, in_dtype, numel, blocksize, reinterpret_cast<uint8_t*>(packed), am, st);
    if (rc) return rc;
    const nf4q::SumPlan sp = nf4q::sum_plan(nblk);
    hipLaunchKernelGGL(nf4_quant_absmax_sum_kernel, dim3((unsigned)sp.parts), dim3(nf4q::kBlock2), 0, st, am, nblk,
                       sp.chunk, parts);
    rc = hip_rc(hipGetLastError());
    if (rc) return rc;
    hipLaunchKernelGGL(nf4_quant_stats_kernel, dim3((unsigned)n2), dim3(nf4q::kBlock2), 0, st, am, nblk, parts,
                       sp.parts, code2, reinterpret_cast<uint8_t*>(absmax_q), reinterpret_cast<float*>(absmax2),
                       reinterpret_cast<float*>(offset));
    return hip_rc(hipGetLastError());
}

}  // extern "C"
