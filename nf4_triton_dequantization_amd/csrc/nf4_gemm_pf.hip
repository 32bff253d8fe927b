// nf4_gemm_pf.hip -- the prefill fused NF4 dequant + GEMM in bitsandbytes semantics for 1..8192
// rows (nf4_gemm_bnb_pf, nf4_gemm_bnb_pf_single): kernel, launcher and C entries.  The plan --
// validation, cfg, geometry, LDS, workspace -- is nf4_gemm_pf_plan.h.
//
// y[M][N] = x[M][K] . W[N][K]^T with W the 16-bit weights nf4_dequant_bnb writes, bit for bit.
// The row-tiled family (nf4_gemm_mt_dev.h) keeps all rows of x in LDS and lets every wave decode
// its own weights in registers: right up to 128 rows, where the decode is paid once.  Past that
// the split turns round:
//  * a workgroup of WV waves (4 / 8) owns BM = 32 WV rows (128 / 256), 128 columns and one K
//    slice, a wave 64 x 64 of it as 4 x 4 MFMA tiles of 16 x 16 (f32_16x16x32): 64 accumulator
//    registers that live for the whole K loop;
//  * K moves in steps of 64: one statistics block per weight row, so a thread decodes with ONE
//    scale.  Per step the workgroup loads the 128 x 32 packed bytes of its tile (16 bytes per
//    thread under 4 waves, 8 under 8), and every thread decodes its piece once -- mt_decode's
//    arithmetic: fp32 product of code and block scale, RNE to 16 bits, the oracle's weight --
//    and writes it to the LDS buffer [128][64] as the 16-byte slots the MFMA fragments are read
//    from.  A weight is decoded once per workgroup and step, whatever BM is; no lane shuffles;
//  * x goes the same way: BM x 64 values per step as 16-byte global loads, four per thread;
//  * a staged row (of x or of weights) is 128 bytes, eight 16-byte slots, slot q holding k = 8q ..
//    8q + 7 of the step, stored rotated by (row >> 1) & 3 slots.  Lane (nl, kh) of an MFMA
//    fragment reads slot 4 (kh & 1) + 2 (kh >> 1) + s in MFMA step s (the same permutation of k
//    on both operands, so the sum is the plain one).  A ds_read_b128 is served in groups of 16
//    lanes made of rows 0-3 / 12-15 of one kh with rows 4-11 of its pair kh ^ 1: with the slots
//    of a pair four apart and the rotation, the 16 lanes of a group fall on 16 different slots
//    of the two 256-byte bank rows they touch;
//  * two buffers each for x and the weights, ONE barrier per step.  Global loads run two steps
//    ahead in two register sets and land -- decoded -- in the other buffer behind the current
//    step's MFMAs;
//  * the weight fragment is the MFMA's A operand and the x fragment its B operand, so a lane
//    holds FOUR CONSECUTIVE COLUMNS of one row of y: one 8-byte store per tile, 16-byte stores
//    to the slab.
// Rows of a block past M repeat row M - 1 (an in-bounds load, no branch) and are never stored;
// steps past the slice's end repeat its last step into a buffer nobody reads.
// Split-K is the family's: fp32 slab per slice, one ticket per (row block, column tile) drawn
// through mt_publish_last; the workgroup drawing the last ticket sums the slabs in slice order
// (the first slice assigns), stores y and puts the slab back to 0.  No poll, no float atomics.
// The result is a function of the inputs and the cfg alone, and a row's bits do not depend on
// the rows around it: the k order of a row's sum is fixed by the cfg.
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_pf_plan.h"

namespace {

struct PfArgs {
    const uint8_t* packed;  // [N][K/2]
    const uint8_t* a1;      // nested: absmax bytes [N K / 64]
    const float* a2;        // nested: absmax2; single: the fp32 absmax
    const float* code2;     // nested: [256]
    const float* offset;    // nested: [1] or null (= 0)
    const void* x;          // [M][K]
    void* y;                // [M][N]
    float* slab;            // [ksplit][M][N] (ksplit > 1)
    uint32_t* counters;     // one ticket per (row block, column tile)
    uint32_t M, N, K;
    uint32_t ksplit, sps, steps, tiles;  // K slices, steps per slice, K / 64, N / 128
    uint32_t sh2;           // log2(blocksize2)
};

// Slot rotation of a staged row (see the header comment).
__device__ __forceinline__ uint32_t pf_rot(uint32_t row) { return (row >> 1) & 3u; }

// The reducer of one (row block, column tile): `live` rows of 32 float4, four elements per
// thread in flight per slice, each element summed in slice order, cleared behind the sum.
// Elements past the tile repeat its last one (an in-bounds load, no branch) and are not stored.
template <int DT, int WV>
__device__ inline void pf_reduce(const PfArgs& A, uint32_t row0, uint32_t live, uint32_t col0) {
    constexpr uint32_t T = 64u * WV, kE = 4;
    const uint32_t total = live * (kPfCols / 4u), plane = A.M * A.N;  // < 2^30 floats: validated
    for (uint32_t b0 = 0; b0 < total; b0 += kE * T) {  // (a workgroup-uniform trip count)
        const uint32_t base = b0 + threadIdx.x;
        uint32_t at[kE];
        f32x4 sum[kE];
#pragma unroll
        for (uint32_t j = 0; j < kE; ++j) {
            const uint32_t e0 = base + j * T, e = e0 < total ? e0 : total - 1u;
            at[j] = (row0 + e / (kPfCols / 4u)) * A.N + col0 + 4u * (e % (kPfCols / 4u));
        }
        for (uint32_t sl = 0; sl < A.ksplit; ++sl) {
            f32x4 v[kE];
#pragma unroll
            for (uint32_t j = 0; j < kE; ++j) v[j] = *reinterpret_cast<const f32x4*>(A.slab + sl * plane + at[j]);
#pragma unroll
            for (uint32_t j = 0; j < kE; ++j) {
                if (sl == 0u) sum[j] = v[j];  // the first slice starts the sum: -0 stays -0
                else {
                    sum[j].x += v[j].x;
                    sum[j].y += v[j].y;
                    sum[j].z += v[j].z;
                    sum[j].w += v[j].w;
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kE; ++j)
            if (base + j * T < total) {
                for (uint32_t sl = 0; sl < A.ksplit; ++sl)
                    *reinterpret_cast<f32x4*>(A.slab + sl * plane + at[j]) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + at[j]) =
                    u32x2{pack2<DT>(sum[j].x, sum[j].y), pack2<DT>(sum[j].z, sum[j].w)};
            }
    }
}

// (two waves per SIMD: two 128-row workgroups or one 256-row workgroup on a CU; without the
// bound the 4-wave form takes 320 registers and a CU holds one workgroup of it)
template <int DT, int SM, int WV>
__global__ __launch_bounds__(64 * WV, 2) void nf4_gemm_pf_kernel(const PfArgs A) {
    constexpr uint32_t T = 64u * WV, BM = 32u * WV;
    constexpr uint32_t kXBuf = BM * kPfRowBytes, kWBuf = kPfCols * kPfRowBytes;
    constexpr int NP = 4;                    // 16-byte pieces of x per thread and step: BM * 8 / T
    constexpr uint32_t WP = T / kPfCols;     // threads per weight row: 2 / 4
    constexpr int WD = 8 / (int)WP;          // packed dwords per thread and step: 4 / 2
    static_assert(BM * 8u == NP * T && WP * WD == 8, "a step divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x 0][x 1][w 0][w 1][code2][codes][flag]
    char* xs = smem;
    char* ws = smem + 2u * kXBuf;
    float* c2tab = reinterpret_cast<float*>(ws + 2u * kWBuf);
    float* lut = c2tab + 256;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t wr = wave >> 1, wc = wave & 1u;  // the wave's 64 x 64 of the tile
    const uint32_t ks = blockIdx.x % A.ksplit, rest = blockIdx.x / A.ksplit;
    const uint32_t tile = rest % A.tiles, rb = rest / A.tiles;
    const uint32_t row0 = rb * BM, col0 = tile * kPfCols;

    if constexpr (SM == kScaleBnb)
        for (uint32_t i = tid; i < 256u; i += T) c2tab[i] = A.code2[i];
    write_lut(lut);
    const float off = load_offset<SM>(A.offset);

    const uint32_t s_begin = ks * A.sps < A.steps ? ks * A.sps : A.steps;
    const uint32_t s_end = s_begin + A.sps < A.steps ? s_begin + A.sps : A.steps;
    const uint32_t n = s_end - s_begin;  // steps of this slice
    auto step_at = [&](uint32_t i) { return s_begin + (i < n ? i : n - 1u); };

    // what a thread moves per step: NP pieces of x, WD packed dwords of weight row wn with their block's statistics
    const uint32_t wn = tid / WP, wh = tid % WP;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;
    u32x4 xr[2][NP];
    uint32_t wq[2][WD], qa[2];
    float qb[2];
    auto load = [&](auto S, uint32_t st) {
        const char* xg = reinterpret_cast<const char*>(A.x);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t p = tid + (uint32_t)i * T, row = p >> 3, seg = p & 7u;
            const uint32_t r = row0 + row < A.M ? row0 + row : A.M - 1u;  // past M: row M - 1 again, never stored
            xr[S][i] = *reinterpret_cast<const u32x4*>(xg + (r * A.K + st * kPfStepK + seg * 8u) * 2u);  // < 2^31: validated
        }
        const uint8_t* wp = A.packed + ((col0 + wn) * kb + st * 32u + wh * (4u * WD));  // < 2^31: validated
        if constexpr (WD == 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(wp);
            wq[S][0] = v.x, wq[S][1] = v.y, wq[S][2] = v.z, wq[S][3] = v.w;
        } else {
            const u32x2 v = *reinterpret_cast<const u32x2*>(wp);
            wq[S][0] = v.x, wq[S][1] = v.y;
        }
        const uint32_t f = (col0 + wn) * bpr + st;  // 64-block on the weight's flat stream
        if constexpr (SM == kScaleBnb) {
            qa[S] = A.a1[f];
            qb[S] = A.a2[f >> A.sh2];
        } else {
            qa[S] = 0u;
            qb[S] = A.a2[f];
        }
    };
    const char* t = reinterpret_cast<const char*>(lut);
    auto store = [&](auto S, uint32_t b) {
        char* xb = xs + b * kXBuf;
        char* wb = ws + b * kWBuf;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t p = tid + (uint32_t)i * T, row = p >> 3, seg = p & 7u;
            *reinterpret_cast<u32x4*>(xb + row * kPfRowBytes + ((seg + pf_rot(row)) & 7u) * 16u) = xr[S][i];
        }
        const float sc = block_scale<SM>(c2tab, qa[S], qb[S], off);
#pragma unroll
        for (int d = 0; d < WD; ++d)
            *reinterpret_cast<u32x4*>(wb + wn * kPfRowBytes + ((wh * WD + (uint32_t)d + pf_rot(wn)) & 7u) * 16u) =
                mt_decode<DT>(t, wq[S][d], sc);
    };

    f32x4 acc[4][4];  // [x row tile][column tile]
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    if (n > 0u) {
        load(I0{}, step_at(0));
        load(I1{}, step_at(1));
    }
    __syncthreads();  // the tables
    if (n > 0u) {
        store(I0{}, 0u);
        load(I0{}, step_at(2));
    }
    __syncthreads();  // the first stage

    const uint32_t q0 = 4u * (kh & 1u) + 2u * (kh >> 1) + pf_rot(nl);  // row 16 t + nl: the rotation depends on nl alone
    const uint32_t wfrag = (wc * 64u + nl) * kPfRowBytes, xfrag = (wr * 64u + nl) * kPfRowBytes;
    // step i of the slice (J = i & 1): its x and weights are in buffer J, step i + 1 in register
    // set J ^ 1 (landed or in flight), step i + 2 in set J (in flight)
    auto step = [&](auto J, uint32_t i) {
        constexpr int j = decltype(J)::value;
        const char* xb = xs + (uint32_t)j * kXBuf + xfrag;
        const char* wb = ws + (uint32_t)j * kWBuf + wfrag;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t slot = ((q0 + (uint32_t)s) & 7u) * 16u;
            u32x4 a[4], b[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) a[ct] = *reinterpret_cast<const u32x4*>(wb + 16u * ct * kPfRowBytes + slot);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) b[mt] = *reinterpret_cast<const u32x4*>(xb + 16u * mt * kPfRowBytes + slot);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = mt_mfma<DT>(a[ct], b[mt], acc[mt][ct]);
            // one set of fragments live at a time: two waves per SIMD hide the reads, and both sets
            // together put the 8-wave form past its 256 registers
            __builtin_amdgcn_sched_barrier(0);
        }
        // step i + 1 (loaded two steps ago) into the other buffer, last read one barrier ago; its
        // registers then take step i + 3
        store(std::integral_constant<int, j ^ 1>{}, (uint32_t)(j ^ 1));
        load(std::integral_constant<int, j ^ 1>{}, step_at(i + 3u));
        __syncthreads();
    };
    for (uint32_t i = 0; i < n; i += 2u) {
        step(I0{}, i);
        if (i + 1u >= n) break;
        step(I1{}, i + 1u);
    }

    // acc[mt][ct][i] is y[row0 + 64 wr + 16 mt + nl][col0 + 64 wc + 16 ct + 4 kh + i]
    const uint32_t ycol = col0 + wc * 64u + 4u * kh;
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const uint32_t m = row0 + wr * 64u + 16u * mt + nl;
            if (m < A.M)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + m * A.N + ycol + 16u * ct) =
                        u32x2{pack2<DT>(acc[mt][ct].x, acc[mt][ct].y), pack2<DT>(acc[mt][ct].z, acc[mt][ct].w)};
        }
        return;
    }
    float* mine = A.slab + ks * (A.M * A.N);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const uint32_t m = row0 + wr * 64u + 16u * mt + nl;
        if (m < A.M)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<f32x4*>(mine + m * A.N + ycol + 16u * ct) = acc[mt][ct];
    }
    if (mt_publish_last(A.counters + rb * A.tiles + tile, A.ksplit, flag))
        pf_reduce<DT, WV>(A, row0, (A.M - row0 < BM ? A.M - row0 : BM), col0);
}

template <int SM>
int launch_pf(const nf4gemm::MtCall& a, const nf4_gemm_cfg& cfg, const float* offset, hipStream_t st) {
    const PfPlan p = pf_plan(cfg, a.M, a.N, a.K);
    PfArgs A{};
    A.packed = a.packed;
    A.a1 = a.a1;
    A.a2 = a.a2;
    A.code2 = a.code2;
    A.offset = offset;
    A.x = a.x;
    A.y = a.y;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.M = (uint32_t)a.M;
    A.N = (uint32_t)a.N;
    A.K = (uint32_t)a.K;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.sps = p.sps;
    A.steps = p.steps;
    A.tiles = p.tiles;
    A.sh2 = mt_log2_blocksize2(a.single, a.blocksize2);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<8, 4>(cfg.waves, [&](auto WV) {
            launch_lds<&nf4_gemm_pf_kernel<DT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
            rc = hip_rc2(hipGetLastError());
        });
    });
    return rc;
}

int gemm_pf_impl(const nf4gemm::MtCall& a, const float* offset, hipStream_t st) {
    nf4_gemm_cfg cfg{};
    bool launch = false;
    const int rc = pf_check(a, device_cus(), &cfg, &launch);
    if (rc || !launch) return rc;
    return a.single ? launch_pf<kScaleBnbSingle>(a, cfg, nullptr, st) : launch_pf<kScaleBnb>(a, cfg, offset, st);
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_pf_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg) {
    nf4_gemm_cfg c = cfg ? *cfg : pf_default_cfg(M, N, K, device_cus());
    if (cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_PF;
    return valid_pf_cfg(c, M, N, K) ? pf_workspace_need(M, N, K, c) : 0;
}

int nf4_gemm_bnb_pf(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                    int64_t nb, const float* code2, const float* absmax2, int64_t n2, const float* offset,
                    int32_t blocksize, int32_t blocksize2, void* y, int32_t out_dtype, int64_t N, int64_t K,
                    void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{false, x,          M, packed,    packed_len, absmax_q,  nb, code2,           absmax2, n2,
                            blocksize, blocksize2, y, out_dtype, N,          K,         workspace, workspace_bytes, cfg};
    return gemm_pf_impl(a, offset, reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_bnb_pf_single(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const float* absmax,
                           int64_t nabs, int32_t blocksize, void* y, int32_t out_dtype, int64_t N, int64_t K,
                           void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{true,      x, M, packed,    packed_len, nullptr, nabs, nullptr,   absmax,          nabs,
                            blocksize, 1, y, out_dtype, N,          K,       workspace, workspace_bytes, cfg};
    return gemm_pf_impl(a, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
