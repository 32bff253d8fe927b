// nf4_gemm_mt_swiglu.hip -- the fused gate/up SwiGLU launch in bitsandbytes semantics for
// 1..128 rows (nf4_gemm_bnb_mt_swiglu): kernel, launcher and C entries.  The plan --
// validation, cfg, geometry, LDS, workspace -- is nf4_gemm_mt_swiglu_plan.h; the device
// pipeline is nf4_gemm_mt_dev.h.
//
// h[M][I] = silu(g) * u with g = x . Wg^T and u = x . Wu^T what nf4_gemm_bnb_mt stores for each
// weight (fp32 accumulation, one RNE to 16 bits), and the rounding chain of
// `F.silu(gate(x)) * up(x)` on 16-bit tensors behind them:
//   s = RNE16(g / (1 + expf(-g)))   fp32, IEEE division        h = RNE16(s * u)   fp32 product
// The pipeline runs with dense rows and the wave's two strips given to the two weights:
//  * a workgroup (WV waves) owns 16 WV columns of h, ALL MT row tiles and one K slice;
//  * a wave owns 16 columns of h: strip 0 is rows col .. col + 15 of the gate weight, strip 1
//    the same rows of the up weight, each with its own statistics, code2 table (two tables in
//    LDS), offset and blocksize2.  acc[mt][0][i] and acc[mt][1][i] are g and u of ONE output
//    element in one lane, so the one-slice epilogue is lane-local and the register budget the
//    row-tiled kernel's.
// Split-K: every slice stores both fp32 planes to its slab ([ksplit][2][M][I]); the last slice
// sums each plane in slice order and applies the chain to four columns at a time.
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_mt_swiglu_plan.h"

namespace {

struct SgArgs {
    const uint8_t* packed[2];  // gate, up: [I][K/2]
    const uint8_t* a1[2];      // nested: absmax bytes [I K / 64]
    const float* a2[2];        // nested: absmax2; single: the fp32 absmax
    const float* code2[2];     // nested: [256]
    const float* offset[2];    // nested: [1] or null (= 0)
    const void* x;             // [M][K]
    void* h;                   // [M][I]
    float* slab;               // [ksplit][2][M][I] (ksplit > 1)
    uint32_t* counters;        // one ticket per column tile
    uint32_t M, I, K;
    uint32_t ksplit, cps, chunks;  // K slices, chunks per slice, K / 128
    uint32_t sh2[2];           // log2(blocksize2)
};

// (the chain -- rne16, swiglu16 -- and the two-plane output policy SgOut are nf4_gemm_mt_dev.h's:
// the expert SwiGLU launch, nf4_gemm_moe_swiglu.hip, uses the same ones)
template <int DT, int MT, int SM, int WV>
__global__ __launch_bounds__(64 * WV) void nf4_gemm_mt_swiglu_kernel(const SgArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2 gate][code2 up][codes][flag]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * 16u * MT * kMtRowBytes);
    float* lut = c2tab + 512;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);
    const uint32_t ks = blockIdx.x % A.ksplit, tile = blockIdx.x / A.ksplit;

    if constexpr (SM == kScaleBnb)
        for (uint32_t i = threadIdx.x; i < 256u; i += 64u * WV) {
            c2tab[i] = A.code2[0][i];
            c2tab[256u + i] = A.code2[1][i];
        }
    write_lut(lut);
    const MtStrips<2> st{{A.packed[0], A.packed[1]}, {A.a1[0], A.a1[1]}, {A.a2[0], A.a2[1]}, c2tab,
                         {load_offset<SM>(A.offset[0]), load_offset<SM>(A.offset[1])}, {A.sh2[0], A.sh2[1]}};
    const MtJob job{A.x, A.h, A.slab, A.counters + tile, smem, lut, flag, A.M, A.I, A.K, tile, ks, A.ksplit, A.cps, A.chunks};
    mt_pipeline<DT, MT, SM, WV, /*SB=*/true, SgOut<DT>>(job, MtDenseRows{A.M}, st);
}

template <int SM>
int launch_sg(const nf4gemm::SgCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const int64_t I = a.mats[0].N;
    const MtPlan p = sg_plan(cfg, a.M, I, a.K);
    SgArgs A{};
    for (int i = 0; i < 2; ++i) {
        const nf4_gemm_bnb_mat& m = a.mats[i];
        A.packed[i] = m.packed;
        A.a1[i] = a.single ? nullptr : m.absmax_q;
        A.a2[i] = m.absmax2;
        A.code2[i] = a.single ? nullptr : m.code2;
        A.offset[i] = a.single ? nullptr : m.offset;
        A.sh2[i] = mt_log2_blocksize2(a.single, m.blocksize2);
    }
    A.x = a.x;
    A.h = a.h;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.M = (uint32_t)a.M;
    A.I = (uint32_t)I;
    A.K = (uint32_t)a.K;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.cps = p.cps;
    A.chunks = p.chunks;
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_mt_swiglu_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_mt_swiglu_workspace_bytes(int64_t M, int64_t I, int64_t K, const nf4_gemm_cfg* cfg) {
    return sg_workspace_need(M, I, K, cfg ? *cfg : sg_default_cfg(M, I, K, device_cus()));
}

int nf4_gemm_bnb_mt_swiglu(const void* x, int64_t M, int64_t K, const void* gate_up, int32_t single, int32_t act,
                           void* h, int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                           void* hip_stream) {
    const nf4gemm::SgCall a{single != 0, x,         M,         K,               reinterpret_cast<const nf4_gemm_bnb_mat*>(gate_up),
                            act,         h,         out_dtype, workspace,       workspace_bytes,
                            cfg};
    nf4_gemm_cfg c{};
    const int rc = sg_check(a, device_cus(), &c);
    if (rc) return rc;
    const hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.single ? launch_sg<kScaleBnbSingle>(a, c, st) : launch_sg<kScaleBnb>(a, c, st);
}

}  // extern "C"
