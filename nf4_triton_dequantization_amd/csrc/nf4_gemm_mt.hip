// nf4_gemm_mt.hip -- the row-tiled fused NF4 dequant + GEMM in bitsandbytes semantics for
// 33..128 rows (nf4_gemm_bnb_mt, nf4_gemm_bnb_mt_single): kernel, launcher and C entries.
// The plan -- validation, cfg, geometry, LDS, workspace -- is nf4_gemm_mt_plan.h; the device
// pipeline, its anatomy and the reasons for it are nf4_gemm_mt_dev.h.  Here it runs with dense
// rows (staged row r is row r of x and y), two column strips of the one weight per wave (a
// workgroup owns 32 WV columns) and the plain sum as output.
#include "nf4_gemm_mt_dev.h"

namespace {

struct MtArgs {
    const uint8_t* packed;  // [N][K/2]
    const uint8_t* a1;      // nested: absmax bytes [N K / 64]
    const float* a2;        // nested: absmax2; single: the fp32 absmax
    const float* code2;     // nested: [256]
    const float* offset;    // nested: [1] or null (= 0)
    const void* x;          // [M][K]
    void* y;                // [M][N]
    float* slab;            // [ksplit][M][N] (ksplit > 1)
    uint32_t* counters;     // one ticket per column tile
    uint32_t M, N, K;
    uint32_t ksplit, cps, chunks;  // K slices, chunks per slice, K / 128
    uint32_t sh2;           // log2(blocksize2)
};

template <int DT, int MT, int SM, int WV>
__global__ __launch_bounds__(64 * WV) void nf4_gemm_mt_kernel(const MtArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2][codes][flag]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * 16u * MT * kMtRowBytes);
    float* lut = c2tab + 256;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);
    const uint32_t ks = blockIdx.x % A.ksplit, tile = blockIdx.x / A.ksplit;

    if constexpr (SM == kScaleBnb)
        for (uint32_t i = threadIdx.x; i < 256u; i += 64u * WV) c2tab[i] = A.code2[i];
    write_lut(lut);
    const MtStrips<1> st{{A.packed}, {A.a1}, {A.a2}, c2tab, {load_offset<SM>(A.offset)}, {A.sh2}};
    const MtJob job{A.x, A.y, A.slab, A.counters + tile, smem, lut, flag, A.M, A.N, A.K, tile, ks, A.ksplit, A.cps, A.chunks};
    mt_pipeline<DT, MT, SM, WV, /*SB=*/true, MtSumOut<DT>>(job, MtDenseRows{A.M}, st);
}

template <int SM>
int launch_mt(const nf4gemm::MtCall& a, const nf4_gemm_cfg& cfg, const float* offset, hipStream_t st) {
    const MtPlan p = mt_plan(cfg, a.M, a.N, a.K);
    MtArgs A{};
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
    A.cps = p.cps;
    A.chunks = p.chunks;
    A.sh2 = mt_log2_blocksize2(a.single, a.blocksize2);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_mt_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

int gemm_mt_impl(const nf4gemm::MtCall& a, const float* offset, hipStream_t st) {
    nf4_gemm_cfg cfg{};
    const int rc = mt_check(a, device_cus(), &cfg);
    if (rc) return rc;
    return a.single ? launch_mt<kScaleBnbSingle>(a, cfg, nullptr, st) : launch_mt<kScaleBnb>(a, cfg, offset, st);
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_mt_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg) {
    return mt_workspace_need(M, N, K, cfg ? *cfg : mt_default_cfg(M, N, K, device_cus()));
}

int nf4_gemm_bnb_mt(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                    int64_t nb, const float* code2, const float* absmax2, int64_t n2, const float* offset,
                    int32_t blocksize, int32_t blocksize2, void* y, int32_t out_dtype, int64_t N, int64_t K,
                    void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{false, x,          M, packed,    packed_len, absmax_q,  nb, code2,           absmax2, n2,
                            blocksize, blocksize2, y, out_dtype, N,          K,         workspace, workspace_bytes, cfg};
    return gemm_mt_impl(a, offset, reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_bnb_mt_single(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const float* absmax,
                           int64_t nabs, int32_t blocksize, void* y, int32_t out_dtype, int64_t N, int64_t K,
                           void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{true,      x, M, packed,    packed_len, nullptr, nabs, nullptr,   absmax,          nabs,
                            blocksize, 1, y, out_dtype, N,          K,       workspace, workspace_bytes, cfg};
    return gemm_mt_impl(a, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
