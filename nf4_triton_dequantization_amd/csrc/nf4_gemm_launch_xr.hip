// nf4_gemm_launch_xr.hip -- launcher of the register-resident kernels (nf4_gemm_xr_kernel / nf4_gemm_xrg_kernel) (instantiates its kernels;
// compiled on its own so that the kernel families build in parallel).
#include "nf4_gemm_launch.h"

namespace nf4gemm {

int NF4_GEMM_FN(launch_xr)(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
              const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st) {
    GemmArgsOf<NF4_GEMM_GRP> A{};
    fill_common(A, count, x, M, K, cfg, workspace);
    A.chunks = (uint32_t)(K / kChunkK);
    A.chunks_per_split = (uint32_t)(cfg.waves * cfg.strips);
    uint32_t strips = 0;
    for (int i = 0; i < count; ++i) {
        K128Mat& m = A.mat[i];
        fill_mat(m, mats[i]);
        m.cg_begin = strips;  // first 16-column strip of the weight in the launch
        m.col_begin = strips * 16u;
        strips += m.N / 16u;
    }
    A.col_groups = strips;
    A.ncols = strips * 16u;
    fill_modes<NF4_GEMM_GRP>(A, mats, count);
    A.per_wg = xr_per_wg(M, strips, cfg, cus, count > 0 ? mats[0].mode : kScaleRef,
                         count > 0 ? group_tables(mats, count) : 0);
    const LaunchShape ls = launch_shape(cfg, M, K, mats, count, cus);
    const uint32_t ks = A.ksplit, lds = ls.dyn;
    const dim3 grid(ls.grid), block(ls.block);
    // <8 waves, 256-deep chunks, depth 2> with two K slices and at most 4 or 8 reduction
    // groups (8 or 16 strips) per workgroup: the groups unrolled (GU), exchanges issued
    // inside the loop
    const int gu = cfg.waves != 16 && cfg.strips == 2 && cfg.depth != 4 && ks == 2 && A.per_wg <= 16
                       ? (A.per_wg <= 8 ? 4 : 8)
                       : 0;
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(dtype, [&](auto DT) {
        pick<2, 1>(M > 16 ? 2 : 1, [&](auto MT) {
            pick<16, 8>(cfg.strips == 4 ? 8 : cfg.waves, [&](auto W) {
                pick<4, 2, 1>(cfg.strips, [&](auto KPW) {
                    if constexpr (W == 8 || KPW != 4)  // two 256-deep chunks per wave: 8 waves only
                        pick<4, 2>(cfg.depth, [&](auto D) {
                            pick<4, 8, 0>(gu, [&](auto GU) {
                                if constexpr (GU == 0 || (W == 8 && KPW == 2 && D == 2)) {
                                    pick<NF4_GEMM_MODES>(count > 0 ? mats[0].mode : kScaleRef, [&](auto SM) {
                                        const uint32_t cap = kLdsPerCu - xr_lds_static(KPW, SM);
                                        // both templates are instantiated for every GU, as ever
                                        constexpr auto xrg = &nf4_gemm_xrg_kernel<DT, MT, W, KPW, D, GU, SM, NF4_GEMM_GRP>;
                                        constexpr auto xr = &nf4_gemm_xr_kernel<DT, MT, W, KPW, D, GU, SM, NF4_GEMM_GRP>;
                                        if (GU) launch_lds<xrg>(cap, grid, block, lds, st, A);
                                        else launch_lds<xr>(cap, grid, block, lds, st, A);
                                        rc = hip_rc2(hipGetLastError());
                                    });
                                }
                            });
                        });
                });
            });
        });
    });
    return rc;
}

}  // namespace nf4gemm
