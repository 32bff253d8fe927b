// nf4_gemm_launch_k128.hip -- launcher of the 128-deep kernel (nf4_gemm_smallm_kernel) (instantiates its kernels;
// compiled on its own so that the kernel families build in parallel).
#include "nf4_gemm_launch.h"

namespace nf4gemm {

// One launch of the 128-deep kernel over `count` weights sharing x (shapes and cfg
// validated; an empty weight owns no column group).
int NF4_GEMM_FN(launch_k128)(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st) {
    const int nt = cfg.strips > 1 ? cfg.strips : 1;  // 16-column strips per wave
    GemmArgsOf<NF4_GEMM_GRP> A{};
    fill_common(A, count, x, M, K, cfg, workspace);
    A.chunks = (uint32_t)(K / kChunkK);
    A.chunks_per_split = (A.chunks + A.ksplit - 1) / A.ksplit;
    uint32_t cgs = 0, cols = 0;
    for (int i = 0; i < count; ++i) {
        K128Mat& m = A.mat[i];
        fill_mat(m, mats[i]);
        m.cg_begin = cgs;
        m.col_begin = cols;
        cgs += m.N / (16u * (uint32_t)nt);
        cols += m.N;
    }
    A.col_groups = cgs;
    A.ncols = cols;
    fill_modes<NF4_GEMM_GRP>(A, mats, count);
    const LaunchShape ls = launch_shape(cfg, M, K, mats, count, cus);
    const bool vs = ls.dyn != 0;  // the scale table in LDS: the vector-scale form
    const dim3 grid(ls.grid), block(ls.block);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(dtype, [&](auto DT) {
        pick<1, 2>((int)((M + 15) / 16), [&](auto MT) {
            pick<4, 2, 1>(cfg.depth, [&](auto D) {
                if constexpr (MT == 1 || D != 4)  // two row tiles: at most 2 chunks in flight
                    pick<8, 4>(cfg.waves, [&](auto W) {
                        pick<4, 2, 1>(nt, [&](auto NT) {
                            pick<NF4_GEMM_MODES>(count > 0 ? mats[0].mode : kScaleRef, [&](auto SM) {
                                constexpr auto scales_in_lds = &nf4_gemm_smallm_kernel<DT, MT, D, W, NT, true, SM, NF4_GEMM_GRP>;
                                constexpr auto scales_gathered = &nf4_gemm_smallm_kernel<DT, MT, D, W, NT, false, SM, NF4_GEMM_GRP>;
                                if (vs) hipLaunchKernelGGL(scales_in_lds, grid, block, ls.dyn, st, A);
                                else hipLaunchKernelGGL(scales_gathered, grid, block, 0, st, A);
                                rc = hip_rc2(hipGetLastError());
                            });
                        });
                    });
            });
        });
    });
    return rc;
}

}  // namespace nf4gemm
