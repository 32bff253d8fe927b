// nf4_gemm_launch_xs.hip -- launcher of the shared-activation kernel (nf4_gemm_xs_kernel) (instantiates its kernels;
// compiled on its own so that the kernel families build in parallel).
#include "nf4_gemm_launch.h"

namespace nf4gemm {

// One launch of the shared-activation kernel over `count` weights sharing x (shapes
// and cfg validated: cfg.depth = KC chunks per slice, cfg.ksplit = ceil(chunks / KC)).
int launch_xs(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
              const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st) {
    GemmArgs A{};
    fill_common(A, count, x, M, K, cfg, workspace);
    A.chunks = (uint32_t)(K / kChunkK);
    A.chunks_per_split = (uint32_t)cfg.depth;
    const uint32_t cols_per_group = 16u * (uint32_t)cfg.waves;
    uint32_t cgs = 0, cols = 0;
    for (int i = 0; i < count; ++i) {
        K128Mat& m = A.mat[i];
        fill_mat(m, mats[i]);
        m.cg_begin = cgs;
        m.col_begin = cols;
        cgs += (m.N + cols_per_group - 1u) / cols_per_group;
        cols += m.N;
    }
    A.col_groups = cgs;
    A.ncols = cols;
    const LaunchShape ls = launch_shape(cfg, M, K, mats, count, cus);
    const dim3 grid(ls.grid), block(ls.block);
    pick<NF4DQ_BF16, NF4DQ_F16>(dtype, [&](auto DT) {
        pick<2, 1>(M > 16 ? 2 : 1, [&](auto MT) {
            pick<8, 4, 2>(cfg.depth, [&](auto KC) {
                pick<8, 4>(cfg.waves, [&](auto W) {
                    launch_lds<&nf4_gemm_xs_kernel<DT, MT, KC, W>>(kLdsPerCu, grid, block, ls.dyn, st, A);
                });
            });
        });
    });
    return hip_rc2(hipGetLastError());
}

}  // namespace nf4gemm
