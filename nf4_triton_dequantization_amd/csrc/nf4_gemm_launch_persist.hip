// nf4_gemm_launch_persist.hip -- launcher of the persistent kernel (nf4_gemm_persist_kernel) (instantiates its kernels;
// compiled on its own so that the kernel families build in parallel).
#include "nf4_gemm_launch.h"

namespace nf4gemm {

// One launch of the persistent kernel over `count` weights sharing x (cfg
// validated per weight and known to run: cfg_runs).  Grid: persist_grid.
int NF4_GEMM_FN(launch_persist)(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                   const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st) {
    StreamArgsOf<NF4_GEMM_GRP> S{};
    fill_common(S, count, x, M, K, cfg, workspace);
    S.T = (uint32_t)cfg.strips;
    S.parts = (uint32_t)(cfg.waves / cfg.strips);
    S.chunks = (uint32_t)(K / kSChunkK);
    S.cps = S.chunks / S.ksplit;
    S.cpp = S.cps / S.parts;
    S.ppr = make_fastdiv(S.cps * 32u);
    S.xstride = S.cps * 512u + 16u;
    uint32_t sg = 0, strips = 0;
    for (int i = 0; i < count; ++i) {
        StreamMat& m = S.mat[i];
        fill_mat(m, mats[i]);
        m.sg_begin = sg;
        m.strip_begin = strips;
        m.nb_bytes = m.nb.d;
        m.n2_bytes = m.n2.d * 4u;
        sg += (uint32_t)(mats[i].N / (16 * cfg.strips));
        strips += (uint32_t)(mats[i].N / 16);
    }
    S.sg_total = sg;
    S.ncols = strips * 16u;
    if (NF4_GEMM_GRP || (count == 1 && mats[0].mode != kScaleRef)) fill_modes<NF4_GEMM_GRP>(S, mats, count);
    if (cfg_runs(cfg, M, K, mats, count, cus) != NF4DQ_OK) return NF4DQ_ERR_ARG;  // not a plan
    const PersistGrid g = persist_grid(M, K, cfg, sg, cus);
    S.zero_off = g.zero_off;
    S.red_off = g.red_off;
    S.out_off = g.out_off;
    const dim3 grid(g.G), block(64 * cfg.waves);
    pick<NF4DQ_BF16, NF4DQ_F16>(dtype, [&](auto DT) {
        pick<4, 8, 16>(cfg.waves, [&](auto W) {
            pick<2, 4>(cfg.depth, [&](auto P) {
                pick<true, false>(S.ksplit > 1, [&](auto SPLIT) {
                    pick<NF4_GEMM_MODES>(count > 0 ? mats[0].mode : kScaleRef, [&](auto SM) {
                        launch_lds<&nf4_gemm_persist_kernel<DT, W, P, SPLIT, SM, NF4_GEMM_GRP>>(kStreamLdsCap, grid, block, g.dyn, st,
                                                                                   S);
                    });
                });
            });
        });
    });
    return hip_rc2(hipGetLastError());
}

}  // namespace nf4gemm
