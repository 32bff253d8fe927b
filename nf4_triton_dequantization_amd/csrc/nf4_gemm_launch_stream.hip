// nf4_gemm_launch_stream.hip -- launcher of the streaming kernel (nf4_gemm_stream_kernel) (instantiates its kernels;
// compiled on its own so that the kernel families build in parallel).
#include "nf4_gemm_launch.h"

namespace nf4gemm {

// One launch of the streaming kernel over `count` weights sharing x (shapes and
// cfg already validated; workspace = counters + ksplit * M * sum(N) / 2 64-bit slab entries).
int launch_stream(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                  const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st) {
    const StreamPlan pl = stream_plan(M, K, cfg);
    StreamArgs S{};
    fill_common(S, count, x, M, K, cfg, workspace);
    S.T = (uint32_t)cfg.strips;
    S.parts = (uint32_t)(cfg.waves / cfg.strips);
    S.chunks = (uint32_t)(K / kSChunkK);
    S.cps = pl.cps;
    S.cpp = (pl.cps + S.parts - 1) / S.parts;
    S.ppr = make_fastdiv(pl.cps * 32u);
    S.xstride = pl.xstride;
    S.zero_off = pl.zero_off;
    S.red_off = pl.red_off;
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
    // vector scales: no absmax wrap inside any row of any weight, and each wave's chunks <= kVsMax
    const bool vs = S.cpp <= (uint32_t)kVsMax && no_wrap_in_row(mats, count, K);
    const LaunchShape ls = launch_shape(cfg, M, K, mats, count, cus);
    const dim3 grid(ls.grid), block(ls.block);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(dtype, [&](auto DT) {
        pick<1, 2>((int)((M + 15) / 16), [&](auto MT) {
            pick<4, 8, 16>(cfg.waves, [&](auto W) {
                pick<2, 4, 8>(cfg.depth, [&](auto P) {
                    // 16 waves only for one row tile, and never 8 chunks deep
                    if constexpr (W != 16 || (MT == 1 && P != 8))
                        pick<true, false>(vs, [&](auto VS) {
                            constexpr auto kernel = &nf4_gemm_stream_kernel<DT, MT, W, P, VS>;
                            launch_lds<kernel>(kStreamLdsCap, grid, block, ls.dyn, st, S);
                            rc = hip_rc2(hipGetLastError());
                        });
                });
            });
        });
    });
    return rc;
}

}  // namespace nf4gemm
