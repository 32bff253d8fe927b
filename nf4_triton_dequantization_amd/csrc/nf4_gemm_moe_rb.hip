// nf4_gemm_moe_rb.hip -- the fused NF4 expert GEMM in row blocks of 128 listed rows
// (nf4_gemm_bnb_moe_rb: up to NF4DQ_MOE_RB_MAX_PAIRS pairs in one capturable launch): launcher
// and C entries.  The kernel is nf4_gemm_moe_dev.h's template with RB = true (DOWN false, W 1);
// the plan -- validation, cfg, geometry, LDS, workspace -- is nf4_gemm_moe_rb_plan.h.
#include "nf4_gemm_moe_dev.h"
#include "nf4_gemm_moe_rb_plan.h"

namespace {

template <int SM>
int launch_moe_rb(const nf4gemm::MoeCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& e = *a.ex;
    const MoeRbPlan p = moe_rb_plan(cfg, a.P, e.experts, e.N, e.K);
    // (the fill reads the plan's tiles, chunks and chunks per slice: the expert GEMM's fields)
    const MoePlan g{p.grid, p.block, p.dyn, p.tiles, p.chunks, p.cps, p.row_tiles, p.tickets};
    const MoeArgsT<1> A = moe_fill<1>(a, a.y, g, cfg);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_moe_kernel<DT, MT, SM, WV, false, 1, true>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_rb_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg) {
    if (!experts) return 0;
    const nf4_moe_experts& e = *reinterpret_cast<const nf4_moe_experts*>(experts);
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return moe_rb_workspace_need(P, e.N, e.K, cfg ? *cfg : moe_rb_default_cfg(P, e.experts, e.N, e.K, device_cus()));
}

int nf4_gemm_bnb_moe_rb(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts, void* y,
                        int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                        void* hip_stream) {
    const nf4gemm::MoeCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(experts), y, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_rb_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex->single ? launch_moe_rb<kScaleBnbSingle>(a, c, st) : launch_moe_rb<kScaleBnb>(a, c, st);
}

}  // extern "C"
