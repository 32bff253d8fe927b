// nf4_gemm_moe.hip -- the fused NF4 expert GEMM of a mixture-of-experts block in bitsandbytes
// semantics (nf4_gemm_bnb_moe): launcher and C entries.  The kernel is nf4_gemm_moe_dev.h's
// template with DOWN = false (nf4_gemm_moe_down.hip launches it with DOWN = true); the plan --
// validation, cfg, geometry, LDS, workspace -- is nf4_gemm_moe_plan.h.
#include "nf4_gemm_moe_dev.h"

namespace {

template <int SM>
int launch_moe(const nf4gemm::MoeCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& e = *a.ex;
    const MoePlan p = moe_plan(cfg, a.P, e.experts, e.N, e.K);
    const MoeArgsT<1> A = moe_fill<1>(a, a.y, p, cfg);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_moe_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg) {
    if (!experts) return 0;
    const nf4_moe_experts& e = *reinterpret_cast<const nf4_moe_experts*>(experts);
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return moe_workspace_need(P, e.N, e.K, cfg ? *cfg : moe_default_cfg(P, e.experts, e.N, e.K, device_cus()));
}

int nf4_gemm_bnb_moe(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts, void* y,
                     int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                     void* hip_stream) {
    const nf4gemm::MoeCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(experts), y, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex->single ? launch_moe<kScaleBnbSingle>(a, c, st) : launch_moe<kScaleBnb>(a, c, st);
}

}  // extern "C"
