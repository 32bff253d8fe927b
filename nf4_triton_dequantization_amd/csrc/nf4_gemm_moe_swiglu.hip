// nf4_gemm_moe_swiglu.hip -- the fused expert SwiGLU launch of a mixture-of-experts block in
// bitsandbytes semantics (nf4_gemm_bnb_moe_swiglu): launcher and C entries.  The kernel is
// nf4_gemm_moe_dev.h's template with W = 2 (the gate and the up stack, the SwiGLU chain behind
// their sums); the plan -- validation, cfg, geometry, LDS, workspace -- is
// nf4_gemm_moe_swiglu_plan.h.
#include "nf4_gemm_moe_dev.h"
#include "nf4_gemm_moe_swiglu_plan.h"

namespace {

template <int SM>
int launch_msg(const nf4gemm::MsgCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& g = a.ex[0];
    const MoePlan p = msg_plan(cfg, a.P, g.experts, g.N, g.K);
    const MoeArgsT<2> A = moe_fill<2>(a, a.h, p, cfg);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_moe_kernel<DT, MT, SM, WV, false, 2>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_swiglu_workspace_bytes(int64_t P, const void* gate_up, const nf4_gemm_cfg* cfg) {
    if (!gate_up) return 0;
    const nf4_moe_experts& g = *reinterpret_cast<const nf4_moe_experts*>(gate_up);
    if (g.experts < 1 || g.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return msg_workspace_need(P, g.N, g.K, cfg ? *cfg : msg_default_cfg(P, g.experts, g.N, g.K, device_cus()));
}

int nf4_gemm_bnb_moe_swiglu(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* gate_up,
                            int32_t act, void* h, int32_t out_dtype, void* workspace, size_t workspace_bytes,
                            const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MsgCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(gate_up), act, h, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = msg_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex[0].single ? launch_msg<kScaleBnbSingle>(a, c, st) : launch_msg<kScaleBnb>(a, c, st);
}

}  // extern "C"
