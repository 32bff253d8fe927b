// nf4_gemm_moe_down.hip -- the fused down projection of a mixture-of-experts block with the
// routed weighted sum, in bitsandbytes semantics (nf4_gemm_bnb_moe_down): launcher and C entries.
// The kernel is the expert GEMM's body under its DOWN flag (nf4_gemm_moe_dev.h); the plan --
// validation, cfg, geometry, LDS, workspace layout -- is nf4_gemm_moe_down_plan.h.
#include "nf4_gemm_moe_dev.h"
#include "nf4_gemm_moe_down_plan.h"

namespace {

template <int SM>
int launch_down(const nf4gemm::DownCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4gemm::MoeCall& m = a.m;
    const nf4_moe_experts& e = *m.ex;
    const MoePlan p = down_plan(cfg, m.P, e.experts, e.N, e.K);
    char* ws = reinterpret_cast<char*>(m.workspace);
    MoeDownArgs D{};
    D.g = moe_fill<1>(m, ws + down_scratch_offset(m.P, e.N, cfg), p, cfg);  // the products go to the scratch
    const MoeArgsT<1>& A = D.g;
    D.c = MoeCombine{A.ids, a.rw, reinterpret_cast<const uint16_t*>(A.y), m.y, A.counters + p.tickets,
                     A.P, A.E, A.N, (uint32_t)a.topk, a.rw_dtype == NF4DQ_F32 ? 1u : 0u};
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(m.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_moe_kernel<DT, MT, SM, WV, true>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, D);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_down_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg) {
    if (!experts) return 0;
    const nf4_moe_experts& e = *reinterpret_cast<const nf4_moe_experts*>(experts);
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return down_workspace_need(P, e.N, e.K, cfg ? *cfg : down_default_cfg(P, e.experts, e.N, e.K, device_cus()));
}

int nf4_gemm_bnb_moe_down(const void* x, const void* expert_ids, int64_t P, int32_t x_div, int32_t topk,
                          const void* routing_weights, int32_t rw_dtype, const void* experts, void* y,
                          int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                          void* hip_stream) {
    const nf4gemm::DownCall a{{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(experts), y, out_dtype,
                               workspace, workspace_bytes, cfg},
                              topk, routing_weights, rw_dtype};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = down_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.m.ex->single ? launch_down<kScaleBnbSingle>(a, c, st) : launch_down<kScaleBnb>(a, c, st);
}

}  // extern "C"
