// nf4_gemm_moe_down_plan.h -- the host-side plan of the fused down projection of a
// mixture-of-experts block with the routed weighted sum (nf4_gemm_bnb_moe_down:
// y[t] = sum_j rw[t k + j] * (x[t k + j] . W_e^T), e = expert_ids[t k + j]), plain C++17 (no HIP):
// argument validation with the status codes, cfg validity, the library's choice, the launch
// geometry, the LDS bytes and the workspace need.  Pure arithmetic, shared by the launcher
// (nf4_gemm_moe_down.hip) and a CPU check (tests/plan/gemm_moe_down_plan_check.cpp).
//
// The GEMM is the expert GEMM's (nf4_gemm_moe_plan.h): the same grid, cfg fields, default rule,
// LDS and slabs, so for one (waves, ksplit) the per-pair products are bit for bit what
// nf4_gemm_bnb_moe stores.  They go as 16-bit values to a scratch [P][N] of the workspace, and a
// second ticket per COLUMN TILE counts one arrival per expert; the last arrival combines the tile.
// The counters of the header are therefore the experts x tiles tickets of the K slices followed
// by the tiles tickets of the combine, and the workspace is never empty.
#pragma once

#include "nf4_gemm_moe_plan.h"

namespace nf4gemm {

inline uint32_t down_lds_bytes(int64_t P) { return moe_lds_bytes(P); }

// cfg fields: kernel = NF4DQ_GEMM_MOE_DOWN; the rest as the expert GEMM's.
inline nf4_gemm_cfg down_as_moe(nf4_gemm_cfg c) {
    c.kernel = c.kernel == NF4DQ_GEMM_MOE_DOWN ? NF4DQ_GEMM_MOE : -1;
    return c;
}
inline bool valid_down_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t N, int64_t K) {
    return valid_moe_cfg(down_as_moe(c), P, N, K);
}

// The library's choice: moe_default_cfg's, field for field, under this entry's kernel id.
inline nf4_gemm_cfg down_default_cfg(int64_t P, int64_t experts, int64_t N, int64_t K, int cus) {
    nf4_gemm_cfg c = moe_default_cfg(P, experts, N, K, cus);
    c.kernel = NF4DQ_GEMM_MOE_DOWN;
    return c;
}

// Launch geometry: the expert GEMM's.  Counters: p.tickets (expert, column tile) tickets, then
// p.tiles tile tickets.
inline MoePlan down_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    return moe_plan(down_as_moe(c), P, experts, N, K);
}
inline size_t down_counters(const MoePlan& p) { return (size_t)p.tickets + p.tiles; }

// Workspace: the header (tickets, 0 between calls), ksplit slabs of P * N floats when ksplit > 1
// (0 between calls), then the 16-bit scratch of P * N elements (don't-care between calls: every
// element the combiner reads was written in the same call).  N % 64 == 0 keeps every part
// 16-byte aligned.  0 only for a shape the entry rejects.
inline size_t down_slab_bytes(int64_t P, int64_t N, const nf4_gemm_cfg& c) {
    return c.ksplit > 1 ? (size_t)c.ksplit * (size_t)P * (size_t)N * 4u : 0;
}
inline size_t down_scratch_offset(int64_t P, int64_t N, const nf4_gemm_cfg& c) { return kHeaderBytes + down_slab_bytes(P, N, c); }
inline size_t down_workspace_need(int64_t P, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (!mt_entry_shape(kMoeEntry, P, N, K)) return 0;
    return down_scratch_offset(P, N, c) + (size_t)P * (size_t)N * 2u;
}

// One call of nf4_gemm_bnb_moe_down: the expert GEMM's call (m.y is [P / topk][N]; m.workspace
// this entry's) and the combine's arguments.
struct DownCall {
    MoeCall m;
    int32_t topk;
    const void* rw;  // [P], fp32 or m.dtype
    int32_t rw_dtype;
};

// Validates a call and answers what runs: NF4DQ_OK and *out (*launch false: P == 0, nothing to
// do), or the status code.  The expert GEMM's rules with its codes in its order (moe_check over
// the same call, its workspace rule left to this one), then topk and rw, then this entry's
// tickets and workspace.  A cfg the caller names never falls back: invalid is NF4DQ_ERR_ARG.
inline int down_check(const DownCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.rw_dtype != NF4DQ_F32 && a.rw_dtype != a.m.dtype) return NF4DQ_ERR_ARG;
    MoeCall m = a.m;
    nf4_gemm_cfg named{};
    if (a.m.cfg) {
        named = *a.m.cfg;
        if (named.kernel == 0) named.kernel = NF4DQ_GEMM_MOE_DOWN;
        named = down_as_moe(named);
        m.cfg = &named;
    }
    alignas(16) static const char any_workspace[16] = {};  // never dereferenced
    m.workspace = const_cast<char*>(any_workspace);
    m.workspace_bytes = ~size_t(0);
    nf4_gemm_cfg c{};
    const int rc = moe_check(m, cus, &c, launch);
    if (rc != NF4DQ_OK || !*launch) return rc;
    *launch = false;
    const nf4_moe_experts& e = *a.m.ex;
    if (a.topk < 1 || a.topk > a.m.P || a.m.P % a.topk) return NF4DQ_ERR_ARG;
    if (!a.rw || !mt_aligned(a.rw, a.rw_dtype == NF4DQ_F32 ? 4 : 2)) return NF4DQ_ERR_ARG;
    c.kernel = NF4DQ_GEMM_MOE_DOWN;
    if (down_counters(down_plan(c, a.m.P, e.experts, e.N, e.K)) * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = down_workspace_need(a.m.P, e.N, e.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (!a.m.workspace || a.m.workspace_bytes < need || !mt_aligned(a.m.workspace, 16)) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
