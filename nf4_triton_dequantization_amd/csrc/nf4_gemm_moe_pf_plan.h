// nf4_gemm_moe_pf_plan.h -- the host-side plan of the fused expert GEMM for prompts
// (nf4_gemm_bnb_moe_pf: 1..NF4DQ_MOE_PF_MAX_PAIRS pairs, routed on the device), plain C++17 (no
// HIP): argument validation with the status codes, cfg validity, the library's choice from (P,
// experts, N, K, CU count), the launch geometry, the LDS bytes and the workspace layout.  Pure
// arithmetic, shared by the launcher (nf4_gemm_moe_pf.hip) and anything that asks the plan on a CPU.
//
// The decomposition.  A routing kernel (one workgroup) groups the P pair indices by expert into
// `perm` -- ascending within an expert, ids outside 0..E-1 in one extra bucket E -- and cuts every
// bucket into SLOTS of at most BM = 32 * waves consecutive entries of perm.  The GEMM's grid is
// slots x column tiles x K slices; a workgroup is the prefill GEMM's (nf4_gemm_pf_plan.h: BM rows,
// 128 columns, one K slice, weights decoded once per 64-deep step into LDS) on the slot's rows of
// ONE expert, x gathered and y scattered through the slot's list.  The host never sees the
// routing, so it launches the upper bound
//     S = ceil(P / BM) + min(E + 1, P)   >=   sum over buckets of ceil(count / BM)
// slots; the ones the routing does not use have no live row and return before any load.
//
// The workspace: [header kHeaderBytes, the tickets in it][ksplit slabs of P * N floats, indexed by
// POSITION IN perm; nothing for one slice][routing tables], so
//     need = kHeaderBytes + (ksplit > 1 ? ksplit * P * N * 4 : 0) + tables,
//     tables = round16(16 * S + 4 * P + 4 * (E + 1)):
// S slot entries {bucket, first position in perm, live rows, 0}, perm[P], count[E + 1].  All of it
// reads 0 between calls: the reducer clears the slabs behind its sums, the last ticket of a tile
// resets itself, and a clear kernel behind the GEMM zeroes the tables.  Unlike the other fused
// entries the need is never 0 for P >= 1.
#pragma once

#include "nf4_gemm_moe_plan.h"
#include "nf4_gemm_pf_plan.h"

namespace nf4gemm {

constexpr uint32_t kMoePfRouteThreads = 1024;  // the routing kernel's one workgroup: 16 waves
constexpr uint32_t kMoePfSlotBytes = 16;       // {bucket, first, live, 0}

// Dynamic LDS: the prefill kernel's, and the slot's list of BM pairs behind it.
inline uint32_t moe_pf_lds_bytes(const nf4_gemm_cfg& c) { return pf_lds_bytes(c) + 4u * pf_block_rows(c); }

inline bool moe_pf_shape(int64_t P, int64_t N, int64_t K) {
    return P >= 1 && P <= NF4DQ_MOE_PF_MAX_PAIRS && N >= (int64_t)kPfCols && N % kPfCols == 0 && K >= (int64_t)kChunkK &&
           K % kChunkK == 0;
}

// cfg fields: kernel = NF4DQ_GEMM_MOE_PF; waves 4 / 8 = slots of 128 / 256 rows; depth 1; ksplit =
// K slices, 1 .. min(K / 64, 16); strips 0.
inline bool valid_moe_pf_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t N, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_MOE_PF || !moe_pf_shape(P, N, K)) return false;
    if (c.waves != 4 && c.waves != 8) return false;
    if (c.depth != 1 || c.strips != 0) return false;
    if (c.ksplit < 1 || c.ksplit > kPfKsplitMax || c.ksplit > K / kPfStepK) return false;
    return moe_pf_lds_bytes(c) <= kLdsPerCu;
}

// The slots the host launches (the header comment's bound).
inline int64_t moe_pf_slots(int64_t P, int64_t experts, const nf4_gemm_cfg& c) {
    const int64_t bm = pf_block_rows(c);
    return (P + bm - 1) / bm + (experts + 1 < P ? experts + 1 : P);
}

// Where the parts of the workspace are, in bytes from its start.
struct MoePfLayout {
    size_t slab, slots, perm, count, need;
};
inline MoePfLayout moe_pf_layout(int64_t P, int64_t experts, int64_t N, const nf4_gemm_cfg& c) {
    MoePfLayout l{};
    l.slab = kHeaderBytes;
    l.slots = l.slab + (c.ksplit > 1 ? (size_t)c.ksplit * (size_t)P * (size_t)N * 4u : 0u);
    l.perm = l.slots + kMoePfSlotBytes * (size_t)moe_pf_slots(P, experts, c);
    l.count = l.perm + 4u * (size_t)P;
    l.need = (l.count + 4u * (size_t)(experts + 1) + 15u) & ~(size_t)15u;
    return l;
}
inline size_t moe_pf_workspace_need(int64_t P, int64_t experts, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (!moe_pf_shape(P, N, K) || experts < 1 || experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return moe_pf_layout(P, experts, N, c).need;
}
inline size_t moe_pf_tickets(int64_t P, int64_t experts, int64_t N, const nf4_gemm_cfg& c) {
    return (size_t)moe_pf_slots(P, experts, c) * (size_t)(N / kPfCols);
}

// The library's choice: pf_default_cfg's rule on the rows an active expert is expected to hold
// under the spread moe_rb_default_cfg assumes -- min(P, experts) experts active, each with its
// share of the pairs: 256-row slots once that share exceeds 128 rows, and as many K slices as keep
// active x slots per expert x column tiles x slices within the CUs while a slice keeps at least
// kPfSliceSteps steps.  One slice where the tickets would not fit the header, and fewer slices
// until the workspace need stays below 2^32, so the choice is valid for every shape the rules
// accept.  NOT SWEPT: the rule is carried over from the prefill GEMM's sweep
// (profiles/gemm_pf/sweep.jsonl), which has no routing; no cfg sweep of this entry has been run.
inline nf4_gemm_cfg moe_pf_default_cfg(int64_t P, int64_t experts, int64_t N, int64_t K, int cus) {
    const int64_t active = P < experts ? (P < 1 ? 1 : P) : (experts < 1 ? 1 : experts);
    const int64_t share = (P + active - 1) / active;
    nf4_gemm_cfg c{NF4DQ_GEMM_MOE_PF, share > 128 ? 8 : 4, 1, 1, 0};
    const int64_t bm = pf_block_rows(c), steps = K / kPfStepK;
    const int64_t wgs = active * ((share + bm - 1) / bm) * (N / kPfCols);
    int64_t ks = wgs > 0 ? cus / wgs : 1;
    if (ks > kPfKsplitMax) ks = kPfKsplitMax;
    if (ks > steps / kPfSliceSteps) ks = steps / kPfSliceSteps;
    if (ks < 1 || moe_pf_tickets(P, experts, N, c) * 4u > kCounterBytes) ks = 1;
    for (c.ksplit = (int)ks; c.ksplit > 1 && moe_pf_layout(P, experts, N, c).need >= (size_t(1) << 32);) --c.ksplit;
    return c;
}

// Launch geometry: grid = slots x column tiles x K slices (slice = block % ksplit, tile = block /
// ksplit % tiles, slot = block / (ksplit * tiles)), sps steps per slice (the last slices may be
// short or empty: they hand in zeros).
struct MoePfPlan {
    uint32_t grid, block, dyn, tiles, slots, steps, sps, bm;
};
inline MoePfPlan moe_pf_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    MoePfPlan p{};
    p.bm = pf_block_rows(c);
    p.tiles = (uint32_t)(N / kPfCols);
    p.slots = (uint32_t)moe_pf_slots(P, experts, c);
    p.steps = (uint32_t)(K / kPfStepK);
    p.sps = (p.steps + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.grid = p.slots * p.tiles * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = moe_pf_lds_bytes(c);
    return p;
}

// The stack's shape rules with this entry's pair bound and the prefill entry's N: moe_rb_check's
// codes in its order.
inline int moe_pf_stack_shape(const nf4_moe_experts& e, int64_t P, int64_t x_div) {
    if (P > NF4DQ_MOE_PF_MAX_PAIRS) return NF4DQ_ERR_SHAPE;
    if (e.blocksize != 64) return NF4DQ_ERR_SHAPE;  // larger statistics blocks: the per-expert loop
    if (!moe_pf_shape(P, e.N, e.K)) return NF4DQ_ERR_SHAPE;
    if (e.N > (int64_t(1) << 18) || e.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    const int64_t xrows = (P + x_div - 1) / x_div;
    if (e.N * (e.K / 2) >= (int64_t(1) << 31) || xrows * e.K * 2 >= (int64_t(1) << 31) || P * e.N * 2 >= (int64_t(1) << 31))
        return NF4DQ_ERR_TOO_LARGE;
    return NF4DQ_OK;
}

// Validates a call (nf4_gemm_bnb_moe's MoeCall) and answers what runs, as moe_rb_check does: the
// same rules in the same order.  A cfg the caller names never falls back: invalid,
// NF4DQ_GEMM_MOE_RB and NF4DQ_GEMM_PF included, is NF4DQ_ERR_ARG.
inline int moe_pf_check(const MoeCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (!a.ex) return NF4DQ_ERR_ARG;
    const nf4_moe_experts& e = *a.ex;
    if (a.P < 0 || a.x_div < 1 || !moe_stack_fields_ok(e)) return NF4DQ_ERR_ARG;
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !a.y || !moe_stack_pointers_ok(e)) return NF4DQ_ERR_ARG;
    // 16-byte loads of x, 8-byte stores of y, 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.ids, 4)) return NF4DQ_ERR_ARG;
    if (const int rc = moe_pf_stack_shape(e, a.P, a.x_div)) return rc;
    if (!moe_stack_strides_ok(e)) return NF4DQ_ERR_SHAPE;
    nf4_gemm_cfg c = a.cfg ? *a.cfg : moe_pf_default_cfg(a.P, e.experts, e.N, e.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MOE_PF;
    if (!valid_moe_pf_cfg(c, a.P, e.N, e.K)) return NF4DQ_ERR_ARG;
    if (c.ksplit > 1 && moe_pf_tickets(a.P, e.experts, e.N, c) * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = moe_pf_workspace_need(a.P, e.experts, e.N, e.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16)) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
