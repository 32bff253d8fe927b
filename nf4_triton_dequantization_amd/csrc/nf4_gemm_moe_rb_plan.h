// nf4_gemm_moe_rb_plan.h -- the host-side plan of the fused expert GEMM in row blocks
// (nf4_gemm_bnb_moe_rb: up to NF4DQ_MOE_RB_MAX_PAIRS pairs), plain C++17 (no HIP): argument
// validation with the status codes, cfg validity, the library's choice from (P, experts, N, K, CU
// count), the launch geometry, the LDS bytes and the workspace need.  Pure arithmetic, shared by
// the launcher (nf4_gemm_moe_rb.hip) and a CPU check (tests/plan/gemm_moe_rb_plan_check.cpp).
//
// The decomposition is nf4_gemm_bnb_moe's (nf4_gemm_moe_plan.h) with one more grid dimension:
// a workgroup owns ONE expert, 32 * waves of its columns, one K slice and one ROW BLOCK, the
// entries [128 rb, 128 rb + 128) of the expert's ascending pair list.  The grid is experts x
// column tiles x K slices x ceil(P / 128) row blocks whatever the routing; a workgroup whose
// expert has no more than 128 rb pairs returns at once.  What one workgroup stages -- at most 128
// rows, the LDS list of 128 entries, the row tiles -- is nf4_gemm_bnb_moe's at min(P, 128) pairs,
// so the stack rules, the cfg fields and the LDS bytes are that plan's.  K slices meet in an fp32
// slab indexed by pair (P * N floats a slice), with one ticket per (expert, column tile, row
// block).
#pragma once

#include "nf4_gemm_moe_plan.h"

namespace nf4gemm {

constexpr int64_t kMoeRbRows = NF4DQ_MOE_MAX_PAIRS;  // listed rows of one row block
static_assert(NF4DQ_MOE_RB_MAX_PAIRS % NF4DQ_MOE_MAX_PAIRS == 0, "whole row blocks");

inline int64_t moe_rb_blocks(int64_t P) { return (P + kMoeRbRows - 1) / kMoeRbRows; }
// The rows one workgroup may stage: all P up to a row block, a row block beyond.
inline int64_t moe_rb_rows(int64_t P) { return P < kMoeRbRows ? P : kMoeRbRows; }

// nf4_gemm_bnb_moe's rules per workgroup under this entry's cfg.kernel.
constexpr MtEntry kMoeRbEntry{NF4DQ_GEMM_MOE_RB, NF4DQ_MOE_MAX_PAIRS, 16u * kMtStrips, 1, kMoeTableBytes};
// Row tiles the kernel is instantiated for: 8 beyond one row block (the run-time guards skip what
// a block does not fill), the expert GEMM's own up to it.
inline int moe_rb_row_tiles(int64_t P) { return moe_row_tiles(moe_rb_rows(P)); }
inline uint32_t moe_rb_lds_bytes(int64_t P) { return moe_lds_bytes(moe_rb_rows(P)); }
inline bool valid_moe_rb_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t N, int64_t K) {
    return P >= 1 && P <= NF4DQ_MOE_RB_MAX_PAIRS && mt_entry_valid(kMoeRbEntry, c, moe_rb_rows(P), N, K);
}

// The library's choice.  The K slices assume the spread moe_entry_ksplit assumes: min(P, experts)
// experts active, each with its share of the pairs, ceil(share / 128) live row blocks each.
// The working grid under it is active x live row blocks x column tiles x K slices, and the K
// slices are the row-tiled family's rule on that grid against one resident workgroup a CU
// beyond 128 pairs (8 row tiles), nf4_gemm_bnb_moe's own count up to 128 (so that the two
// entries choose alike where both run).
// NOT MEASURED beyond 128 pairs: the rule is carried over from nf4_gemm_bnb_moe, whose sweep
// (profiles/gemm_moe/sweep_slices.jsonl) ends at 128 pairs; no sweep of this entry has been run.
// With many rows per expert a slab of P * N floats per slice is written, read and cleared, so a
// slice costs more here than there; the rule answers 1 wherever the assumed grid alone fills the
// CUs, which it does at Mixtral's shapes from 256 pairs on (pinned in the plan check).
inline nf4_gemm_cfg moe_rb_default_cfg(int64_t P, int64_t experts, int64_t N, int64_t K, int cus) {
    nf4_gemm_cfg c{NF4DQ_GEMM_MOE_RB, N % 128 == 0 ? 4 : 2, 1, 1, kMtStrips};
    const int64_t active = P < experts ? (P < 1 ? 1 : P) : (experts < 1 ? 1 : experts);
    const int64_t live = moe_rb_blocks((P + active - 1) / active);
    const int resident = P > kMoeRbRows ? 1 : moe_resident(P);
    c.ksplit = mt_entry_ksplit((int64_t)cus * resident, N / mt_entry_cols(kMoeRbEntry, c) * active * (live < 1 ? 1 : live), K);
    return c;
}

// Launch geometry: nf4_gemm_bnb_moe's at the rows of one workgroup, once per row block (block =
// ((rb * experts + expert) * tiles + tile) * ksplit + slice); tickets = experts x column tiles x
// row blocks.
struct MoeRbPlan {
    uint32_t grid, block, dyn, tiles, chunks, cps, row_tiles, tickets, row_blocks;
};
inline MoeRbPlan moe_rb_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    const MoePlan g = moe_entry_plan(kMoeRbEntry, c, moe_rb_rows(P), experts, N, K);
    const uint32_t rbs = (uint32_t)moe_rb_blocks(P);
    return MoeRbPlan{g.grid * rbs, g.block, g.dyn, g.tiles, g.chunks, g.cps, g.row_tiles, g.tickets * rbs, rbs};
}
// (ksplit slabs of P * N floats indexed by pair; nothing for one slice or a shape the entry rejects)
inline size_t moe_rb_workspace_need(int64_t P, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (P < 1 || P > NF4DQ_MOE_RB_MAX_PAIRS || !mt_entry_shape(kMoeRbEntry, moe_rb_rows(P), N, K)) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * (size_t)P * (size_t)N * 4u : 0;
}

// moe_stack_shape with this entry's pair bound: the codes in the same order.
inline int moe_rb_stack_shape(const nf4_moe_experts& e, int64_t P) {
    if (P > NF4DQ_MOE_RB_MAX_PAIRS) return NF4DQ_ERR_SHAPE;
    if (const int rc = moe_stack_shape(e, moe_rb_rows(P))) return rc;
    return P * e.K * 2 >= (int64_t(1) << 31) ? NF4DQ_ERR_TOO_LARGE : NF4DQ_OK;
}

// Validates a call (nf4_gemm_bnb_moe's MoeCall) and answers what runs, as moe_check does: the
// same rules in the same order, then mt_entry_resolve's tail with the tickets and the slab of
// all the row blocks.  A cfg the caller names never falls back: invalid, NF4DQ_GEMM_MOE
// included, is NF4DQ_ERR_ARG.
inline int moe_rb_check(const MoeCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (!a.ex) return NF4DQ_ERR_ARG;
    const nf4_moe_experts& e = *a.ex;
    if (a.P < 0 || a.x_div < 1 || !moe_stack_fields_ok(e)) return NF4DQ_ERR_ARG;
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !a.y || !moe_stack_pointers_ok(e)) return NF4DQ_ERR_ARG;
    // 16-byte loads of x, 8-byte stores of y, 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.ids, 4)) return NF4DQ_ERR_ARG;
    if (const int rc = moe_rb_stack_shape(e, a.P)) return rc;
    if (!moe_stack_strides_ok(e)) return NF4DQ_ERR_SHAPE;
    nf4_gemm_cfg c = a.cfg ? *a.cfg : moe_rb_default_cfg(a.P, e.experts, e.N, e.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MOE_RB;
    if (c.strips == 0) c.strips = kMtStrips;
    if (!valid_moe_rb_cfg(c, a.P, e.N, e.K)) return NF4DQ_ERR_ARG;
    const size_t tickets = (size_t)(e.N / mt_entry_cols(kMoeRbEntry, c)) * (size_t)e.experts * (size_t)moe_rb_blocks(a.P);
    if (c.ksplit > 1 && tickets * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = moe_rb_workspace_need(a.P, e.N, e.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
