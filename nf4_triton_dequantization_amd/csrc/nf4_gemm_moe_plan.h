// nf4_gemm_moe_plan.h -- the host-side plan of the fused expert GEMM of a mixture-of-experts
// block (nf4_gemm_bnb_moe), plain C++17 (no HIP): argument validation with the status codes,
// cfg validity, the library's choice from (P, experts, N, K, CU count), the launch geometry,
// the LDS bytes and the workspace need.  Pure arithmetic, shared by the launcher
// (nf4_gemm_moe.hip) and a CPU check (tests/plan/gemm_moe_plan_check.cpp).
//
// The decomposition is the row-tiled family's (nf4_gemm_mt_plan.h) once per expert: a
// workgroup of `waves` waves owns ONE expert, 32 * waves of its output columns, all the
// expert's rows and one K slice.  Which rows those are is found on the device: the workgroup
// reads the P expert ids and lists its expert's pairs in ascending order.  The grid is experts
// x column tiles x K slices whatever the routing; a workgroup whose expert has no pair returns
// at once.  K slices meet in an fp32 slab of the caller's workspace, indexed by pair (a pair
// belongs to one expert, so experts never collide), with one ticket per (expert, column tile).
#pragma once

#include "nf4_gemm_mt_plan.h"

namespace nf4gemm {

// behind the x buffers: the row-tiled kernel's tables, then the expert's pair list twice (the
// x row and the y row of every staged row)
constexpr uint32_t kMoeListBytes = 2u * 4u * NF4DQ_MOE_MAX_PAIRS;
constexpr uint32_t kMoeTableBytes = kMtTableBytes + kMoeListBytes;
static_assert(NF4DQ_MOE_MAX_PAIRS == NF4DQ_GEMM_MT_MAX_M, "the row tiles are the row-tiled family's");

// Row tiles the kernel is instantiated for: one expert may get all P pairs.
inline int moe_row_tiles(int64_t P) { return mt_row_tiles(P); }

// The row-tiled family's rules (nf4_gemm_mt_plan.h) once per expert: its cfg fields and validity,
// 32 columns per wave, one plane per slice indexed by pair, one ticket per (expert, column tile).
constexpr MtEntry kMoeEntry{NF4DQ_GEMM_MOE, NF4DQ_MOE_MAX_PAIRS, 16u * kMtStrips, 1, kMoeTableBytes};
inline uint32_t moe_lds_bytes(int64_t P) { return mt_entry_lds(kMoeEntry, P); }
inline bool valid_moe_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t N, int64_t K) { return mt_entry_valid(kMoeEntry, c, P, N, K); }

// Workgroups of 4 waves a CU holds at once, by row tiles: two with two row tiles (at most 256
// registers a lane, the kernel's launch bound), one beyond.
inline int moe_resident(int64_t P) { return moe_row_tiles(P) <= 2 ? 2 : 1; }

// The K slices of an expert entry.  The host never sees the routing, so the plan ASSUMES the
// spread a router aims at: min(P, experts) experts active, each with its share of the pairs.
// Under it the working grid is active x column tiles x K slices, and the K slices are the
// row-tiled family's rule on that grid against `resident` workgroups a CU.
inline int moe_entry_ksplit(const MtEntry& e, const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K,
                            int cus, int resident) {
    const int64_t active = P < experts ? (P < 1 ? 1 : P) : (experts < 1 ? 1 : experts);
    return mt_entry_ksplit((int64_t)cus * resident, N / mt_entry_cols(e, c) * active, K);
}

// The library's choice: moe_entry_ksplit with moe_resident() workgroups a CU.  Measured
// on MI355X at Mixtral's shapes with 8 experts (profiles/gemm_moe/sweep_slices.jsonl, 1..16
// slices): the rule's count is the fastest at 7 of the 8 (shape, T) cells and within 9 % at the
// eighth (4096 x 14336 at 4 tokens: 2 slices 102 us, 3 slices 94 us); a grid beyond what the CUs
// hold costs up to 3 x.  The kernel decodes every weight on the VALU with one or two waves per
// SIMD, so with few rows it is bound by that decode, not by HBM: more resident workgroups are
// what the slices buy.  Fewer active experts than assumed (pairs piling onto
// one expert) leave CUs idle, never oversubscribed; the result is right for every routing, only
// the speed depends on it.
inline nf4_gemm_cfg moe_default_cfg(int64_t P, int64_t experts, int64_t N, int64_t K, int cus) {
    nf4_gemm_cfg c{NF4DQ_GEMM_MOE, N % 128 == 0 ? 4 : 2, 1, 1, kMtStrips};
    c.ksplit = moe_entry_ksplit(kMoeEntry, c, P, experts, N, K, cus, moe_resident(P));
    return c;
}

// Launch geometry: the family's with the experts as groups; tickets = experts x column tiles.
struct MoePlan {
    uint32_t grid, block, dyn, tiles, chunks, cps, row_tiles, tickets;
};
inline MoePlan moe_entry_plan(const MtEntry& e, const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    const MtPlan g = mt_entry_plan(e, c, P, N, K, experts);
    return MoePlan{g.grid, g.block, g.dyn, g.tiles, g.chunks, g.cps, g.row_tiles, g.tiles * (uint32_t)experts};
}
inline MoePlan moe_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    return moe_entry_plan(kMoeEntry, c, P, experts, N, K);
}
// (ksplit slabs of P * N floats indexed by pair)
inline size_t moe_workspace_need(int64_t P, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    return mt_entry_workspace(kMoeEntry, P, N, K, c);
}

// The rules of ONE stack of experts, for moe_check and msg_check.  Each returns one status code,
// and the checks call them in the order the codes are pinned in: fields (ARG), P == 0, pointers
// (ARG), shape (SHAPE, then TOO_LARGE), strides (SHAPE).
inline bool moe_stack_fields_ok(const nf4_moe_experts& e) {
    if (e.N < 0 || e.K < 0 || e.packed_stride < 0 || e.nb_stride < 0 || e.n2_stride < 0 || e.code2_stride < 0) return false;
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return false;
    if (e.blocksize < 64 || e.blocksize > 4096 || (e.blocksize & (e.blocksize - 1))) return false;
    return e.single || (e.blocksize2 >= 4 && !(e.blocksize2 & (e.blocksize2 - 1)));
}
// (16-byte loads of the packed weight, every expert's: the stride keeps the alignment)
inline bool moe_stack_pointers_ok(const nf4_moe_experts& e) {
    if (!e.packed || !e.absmax2 || (!e.single && (!e.absmax_q || !e.code2))) return false;
    return mt_aligned(e.packed, 16) && e.packed_stride % 16 == 0 && mt_aligned(e.absmax2, 4) && mt_aligned(e.code2, 4) &&
           mt_aligned(e.offset, 4);
}
inline int moe_stack_shape(const nf4_moe_experts& e, int64_t P) {
    if (e.blocksize != 64) return NF4DQ_ERR_SHAPE;  // larger statistics blocks: the per-expert loop
    if (P > NF4DQ_MOE_MAX_PAIRS || e.N < 64 || e.N % 64 || e.K < (int64_t)kChunkK || e.K % kChunkK) return NF4DQ_ERR_SHAPE;
    if (e.N > (int64_t(1) << 18) || e.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    if (e.N * (e.K / 2) >= (int64_t(1) << 31) || P * e.K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    return NF4DQ_OK;
}
inline bool moe_stack_strides_ok(const nf4_moe_experts& e) {
    const int64_t plen = e.N * (e.K / 2), nblk = e.N * e.K / 64;
    if (e.packed_stride < plen) return false;
    if (e.single ? e.n2_stride < nblk : (e.nb_stride < nblk || e.n2_stride < (nblk + e.blocksize2 - 1) / e.blocksize2)) return false;
    return e.single || e.code2_stride == 0 || e.code2_stride >= 256;
}

// One call of nf4_gemm_bnb_moe.
struct MoeCall {
    const void* x;
    const void* ids;
    int64_t P;
    int32_t x_div;
    const nf4_moe_experts* ex;
    void* y;
    int32_t dtype;
    void* workspace;
    size_t workspace_bytes;
    const nf4_gemm_cfg* cfg;
};

// Validates a call and answers what runs: NF4DQ_OK and *out (*launch false: P == 0, nothing to
// do), or the status code.  A cfg the caller names never falls back: invalid is NF4DQ_ERR_ARG.
inline int moe_check(const MoeCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (!a.ex) return NF4DQ_ERR_ARG;
    const nf4_moe_experts& e = *a.ex;
    if (a.P < 0 || a.x_div < 1 || !moe_stack_fields_ok(e)) return NF4DQ_ERR_ARG;
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !a.y || !moe_stack_pointers_ok(e)) return NF4DQ_ERR_ARG;
    // 16-byte loads of x, 8-byte stores of y, 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.ids, 4)) return NF4DQ_ERR_ARG;
    if (const int rc = moe_stack_shape(e, a.P)) return rc;
    if (!moe_stack_strides_ok(e)) return NF4DQ_ERR_SHAPE;
    const int rc = mt_entry_resolve(kMoeEntry, a.cfg, moe_default_cfg(a.P, e.experts, e.N, e.K, cus), a.P, e.N, e.K, e.experts,
                                    a.workspace, a.workspace_bytes, out);
    *launch = rc == NF4DQ_OK;
    return rc;
}

}  // namespace nf4gemm
