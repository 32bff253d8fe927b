// nf4_gemm_moe_swiglu_plan.h -- the host-side plan of the fused expert SwiGLU launch of a
// mixture-of-experts block (nf4_gemm_bnb_moe_swiglu: h[p] = silu(x . Wg_e^T) * (x . Wu_e^T) with
// e = expert_ids[p]), plain C++17 (no HIP): argument validation with the status codes, cfg
// validity, the library's choice from (P, experts, I, K, CU count), the launch geometry, the LDS
// bytes and the workspace need.  Pure arithmetic, shared by the launcher
// (nf4_gemm_moe_swiglu.hip) and a CPU check (tests/plan/gemm_moe_swiglu_plan_check.cpp).
//
// The decomposition is the expert GEMM's (nf4_gemm_moe_plan.h) with the SwiGLU launch's strips
// (nf4_gemm_mt_swiglu_plan.h): a workgroup of `waves` waves owns ONE expert, 16 * waves columns
// of h, all the expert's rows and one K slice; a wave owns 16 columns -- strip 0 is rows
// col .. col + 15 of the expert's gate weight, strip 1 the same rows of its up weight, each with
// its own statistics, code2 table, offset and blocksize2.  The grid is experts x column tiles x
// K slices whatever the routing.  K slices meet in two fp32 planes per slice,
// [ksplit][2][P][I], indexed by pair, with one ticket per (expert, column tile).
#pragma once

#include "nf4_gemm_moe_plan.h"
#include "nf4_gemm_mt_swiglu_plan.h"

namespace nf4gemm {

// behind the x buffers: the SwiGLU launch's tables (two code2 tables, the codes, the flag), then
// the expert's pair list twice
constexpr uint32_t kMsgTableBytes = kSgTableBytes + kMoeListBytes;

// The expert GEMM's rules over 16 columns of h per wave (32 / 64 a workgroup) and two planes per
// slice, the gate plane and the up plane of P * I floats indexed by pair.
constexpr MtEntry kMsgEntry{NF4DQ_GEMM_MOE_SWIGLU, NF4DQ_MOE_MAX_PAIRS, 16u, 2, kMsgTableBytes};
inline uint32_t msg_cols(const nf4_gemm_cfg& c) { return mt_entry_cols(kMsgEntry, c); }
inline uint32_t msg_lds_bytes(int64_t P) { return mt_entry_lds(kMsgEntry, P); }
inline bool valid_msg_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t I, int64_t K) { return mt_entry_valid(kMsgEntry, c, P, I, K); }

// Workgroups of 4 waves a CU holds at once, by row tiles: the kernel's launch bound.  With two row
// tiles the two-table kernel and its expf epilogue stay within 256 registers without a spill
// (DESIGN section 4b), so two are resident as in the expert GEMM; one beyond.
inline int msg_resident(int64_t P) { return moe_row_tiles(P) <= 2 ? 2 : 1; }

// The library's choice: moe_default_cfg's rule over this launch's column tiles -- four waves (64
// columns of h, 128 weight rows: I % 64 == 0 always allows them), min(P, experts) experts assumed
// active, and as many K slices as keep active x tiles x slices within what the CUs hold at once
// (msg_resident() workgroups each) while a slice keeps at least kMtSliceChunks chunks.  A slice
// costs two planes of the expert's rows written, read and cleared.  Measured on MI355X over
// waves 2 / 4 x 1..16 slices at Mixtral's w1 / w3 (14336 x 4096, 8 experts, top-2) for 2 / 8 / 32 /
// 128 pairs (profiles/gemm_moe_swiglu/sweep_slices.jsonl): the rule's choice there -- four waves,
// ONE slice, 224 column tiles per expert -- is the fastest of the 32 cfgs in every cell (60 / 148 /
// 201 / 357 us; two slices 85 / 222 / 315 / 494, sixteen 4x - 8x; two waves with one slice tie at
// 8 and 32 pairs and lose 8 - 13 % at 2 and 128), so the rule stands as moe_default_cfg's.  What
// it rests on beyond that shape is the expert GEMM's sweep (nf4_gemm_moe_plan.h): slices buy
// resident workgroups where the column tiles do not fill the CUs, and a grid beyond what the CUs
// hold costs more than it buys.  Shapes with few column tiles and a long K were not swept here.
inline nf4_gemm_cfg msg_default_cfg(int64_t P, int64_t experts, int64_t I, int64_t K, int cus) {
    nf4_gemm_cfg c{NF4DQ_GEMM_MOE_SWIGLU, 4, 1, 1, kMtStrips};
    c.ksplit = moe_entry_ksplit(kMsgEntry, c, P, experts, I, K, cus, msg_resident(P));
    return c;
}
inline MoePlan msg_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t I, int64_t K) {
    return moe_entry_plan(kMsgEntry, c, P, experts, I, K);
}
inline size_t msg_workspace_need(int64_t P, int64_t I, int64_t K, const nf4_gemm_cfg& c) {
    return mt_entry_workspace(kMsgEntry, P, I, K, c);
}

// One call of nf4_gemm_bnb_moe_swiglu: ex[0] is the gate stack, ex[1] the up stack.
struct MsgCall {
    const void* x;
    const void* ids;
    int64_t P;
    int32_t x_div;
    const nf4_moe_experts* ex;
    int32_t act;
    void* h;
    int32_t dtype;
    void* workspace;
    size_t workspace_bytes;
    const nf4_gemm_cfg* cfg;
};

// Validates a call and answers what runs: NF4DQ_OK and *out (*launch false: P == 0, nothing to
// do), or the status code -- moe_check's rules and order, applied to each stack.  A cfg the
// caller names never falls back: invalid is NF4DQ_ERR_ARG.
inline int msg_check(const MsgCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (a.act != NF4DQ_ACT_SILU) return NF4DQ_ERR_ARG;
    if (!a.ex) return NF4DQ_ERR_ARG;
    const nf4_moe_experts& g = a.ex[0];
    const nf4_moe_experts& u = a.ex[1];
    if (a.P < 0 || a.x_div < 1 || !moe_stack_fields_ok(g) || !moe_stack_fields_ok(u)) return NF4DQ_ERR_ARG;
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !a.h || !moe_stack_pointers_ok(g) || !moe_stack_pointers_ok(u)) return NF4DQ_ERR_ARG;
    // 16-byte loads of x, 8-byte stores of h, 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.h, 8) || !mt_aligned(a.ids, 4)) return NF4DQ_ERR_ARG;
    if (g.N != u.N || g.K != u.K || g.experts != u.experts || (g.single != 0) != (u.single != 0)) return NF4DQ_ERR_SHAPE;
    if (u.blocksize != 64) return NF4DQ_ERR_SHAPE;  // (the gate's: moe_stack_shape; N and K are the gate's by now)
    if (const int rc = moe_stack_shape(g, a.P)) return rc;
    if (!moe_stack_strides_ok(g) || !moe_stack_strides_ok(u)) return NF4DQ_ERR_SHAPE;
    const int rc = mt_entry_resolve(kMsgEntry, a.cfg, msg_default_cfg(a.P, g.experts, g.N, g.K, cus), a.P, g.N, g.K, g.experts,
                                    a.workspace, a.workspace_bytes, out);
    *launch = rc == NF4DQ_OK;
    return rc;
}

}  // namespace nf4gemm
