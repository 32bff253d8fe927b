// nf4_gemm_moe_dec_plan.h -- the host-side plan of the fused expert GEMM for decode in 16-row
// slots (nf4_gemm_bnb_moe_dec: 1..NF4DQ_MOE_MAX_PAIRS pairs, routed on the device), plain C++17
// (no HIP): argument validation with the status codes, cfg validity, the library's choice from
// (P, experts, N, K, CU count), the launch geometry, the LDS bytes and the workspace need.  Pure
// arithmetic, shared by the launcher (nf4_gemm_moe_dec.hip) and anything that asks the plan on a
// CPU.
//
// The decomposition.  A SLOT is one (expert, block of 16 consecutive entries of that expert's
// ascending pair list); slots are numbered in (expert, block) order.  The grid is slots x column
// tiles of 64 columns x K slices, fixed by the host whatever the routing: it launches
//     S = min(E, P) + (P - min(E, P)) / 16   >=   sum over experts of ceil(count / 16)
// slots (an active expert's first slot takes at least one pair, every further one follows 16 more:
// E - 1 experts with one pair each and one expert with the rest reaches it).  Every workgroup finds
// its slot's expert and its at most 16 pairs from the P ids on the device; a slot past the used
// ones returns before any weight or statistics load.  Inside a workgroup K is split over the
// WAVES: wave w of K slice ks owns the `strips` 128-deep chunks from (ks * waves + w) * strips,
// holds the slot's rows of x for them in registers as MFMA fragments for the whole launch, and
// walks the tile's four 16-column strips with a `depth`-deep register ring of 16-byte packed
// loads.  The waves' partial tiles meet in LDS and are summed in wave order; K slices meet in the
// family's fp32 slab indexed by pair, with one ticket per (slot, column tile).
//
// LDS of one workgroup: the pair table (64 KiB: 256 packed bytes x 32 copies x two fp32 codes,
// which the waves' partial tiles reuse once the strips are done), one code2 table, the experts'
// pair counts and first slots (2 x 256 words) and the slot's list: kMoeDecLdsBytes = 68688.  A CU
// (160 KiB) therefore holds TWO workgroups by LDS; the kernel is compiled for at least 4 waves
// per SIMD (at most 128 registers a lane), so a CU holds two workgroups of 8 waves or one of 16
// waves: 4 waves per SIMD either way (moe_dec_resident()).
#pragma once

#include "nf4_gemm_moe_plan.h"

namespace nf4gemm {

constexpr int64_t kMoeDecRows = 16;      // pairs of one slot: one MFMA M-tile
constexpr uint32_t kMoeDecCols = 64;     // columns of one workgroup: four 16-column strips
constexpr int kMoeDecTileStrips = 4;
constexpr int kMoeDecKsplitMax = 16;
constexpr uint32_t kMoeDecPairTableBytes = 256u * 32u * 8u;
// [pair table | partial tiles][code2][pair counts][first slots][flag, expert, rows, pad][the slot's 16 pairs]
constexpr uint32_t kMoeDecLdsBytes = kMoeDecPairTableBytes + 1024u + 1024u + 1024u + 16u + 64u;
static_assert(kMoeDecLdsBytes == 68688 && 2u * kMoeDecLdsBytes <= kLdsPerCu, "two workgroups a CU by LDS");
static_assert(16u * kMoeDecTileStrips * 64u * 16u <= kMoeDecPairTableBytes, "16 waves' partial tiles fit the pair table");

// Workgroups a CU holds at once: 4 waves per SIMD.
inline int moe_dec_resident(const nf4_gemm_cfg& c) { return c.waves == 8 ? 2 : 1; }

// The slots the host launches (the header comment's bound).
inline int64_t moe_dec_slots(int64_t P, int64_t experts) {
    const int64_t first = experts < P ? experts : P;
    return first + (P - first) / kMoeDecRows;
}

// Chunks one K slice covers, and the slices K then needs (the register-resident family's rule).
inline int64_t moe_dec_slice_chunks(const nf4_gemm_cfg& c) { return (int64_t)c.waves * c.strips; }
inline int64_t moe_dec_slices(const nf4_gemm_cfg& c, int64_t K) {
    const int64_t per = moe_dec_slice_chunks(c);
    return per > 0 ? (K / kChunkK + per - 1) / per : 0;
}

inline bool moe_dec_shape(int64_t P, int64_t N, int64_t K) {
    return P >= 1 && P <= NF4DQ_MOE_MAX_PAIRS && N >= (int64_t)kMoeDecCols && N % kMoeDecCols == 0 && K >= (int64_t)kChunkK &&
           K % kChunkK == 0;
}

// cfg fields: kernel = NF4DQ_GEMM_MOE_DEC; waves 8 / 16; depth = strips of the tile in flight per
// wave, 2 / 4; strips = 128-deep chunks per wave, 1 / 2 (four chunks per wave -- 64 registers of x
// fragments beside the ring -- do not fit the 128 registers that 4 waves per SIMD leave: the
// compiler spilled 49..65 of them, so the form is not instantiated); ksplit =
// ceil(K / 128 / (waves * strips)), at most 16.
inline bool valid_moe_dec_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t N, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_MOE_DEC || !moe_dec_shape(P, N, K)) return false;
    if (c.waves != 8 && c.waves != 16) return false;
    if (c.depth != 2 && c.depth != 4) return false;
    if (c.strips != 1 && c.strips != 2) return false;
    return c.ksplit >= 1 && c.ksplit <= kMoeDecKsplitMax && c.ksplit == moe_dec_slices(c, K);
}

// The library's choice.  The host never sees the routing, so it ASSUMES the spread
// moe_default_cfg assumes: min(P, experts) experts active, each with its share of the pairs, so
// active x ceil(share / 16) slots at work.  Among (waves, strips) = (8, 1), (16, 1), (16, 2)
// -- 8, 16 and 32 chunks a slice -- it takes the most slices K admits, and fewer (a deeper
// workgroup, whose routing prologue and table build are paid less often) only while slots x
// column tiles x slices still fills the CUs' resident workgroups.  Depth 4: the whole tile in
// flight.
// NOT SWEPT: the candidates and the fill rule are carried over from the small-M families'
// (nf4_gemm_plan.h); no cfg sweep of this entry has been run.
inline nf4_gemm_cfg moe_dec_default_cfg(int64_t P, int64_t experts, int64_t N, int64_t K, int cus) {
    const int64_t tiles = N / kMoeDecCols;
    const int64_t active = P < experts ? (P < 1 ? 1 : P) : (experts < 1 ? 1 : experts);
    const int64_t share = ((P < 1 ? 1 : P) + active - 1) / active;
    const int64_t slots = active * ((share + kMoeDecRows - 1) / kMoeDecRows);
    const int cand[3][2] = {{8, 1}, {16, 1}, {16, 2}};
    nf4_gemm_cfg best{NF4DQ_GEMM_MOE_DEC, 16, 4, 0, 2};
    for (const auto& wc : cand) {
        nf4_gemm_cfg c{NF4DQ_GEMM_MOE_DEC, wc[0], 4, 0, wc[1]};
        const int64_t ks = moe_dec_slices(c, K);
        if (ks > kMoeDecKsplitMax) continue;
        c.ksplit = (int)ks;
        if (best.ksplit == 0 || (ks < best.ksplit && slots * tiles * ks >= (int64_t)cus * moe_dec_resident(c))) best = c;
    }
    if (best.ksplit == 0) best.ksplit = (int)moe_dec_slices(best, K);  // K beyond every candidate: rejected by the shape rule
    return best;
}

// Launch geometry: grid = slots x column tiles x K slices (slice = block % ksplit, tile = block /
// ksplit % tiles, slot = block / (ksplit * tiles)); tickets = slots x column tiles.
struct MoeDecPlan {
    uint32_t grid, block, dyn, tiles, slots, chunks, tickets;
};
inline MoeDecPlan moe_dec_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    MoeDecPlan p{};
    p.tiles = (uint32_t)(N / kMoeDecCols);
    p.slots = (uint32_t)moe_dec_slots(P, experts);
    p.chunks = (uint32_t)(K / kChunkK);
    p.tickets = p.slots * p.tiles;
    p.grid = p.tickets * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = kMoeDecLdsBytes;
    return p;
}
// (ksplit slabs of P * N floats indexed by pair; nothing for one slice or a shape the entry rejects)
inline size_t moe_dec_workspace_need(int64_t P, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (!moe_dec_shape(P, N, K)) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * (size_t)P * (size_t)N * 4u : 0;
}

// moe_stack_shape, and K within what 16 slices of 16 waves x 2 chunks cover.
inline int moe_dec_stack_shape(const nf4_moe_experts& e, int64_t P) {
    if (const int rc = moe_stack_shape(e, P)) return rc;
    return e.K / kChunkK > (int64_t)kMoeDecKsplitMax * 16 * 2 ? NF4DQ_ERR_TOO_LARGE : NF4DQ_OK;
}

// Validates a call (nf4_gemm_bnb_moe's MoeCall) and answers what runs, as moe_check does: the same
// rules in the same order.  A cfg the caller names never falls back: invalid, NF4DQ_GEMM_MOE
// included, is NF4DQ_ERR_ARG.
inline int moe_dec_check(const MoeCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (!a.ex) return NF4DQ_ERR_ARG;
    const nf4_moe_experts& e = *a.ex;
    if (a.P < 0 || a.x_div < 1 || !moe_stack_fields_ok(e)) return NF4DQ_ERR_ARG;
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !a.y || !moe_stack_pointers_ok(e)) return NF4DQ_ERR_ARG;
    // 16-byte loads of x, 4-byte stores of y (8-byte ones in the reducer), 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.ids, 4)) return NF4DQ_ERR_ARG;
    if (const int rc = moe_dec_stack_shape(e, a.P)) return rc;
    if (!moe_stack_strides_ok(e)) return NF4DQ_ERR_SHAPE;
    nf4_gemm_cfg c = a.cfg ? *a.cfg : moe_dec_default_cfg(a.P, e.experts, e.N, e.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MOE_DEC;
    if (!valid_moe_dec_cfg(c, a.P, e.N, e.K)) return NF4DQ_ERR_ARG;
    if (c.ksplit > 1 && (size_t)moe_dec_plan(c, a.P, e.experts, e.N, e.K).tickets * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = moe_dec_workspace_need(a.P, e.N, e.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
