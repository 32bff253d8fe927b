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

inline uint32_t msg_cols(const nf4_gemm_cfg& c) { return sg_cols(c); }
inline uint32_t msg_lds_bytes(int64_t P) { return 2u * mt_xbuf_bytes(P) + kMsgTableBytes; }

// cfg fields: kernel = NF4DQ_GEMM_MOE_SWIGLU; the rest as the SwiGLU launch's (waves 2 / 4: 32 /
// 64 columns of h, depth 1, ksplit 1 .. min(K / 128, 16), strips 2 or 0).
inline bool valid_msg_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t I, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_MOE_SWIGLU || P < 1 || P > NF4DQ_MOE_MAX_PAIRS || I < 64 || K < (int64_t)kChunkK) return false;
    if (c.waves != 2 && c.waves != 4) return false;
    if (c.depth != 1 || (c.strips != 0 && c.strips != kMtStrips)) return false;
    if (I % msg_cols(c)) return false;
    if (c.ksplit < 1 || c.ksplit > kMtKsplitMax || c.ksplit > K / kChunkK) return false;
    return msg_lds_bytes(P) <= kLdsPerCu;
}

// Workgroups of 4 waves a CU holds at once, by row tiles: the kernel's launch bound.  With two row
// tiles the two-table kernel and its expf epilogue stay within 256 registers without a spill
// (DESIGN section 4b), so two are resident as in the expert GEMM; one beyond.
inline int msg_resident(int64_t P) { return moe_row_tiles(P) <= 2 ? 2 : 1; }

// The library's choice: moe_default_cfg's rule over this launch's column tiles -- four waves (64
// columns of h, 128 weight rows: I % 64 == 0 always allows them), min(P, experts) experts assumed
// active, and as many K slices as keep active x tiles x slices within what the CUs hold at once
// (msg_resident() workgroups each) while a slice keeps at least kMoeSliceChunks chunks.  A slice
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
    const int64_t active = P < experts ? (P < 1 ? 1 : P) : (experts < 1 ? 1 : experts);
    const int64_t tiles = I / msg_cols(c) * active, chunks = K / kChunkK;
    int64_t ks = tiles > 0 ? (int64_t)cus * msg_resident(P) / tiles : 1;
    if (ks > kMtKsplitMax) ks = kMtKsplitMax;
    if (ks > chunks / kMoeSliceChunks) ks = chunks / kMoeSliceChunks;
    c.ksplit = ks < 1 ? 1 : (int)ks;
    return c;
}

// Launch geometry: the expert GEMM's (slice = block % ksplit, tile = block / ksplit % tiles,
// expert = block / (ksplit * tiles)) over column tiles of 16 * waves.
inline MoePlan msg_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t I, int64_t K) {
    MoePlan p{};
    p.tiles = (uint32_t)(I / msg_cols(c));
    p.chunks = (uint32_t)(K / kChunkK);
    p.cps = (p.chunks + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.row_tiles = (uint32_t)moe_row_tiles(P);
    p.tickets = p.tiles * (uint32_t)experts;
    p.grid = p.tickets * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = msg_lds_bytes(P);
    return p;
}

// Workspace: the header (one ticket per (expert, column tile) among its counters) and, per K
// slice, the gate plane and the up plane of P * I floats indexed by pair, all 0 between calls.
// Nothing for one slice, nothing for a shape the entry rejects.
inline size_t msg_workspace_need(int64_t P, int64_t I, int64_t K, const nf4_gemm_cfg& c) {
    if (P < 1 || P > NF4DQ_MOE_MAX_PAIRS || I < 64 || I % 64 || K < (int64_t)kChunkK || K % kChunkK) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * 2u * (size_t)P * (size_t)I * 4u : 0;
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
    if (a.P < 0 || a.x_div < 1) return NF4DQ_ERR_ARG;
    for (int i = 0; i < 2; ++i) {
        const nf4_moe_experts& e = a.ex[i];
        if (e.N < 0 || e.K < 0 || e.packed_stride < 0 || e.nb_stride < 0 || e.n2_stride < 0 || e.code2_stride < 0)
            return NF4DQ_ERR_ARG;
        if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return NF4DQ_ERR_ARG;
        if (e.blocksize < 64 || e.blocksize > 4096 || (e.blocksize & (e.blocksize - 1))) return NF4DQ_ERR_ARG;
        if (!e.single && (e.blocksize2 < 4 || (e.blocksize2 & (e.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
    }
    const nf4_moe_experts& g = a.ex[0];
    const nf4_moe_experts& u = a.ex[1];
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !a.h) return NF4DQ_ERR_ARG;
    for (int i = 0; i < 2; ++i) {
        const nf4_moe_experts& e = a.ex[i];
        if (!e.packed || !e.absmax2 || (!e.single && (!e.absmax_q || !e.code2))) return NF4DQ_ERR_ARG;
        if (!mt_aligned(e.packed, 16) || e.packed_stride % 16 || !mt_aligned(e.absmax2, 4) || !mt_aligned(e.code2, 4) ||
            !mt_aligned(e.offset, 4))
            return NF4DQ_ERR_ARG;
    }
    // 16-byte loads of x and the packed weights, 8-byte stores of h, 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.h, 8) || !mt_aligned(a.ids, 4)) return NF4DQ_ERR_ARG;
    if (g.N != u.N || g.K != u.K || g.experts != u.experts || (g.single != 0) != (u.single != 0)) return NF4DQ_ERR_SHAPE;
    if (g.blocksize != 64 || u.blocksize != 64) return NF4DQ_ERR_SHAPE;  // larger statistics blocks: the composite
    const bool single = g.single != 0;
    const int64_t I = g.N, K = g.K;
    if (a.P > NF4DQ_MOE_MAX_PAIRS || I < 64 || I % 64 || K < (int64_t)kChunkK || K % kChunkK) return NF4DQ_ERR_SHAPE;
    if (I > (int64_t(1) << 18) || K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    const int64_t plen = I * (K / 2), nblk = I * K / 64;
    if (plen >= (int64_t(1) << 31) || a.P * K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    for (int i = 0; i < 2; ++i) {
        const nf4_moe_experts& e = a.ex[i];
        if (e.packed_stride < plen) return NF4DQ_ERR_SHAPE;
        if (single ? e.n2_stride < nblk : (e.nb_stride < nblk || e.n2_stride < (nblk + e.blocksize2 - 1) / e.blocksize2))
            return NF4DQ_ERR_SHAPE;
        if (!single && e.code2_stride != 0 && e.code2_stride < 256) return NF4DQ_ERR_SHAPE;
    }
    nf4_gemm_cfg c = a.cfg ? *a.cfg : msg_default_cfg(a.P, g.experts, I, K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MOE_SWIGLU;
    if (c.strips == 0) c.strips = kMtStrips;
    if (!valid_msg_cfg(c, a.P, I, K)) return NF4DQ_ERR_ARG;
    if (c.ksplit > 1 && (size_t)msg_plan(c, a.P, g.experts, I, K).tickets * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = msg_workspace_need(a.P, I, K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // plane entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
