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
inline uint32_t moe_lds_bytes(int64_t P) { return 2u * mt_xbuf_bytes(P) + kMoeTableBytes; }

// cfg fields: kernel = NF4DQ_GEMM_MOE; the rest as the row-tiled family's (waves 2 / 4, depth
// 1, ksplit 1 .. min(K / 128, 16), strips 2 or 0).
inline bool valid_moe_cfg(const nf4_gemm_cfg& c, int64_t P, int64_t N, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_MOE || P < 1 || P > NF4DQ_MOE_MAX_PAIRS || N < 64 || K < (int64_t)kChunkK) return false;
    if (c.waves != 2 && c.waves != 4) return false;
    if (c.depth != 1 || (c.strips != 0 && c.strips != kMtStrips)) return false;
    if (N % mt_cols(c)) return false;
    if (c.ksplit < 1 || c.ksplit > kMtKsplitMax || c.ksplit > K / kChunkK) return false;
    return moe_lds_bytes(P) <= kLdsPerCu;
}

// Workgroups of 4 waves a CU holds at once, by row tiles: two with two row tiles (at most 256
// registers a lane, the kernel's launch bound), one beyond.
inline int moe_resident(int64_t P) { return moe_row_tiles(P) <= 2 ? 2 : 1; }

// The library's choice.  The host never sees the routing, so the plan ASSUMES the spread a
// router aims at: min(P, experts) experts active, each with its share of the pairs.  Under it
// the working grid is active x column tiles x K slices, and the K slices are the row-tiled
// family's rule on that grid: as many as keep it within what the CUs hold at once
// (moe_resident() workgroups each) while a slice keeps at least kMoeSliceChunks chunks.  Measured
// on MI355X at Mixtral's shapes with 8 experts (profiles/gemm_moe/sweep_slices.jsonl, 1..16
// slices): the rule's count is the fastest at 7 of the 8 (shape, T) cells and within 9 % at the
// eighth (4096 x 14336 at 4 tokens: 2 slices 102 us, 3 slices 94 us); a grid beyond what the CUs
// hold costs up to 3 x.  The kernel decodes every weight on the VALU with one or two waves per
// SIMD, so with few rows it is bound by that decode, not by HBM: more resident workgroups are
// what the slices buy.  Fewer active experts than assumed (pairs piling onto
// one expert) leave CUs idle, never oversubscribed; the result is right for every routing, only
// the speed depends on it.
constexpr int kMoeSliceChunks = 6;
inline nf4_gemm_cfg moe_default_cfg(int64_t P, int64_t experts, int64_t N, int64_t K, int cus) {
    nf4_gemm_cfg c{NF4DQ_GEMM_MOE, N % 128 == 0 ? 4 : 2, 1, 1, kMtStrips};
    const int64_t active = P < experts ? (P < 1 ? 1 : P) : (experts < 1 ? 1 : experts);
    const int64_t tiles = N / mt_cols(c) * active, chunks = K / kChunkK;
    int64_t ks = tiles > 0 ? (int64_t)cus * moe_resident(P) / tiles : 1;
    if (ks > kMtKsplitMax) ks = kMtKsplitMax;
    if (ks > chunks / kMoeSliceChunks) ks = chunks / kMoeSliceChunks;
    c.ksplit = ks < 1 ? 1 : (int)ks;
    return c;
}

// Launch geometry: grid = experts x column tiles x K slices (slice = block % ksplit, tile =
// block / ksplit % tiles, expert = block / (ksplit * tiles)); cps chunks per slice (the last
// slices may be short or empty: they hand in zeros); tickets = experts x column tiles.
struct MoePlan {
    uint32_t grid, block, dyn, tiles, chunks, cps, row_tiles, tickets;
};
inline MoePlan moe_plan(const nf4_gemm_cfg& c, int64_t P, int64_t experts, int64_t N, int64_t K) {
    MoePlan p{};
    p.tiles = (uint32_t)(N / mt_cols(c));
    p.chunks = (uint32_t)(K / kChunkK);
    p.cps = (p.chunks + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.row_tiles = (uint32_t)moe_row_tiles(P);
    p.tickets = p.tiles * (uint32_t)experts;
    p.grid = p.tickets * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = moe_lds_bytes(P);
    return p;
}

// Workspace: the fused GEMM's layout -- the header (one ticket per (expert, column tile) among
// its counters, 0 between calls) and ksplit slabs of P * N floats indexed by pair, 0 between
// calls.  Nothing for one slice, nothing for a shape the entry rejects.
inline size_t moe_workspace_need(int64_t P, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (P < 1 || P > NF4DQ_MOE_MAX_PAIRS || N < 64 || N % 64 || K < (int64_t)kChunkK || K % kChunkK) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * (size_t)P * (size_t)N * 4u : 0;
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
    const bool single = e.single != 0;
    if (a.P < 0 || e.N < 0 || e.K < 0 || e.packed_stride < 0 || e.nb_stride < 0 || e.n2_stride < 0 || e.code2_stride < 0)
        return NF4DQ_ERR_ARG;
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS || a.x_div < 1) return NF4DQ_ERR_ARG;
    if (e.blocksize < 64 || e.blocksize > 4096 || (e.blocksize & (e.blocksize - 1))) return NF4DQ_ERR_ARG;
    if (!single && (e.blocksize2 < 4 || (e.blocksize2 & (e.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
    if (a.P == 0) return NF4DQ_OK;
    if (!a.x || !a.ids || !e.packed || !e.absmax2 || !a.y || (!single && (!e.absmax_q || !e.code2))) return NF4DQ_ERR_ARG;
    // 16-byte loads of x and the packed weight (every expert's: the stride keeps the alignment),
    // 8-byte stores of y, 4-byte loads of the ids
    if (!mt_aligned(a.x, 16) || !mt_aligned(e.packed, 16) || e.packed_stride % 16 || !mt_aligned(a.y, 8) ||
        !mt_aligned(e.absmax2, 4) || !mt_aligned(a.ids, 4) || !mt_aligned(e.code2, 4) || !mt_aligned(e.offset, 4))
        return NF4DQ_ERR_ARG;
    if (e.blocksize != 64) return NF4DQ_ERR_SHAPE;  // larger statistics blocks: the per-expert loop
    if (a.P > NF4DQ_MOE_MAX_PAIRS || e.N < 64 || e.N % 64 || e.K < (int64_t)kChunkK || e.K % kChunkK) return NF4DQ_ERR_SHAPE;
    if (e.N > (int64_t(1) << 18) || e.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    const int64_t plen = e.N * (e.K / 2), nblk = e.N * e.K / 64;
    if (plen >= (int64_t(1) << 31) || a.P * e.K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    if (e.packed_stride < plen) return NF4DQ_ERR_SHAPE;
    if (single ? e.n2_stride < nblk : (e.nb_stride < nblk || e.n2_stride < (nblk + e.blocksize2 - 1) / e.blocksize2))
        return NF4DQ_ERR_SHAPE;
    if (!single && e.code2_stride != 0 && e.code2_stride < 256) return NF4DQ_ERR_SHAPE;
    nf4_gemm_cfg c = a.cfg ? *a.cfg : moe_default_cfg(a.P, e.experts, e.N, e.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MOE;
    if (c.strips == 0) c.strips = kMtStrips;
    if (!valid_moe_cfg(c, a.P, e.N, e.K)) return NF4DQ_ERR_ARG;
    if (c.ksplit > 1 && (size_t)moe_plan(c, a.P, e.experts, e.N, e.K).tickets * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = moe_workspace_need(a.P, e.N, e.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
