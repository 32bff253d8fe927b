// nf4_gemm_mt_swiglu_plan.h -- the host-side plan of the fused gate/up SwiGLU launch
// (nf4_gemm_bnb_mt_swiglu: h = silu(x . Wg^T) * (x . Wu^T) for 1..128 rows), plain C++17 (no
// HIP): argument validation with the status codes, cfg validity, the library's choice from
// (M, I, K, CU count), the launch geometry, the LDS bytes and the workspace need.  Pure
// arithmetic, shared by the launcher (nf4_gemm_mt_swiglu.hip) and a CPU check
// (tests/plan/gemm_mt_swiglu_plan_check.cpp).
//
// The decomposition is the row-tiled family's (nf4_gemm_mt_plan.h) with the wave's two strips
// given to the two weights: a workgroup of `waves` waves owns 16 * waves columns of h, ALL row
// tiles and one K slice; a wave owns 16 columns of h -- strip 0 is rows col .. col + 15 of the
// gate weight, strip 1 the same rows of the up weight, each with its own statistics, code2
// table, offset and blocksize2 -- so g and u of one output element end in one lane.  K slices
// meet in two fp32 planes per slice, [ksplit][2][M][I]; the slice drawing the last ticket sums
// each plane in slice order and applies the chain.
#pragma once

#include "nf4_gemm_mt_plan.h"

namespace nf4gemm {

constexpr uint32_t kSgTableBytes = 2 * 1024 + 64 + 16;  // behind the x buffers: two code2 tables, the NF4 codes, the reducer flag

inline uint32_t sg_cols(const nf4_gemm_cfg& c) { return 16u * (uint32_t)c.waves; }
// Dynamic LDS: the row-tiled layout with a second code2 table.
inline uint32_t sg_lds_bytes(int64_t M) { return 2u * mt_xbuf_bytes(M) + kSgTableBytes; }

// cfg fields: kernel = NF4DQ_GEMM_MT_SWIGLU; waves = waves per workgroup (2 / 4: 32 / 64 columns
// of h); depth = K stage in 128-deep chunks (1); ksplit = K slices (1 .. min(K / 128, 16));
// strips = 16-row weight strips per wave (2: one of gate, one of up; 0 = 2).
inline bool valid_sg_cfg(const nf4_gemm_cfg& c, int64_t M, int64_t I, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_MT_SWIGLU || M < 1 || M > NF4DQ_GEMM_MT_MAX_M || I < 64 || K < (int64_t)kChunkK) return false;
    if (c.waves != 2 && c.waves != 4) return false;
    if (c.depth != 1 || (c.strips != 0 && c.strips != kMtStrips)) return false;
    if (I % sg_cols(c)) return false;
    if (c.ksplit < 1 || c.ksplit > kMtKsplitMax || c.ksplit > K / kChunkK) return false;
    return sg_lds_bytes(M) <= kLdsPerCu;
}

// The library's choice: mt_default_cfg's rule over this launch's column tiles -- four waves
// (64 columns of h, 128 weight rows: I % 64 == 0 always allows them) and as many K slices as
// keep the grid within the CUs while a slice keeps at least kMtSliceChunks chunks.  A slice
// costs two planes of M * I floats written, read and cleared.  Measured on MI355X over 2 / 4
// waves x 1..16 slices (profiles/gemm_mt_swiglu/sweep_slices.jsonl): at 14336x4096 and
// 11008x4096 (224 / 172 tiles on 256 CUs) the rule's ONE slice is the fastest count from 48
// rows up -- two cost 1.3x - 1.4x at 64 and 128 rows, more cost more -- and within 2.5 % of two
// at 32; four waves are within 3 % of two at 48 and 64 rows and 5 - 16 % ahead at 32, 96 and
// 128.  (Up to 8 rows two slices measure 6 - 9 % faster than one; the small-M entries take half
// the time there anyway.)
inline nf4_gemm_cfg sg_default_cfg(int64_t M, int64_t I, int64_t K, int cus) {
    (void)M;
    nf4_gemm_cfg c{NF4DQ_GEMM_MT_SWIGLU, 4, 1, 1, kMtStrips};
    const int64_t tiles = I / sg_cols(c), chunks = K / kChunkK;
    int64_t ks = tiles > 0 ? cus / tiles : 1;
    if (ks > kMtKsplitMax) ks = kMtKsplitMax;
    if (ks > chunks / kMtSliceChunks) ks = chunks / kMtSliceChunks;
    c.ksplit = ks < 1 ? 1 : (int)ks;
    return c;
}

// Launch geometry: grid = column tiles x K slices (slice = block % ksplit), cps chunks per slice
// (the last slices may be short or empty: they hand in zeros).
inline MtPlan sg_plan(const nf4_gemm_cfg& c, int64_t M, int64_t I, int64_t K) {
    MtPlan p{};
    p.tiles = (uint32_t)(I / sg_cols(c));
    p.chunks = (uint32_t)(K / kChunkK);
    p.cps = (p.chunks + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.row_tiles = (uint32_t)mt_row_tiles(M);
    p.grid = p.tiles * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = sg_lds_bytes(M);
    return p;
}

// Workspace: the row-tiled family's layout and contract -- the header (one ticket per column
// tile) and, per K slice, the gate plane and the up plane of M * I floats each, all 0 between
// calls.  Nothing for one slice, nothing for a shape the entry rejects.
inline size_t sg_workspace_need(int64_t M, int64_t I, int64_t K, const nf4_gemm_cfg& c) {
    if (M < 1 || M > NF4DQ_GEMM_MT_MAX_M || I < 64 || I % 64 || K < (int64_t)kChunkK || K % kChunkK) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * 2u * (size_t)M * (size_t)I * 4u : 0;
}

// One call of nf4_gemm_bnb_mt_swiglu: mats[0] is the gate weight, mats[1] the up weight.
struct SgCall {
    bool single;
    const void* x;
    int64_t M, K;
    const nf4_gemm_bnb_mat* mats;
    int32_t act;
    void* h;
    int32_t dtype;
    void* workspace;
    size_t workspace_bytes;
    const nf4_gemm_cfg* cfg;
};

// Validates a call and answers what runs: NF4DQ_OK and *out, or the status code -- mt_check's
// rules and order, applied to each weight.  A cfg the caller names never falls back.
inline int sg_check(const SgCall& a, int cus, nf4_gemm_cfg* out) {
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (a.act != NF4DQ_ACT_SILU) return NF4DQ_ERR_ARG;
    if (a.M < 0 || a.K < 0 || !a.mats || !a.x || !a.h) return NF4DQ_ERR_ARG;
    for (int i = 0; i < 2; ++i) {
        const nf4_gemm_bnb_mat& m = a.mats[i];
        if (m.N < 0 || m.n2 < 0 || m.packed_len < 0 || (!a.single && m.nb < 0)) return NF4DQ_ERR_ARG;
        if (m.blocksize < 64 || m.blocksize > 4096 || (m.blocksize & (m.blocksize - 1))) return NF4DQ_ERR_ARG;
        if (!a.single && (m.blocksize2 < 4 || (m.blocksize2 & (m.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
        if (!m.packed || !m.absmax2 || (!a.single && (!m.absmax_q || !m.code2))) return NF4DQ_ERR_ARG;
        if (!mt_aligned(m.packed, 16) || !mt_aligned(m.absmax2, 4)) return NF4DQ_ERR_ARG;
    }
    // 16-byte loads of x and the packed weights, 8-byte stores of h
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.h, 8)) return NF4DQ_ERR_ARG;
    if (a.mats[0].blocksize != 64 || a.mats[1].blocksize != 64) return NF4DQ_ERR_SHAPE;  // larger statistics blocks: the composite
    const int64_t I = a.mats[0].N;
    if (a.mats[1].N != I) return NF4DQ_ERR_SHAPE;
    if (a.M < 1 || a.M > NF4DQ_GEMM_MT_MAX_M || I < 64 || I % 64 || a.K < (int64_t)kChunkK || a.K % kChunkK)
        return NF4DQ_ERR_SHAPE;
    if (I > (int64_t(1) << 18) || a.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    const int64_t nblk = I * a.K / 64;
    for (int i = 0; i < 2; ++i) {
        const nf4_gemm_bnb_mat& m = a.mats[i];
        if (m.packed_len != I * (a.K / 2)) return NF4DQ_ERR_SHAPE;
        if (m.packed_len >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
        if (a.single ? m.n2 < nblk : (m.nb < nblk || m.n2 < (nblk + m.blocksize2 - 1) / m.blocksize2)) return NF4DQ_ERR_SHAPE;
    }
    if (a.M * a.K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    nf4_gemm_cfg c = a.cfg ? *a.cfg : sg_default_cfg(a.M, I, a.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MT_SWIGLU;
    if (c.strips == 0) c.strips = kMtStrips;
    if (!valid_sg_cfg(c, a.M, I, a.K)) return NF4DQ_ERR_ARG;
    const size_t need = sg_workspace_need(a.M, I, a.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // plane entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
