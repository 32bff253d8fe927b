// nf4_gemm_pf_plan.h -- the host-side plan of the prefill fused GEMM (1..8192 rows;
// nf4_gemm_bnb_pf / nf4_gemm_bnb_pf_single), plain C++17 (no HIP): argument validation with the
// status codes, cfg validity, the library's choice from (M, N, K, CU count), the launch
// geometry, the LDS bytes and the workspace need.  Pure arithmetic, shared by the launcher
// (nf4_gemm_pf.hip) and anything that wants to ask the plan on a CPU.
//
// The decomposition.  A workgroup of `waves` waves owns a block of BM = 32 * waves rows (128 or
// 256), one tile of 128 columns and one K slice; a wave owns 64 x 64 of it.  Per 64-deep K step
// the workgroup decodes its 128 x 64 weights ONCE into LDS (every thread a piece of one
// statistics block) and stages BM x 64 of x beside them; all waves read their MFMA fragments
// from there.  Two buffers each, one barrier per step.  K slices meet in the family's fp32 slab
// (nf4_gemm_mt_plan.h): one ticket per (row block, column tile), the last ticket reduces.
#pragma once

#include "nf4_gemm_mt_plan.h"

namespace nf4gemm {

constexpr uint32_t kPfStepK = 64;        // K depth of a step: one statistics block per weight row
constexpr uint32_t kPfCols = 128;        // columns of a workgroup's tile
constexpr uint32_t kPfRowBytes = 128;    // a staged row of x or of decoded weights: 64 16-bit values, 8 rotated slots
constexpr int kPfKsplitMax = kMtKsplitMax;
constexpr uint32_t kPfTableBytes = kMtTableBytes;  // behind the buffers: code2, the NF4 codes, the reducer flag
constexpr int kPfSliceSteps = 16;        // steps a K slice keeps under the library's choice

inline uint32_t pf_block_rows(const nf4_gemm_cfg& c) { return 32u * (uint32_t)c.waves; }
// Dynamic LDS: [x 0][x 1][w 0][w 1][tables] -- 64 KiB + tables at 128 rows (two workgroups per
// CU), 96 KiB + tables at 256.
inline uint32_t pf_lds_bytes(const nf4_gemm_cfg& c) {
    return 2u * pf_block_rows(c) * kPfRowBytes + 2u * kPfCols * kPfRowBytes + kPfTableBytes;
}

// The shapes the entries take: rows within the bound, N in 128s, K as the row-tiled family's.
inline bool pf_shape(int64_t M, int64_t N, int64_t K) {
    return M >= 1 && M <= NF4DQ_GEMM_PF_MAX_M && N >= (int64_t)kPfCols && N % kPfCols == 0 && K >= (int64_t)kChunkK &&
           K % kChunkK == 0;
}

// cfg fields: kernel = NF4DQ_GEMM_PF; waves 4 / 8 = row blocks of 128 / 256; depth 1; ksplit =
// K slices, 1 .. min(K / 64, 16); strips 0.
inline bool valid_pf_cfg(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_PF || !pf_shape(M, N, K)) return false;
    if (c.waves != 4 && c.waves != 8) return false;
    if (c.depth != 1 || c.strips != 0) return false;
    if (c.ksplit < 1 || c.ksplit > kPfKsplitMax || c.ksplit > K / kPfStepK) return false;
    return pf_lds_bytes(c) <= kLdsPerCu;
}

// The library's choice: 256-row blocks as soon as there is more than one 128-row block (half the
// weight decodes and half the weight traffic per row; measured faster than two 128-row blocks
// already at 129 rows), and as many K slices as keep row blocks x column tiles x slices within the
// CUs while a slice keeps at least kPfSliceSteps steps (measured on MI355X at 4096^2 and
// 14336x4096, 129 / 512 / 2048 rows: the fastest cfg of the sweep in five cells of six, 1.3 %
// behind it in the sixth; slices of 8 steps cost 14 % at 4096^2 and 129 rows;
// profiles/gemm_pf/sweep.jsonl).
inline nf4_gemm_cfg pf_default_cfg(int64_t M, int64_t N, int64_t K, int cus) {
    nf4_gemm_cfg c{NF4DQ_GEMM_PF, M > 128 ? 8 : 4, 1, 1, 0};
    const int64_t bm = pf_block_rows(c), wgs = ((M + bm - 1) / bm) * (N / kPfCols), steps = K / kPfStepK;
    int64_t ks = wgs > 0 ? cus / wgs : 1;
    if (ks > kPfKsplitMax) ks = kPfKsplitMax;
    if (ks > steps / kPfSliceSteps) ks = steps / kPfSliceSteps;
    c.ksplit = ks < 1 ? 1 : (int)ks;
    return c;
}

// Launch geometry: grid = row blocks x column tiles x K slices (slice = block % ksplit, tile =
// block / ksplit % tiles, row block = block / (ksplit * tiles)), sps steps per slice (the last
// slices may be short or empty: they hand in zeros).
struct PfPlan {
    uint32_t grid, block, dyn, tiles, row_blocks, steps, sps;
};
inline PfPlan pf_plan(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) {
    PfPlan p{};
    const uint32_t bm = pf_block_rows(c);
    p.tiles = (uint32_t)(N / kPfCols);
    p.row_blocks = (uint32_t)((M + bm - 1) / bm);
    p.steps = (uint32_t)(K / kPfStepK);
    p.sps = (p.steps + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.grid = p.row_blocks * p.tiles * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = pf_lds_bytes(c);
    return p;
}

// Workspace: the family's layout -- the header with the tickets, then ksplit slabs of M * N
// floats, all 0 between calls.  Nothing for one slice, nothing for a shape the entry rejects.
inline size_t pf_workspace_need(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (!pf_shape(M, N, K)) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * (size_t)M * (size_t)N * 4u : 0;
}

// Validates a call (MtCall: the row-tiled entries' argument list) and answers what runs:
// NF4DQ_OK with *launch and *out, or the status code.  A cfg the caller names never falls back.
inline int pf_check(const MtCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (a.M < 0 || a.N < 0 || a.K < 0 || a.nb < 0 || a.n2 < 0 || a.packed_len < 0) return NF4DQ_ERR_ARG;
    if (a.blocksize < 64 || a.blocksize > 4096 || (a.blocksize & (a.blocksize - 1))) return NF4DQ_ERR_ARG;
    if (!a.single && (a.blocksize2 < 4 || (a.blocksize2 & (a.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
    if (!a.x || !a.packed || !a.a2 || !a.y || (!a.single && (!a.a1 || !a.code2))) return NF4DQ_ERR_ARG;
    // 16-byte loads of x, 8-byte loads of the packed weight (16 under 4 waves), 8-byte stores of y
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.packed, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.a2, 4)) return NF4DQ_ERR_ARG;
    if (a.blocksize != 64) return NF4DQ_ERR_SHAPE;
    if (!pf_shape(a.M ? a.M : 1, a.N, a.K)) return NF4DQ_ERR_SHAPE;  // (no rows: the weight's rules still hold)
    if (a.N > (int64_t(1) << 18) || a.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    if (a.packed_len != a.N * (a.K / 2)) return NF4DQ_ERR_SHAPE;
    if (a.packed_len >= (int64_t(1) << 31) || a.M * a.K * 2 >= (int64_t(1) << 31) || a.M * a.N * 2 >= (int64_t(1) << 31))
        return NF4DQ_ERR_TOO_LARGE;
    const int64_t nblk = a.N * a.K / 64;
    if (a.single ? a.n2 < nblk : (a.nb < nblk || a.n2 < (nblk + a.blocksize2 - 1) / a.blocksize2)) return NF4DQ_ERR_SHAPE;
    if (a.M == 0) return NF4DQ_OK;  // all else valid: nothing to do, nothing launched
    nf4_gemm_cfg c = a.cfg ? *a.cfg : pf_default_cfg(a.M, a.N, a.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_PF;
    if (!valid_pf_cfg(c, a.M, a.N, a.K)) return NF4DQ_ERR_ARG;
    const PfPlan p = pf_plan(c, a.M, a.N, a.K);
    if (c.ksplit > 1 && (size_t)p.row_blocks * p.tiles * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = pf_workspace_need(a.M, a.N, a.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
