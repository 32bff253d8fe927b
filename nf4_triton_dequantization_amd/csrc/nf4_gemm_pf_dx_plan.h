// nf4_gemm_pf_dx_plan.h -- the host-side plan of the fused input-gradient GEMM of an NF4 weight
// (dx = g . W, 1..8192 rows; nf4_gemm_bnb_pf_dx / nf4_gemm_bnb_pf_dx_single), plain C++17 (no
// HIP): argument validation with the status codes, cfg validity, the library's choice from
// (M, N, K, CU count), the launch geometry, the LDS bytes and the workspace need.  Pure
// arithmetic, shared by the launcher (nf4_gemm_pf_dx.hip) and anything that asks the plan on a CPU.
//
// The decomposition is the prefill GEMM's (nf4_gemm_pf_plan.h) with N and K in each other's
// roles.  A workgroup of `waves` waves owns a block of BM = 32 * waves rows of g (128 or 256), one
// tile of 128 output columns k0 .. k0 + 127 and one slice of N; a wave owns 64 x 64 of it.  The
// reduction runs over N in steps of 64 weight rows: per step the workgroup stages the 64 x 64
// packed bytes of W[n0 .. n0 + 63][k0 .. k0 + 127] raw in LDS, forms the step's 128 block scales
// once, decodes the tile TRANSPOSED into [128 k][64 n] and stages BM x 64 of g beside it; all
// waves read their MFMA fragments from there.  Two buffers of each, one barrier per step.  Slices
// of N meet in the family's fp32 slab (nf4_gemm_mt_plan.h): one ticket per (row block, column
// tile), the last ticket reduces.
#pragma once

#include "nf4_gemm_pf_plan.h"

namespace nf4gemm {

constexpr uint32_t kDxStepN = 64;                      // weight rows of a step: one slot row of the decoded tile
constexpr uint32_t kDxCols = kPfCols;                  // output columns (k) of a workgroup's tile: two statistics blocks per weight row
constexpr uint32_t kDxRawBytes = kDxStepN * (kDxCols / 2u);      // a step's packed bytes: 64 rows x 64 bytes
constexpr uint32_t kDxScaleBytes = kDxStepN * (kDxCols / 64u) * 4u;  // a step's block scales: [2 blocks][64 rows] floats
constexpr int kDxSliceSteps = kPfSliceSteps;           // steps a slice of N keeps under the library's choice

// Dynamic LDS: [g 0][g 1][w 0][w 1][raw 0][raw 1][scales 0][scales 1][tables] -- 73 KiB + tables
// at 128 rows (two workgroups per CU), 105 KiB + tables at 256.
inline uint32_t dx_lds_bytes(const nf4_gemm_cfg& c) {
    return 2u * pf_block_rows(c) * kPfRowBytes + 2u * kDxCols * kPfRowBytes + 2u * kDxRawBytes + 2u * kDxScaleBytes +
           kPfTableBytes;
}

// The shapes the entries take: rows within the prefill bound, K (the output columns) in 128s, N
// (the reduction) in 64s.
inline bool dx_shape(int64_t M, int64_t N, int64_t K) {
    return M >= 1 && M <= NF4DQ_GEMM_PF_MAX_M && K >= (int64_t)kDxCols && K % kDxCols == 0 && N >= (int64_t)kDxStepN &&
           N % kDxStepN == 0;
}

// cfg fields: kernel = NF4DQ_GEMM_PF_DX; waves 4 / 8 = row blocks of 128 / 256; depth 1; ksplit =
// slices of N, 1 .. min(N / 64, 16); strips 0.
inline bool valid_dx_cfg(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) {
    if (c.kernel != NF4DQ_GEMM_PF_DX || !dx_shape(M, N, K)) return false;
    if (c.waves != 4 && c.waves != 8) return false;
    if (c.depth != 1 || c.strips != 0) return false;
    if (c.ksplit < 1 || c.ksplit > kPfKsplitMax || c.ksplit > N / kDxStepN) return false;
    return dx_lds_bytes(c) <= kLdsPerCu;
}

// The library's choice: pf_default_cfg's rule with N and K in each other's roles -- 256-row blocks
// past 128 rows, and as many slices of N as keep row blocks x column tiles x slices within the CUs
// while a slice keeps at least kDxSliceSteps steps.  CARRIED OVER from the prefill kernel's sweep,
// NOT swept for this kernel.
inline nf4_gemm_cfg dx_default_cfg(int64_t M, int64_t N, int64_t K, int cus) {
    nf4_gemm_cfg c{NF4DQ_GEMM_PF_DX, M > 128 ? 8 : 4, 1, 1, 0};
    const int64_t bm = pf_block_rows(c), wgs = ((M + bm - 1) / bm) * (K / kDxCols), steps = N / kDxStepN;
    int64_t ks = wgs > 0 ? cus / wgs : 1;
    if (ks > kPfKsplitMax) ks = kPfKsplitMax;
    if (ks > steps / kDxSliceSteps) ks = steps / kDxSliceSteps;
    c.ksplit = ks < 1 ? 1 : (int)ks;
    return c;
}

// Launch geometry: grid = row blocks x column tiles x slices (slice = block % ksplit, tile =
// block / ksplit % tiles, row block = block / (ksplit * tiles)), sps steps per slice (the last
// slices may be short or empty: they hand in zeros).
inline PfPlan dx_plan(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) {
    PfPlan p{};
    const uint32_t bm = pf_block_rows(c);
    p.tiles = (uint32_t)(K / kDxCols);
    p.row_blocks = (uint32_t)((M + bm - 1) / bm);
    p.steps = (uint32_t)(N / kDxStepN);
    p.sps = (p.steps + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.grid = p.row_blocks * p.tiles * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = dx_lds_bytes(c);
    return p;
}

// Workspace: the family's layout -- the header with the tickets, then ksplit slabs of M * K
// floats, all 0 between calls.  Nothing for one slice, nothing for a shape the entry rejects.
inline size_t dx_workspace_need(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (!dx_shape(M, N, K)) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * (size_t)M * (size_t)K * 4u : 0;
}

// Validates a call (MtCall with x = g [M][N] and y = dx [M][K]) and answers what runs: NF4DQ_OK
// with *launch and *out, or the status code -- pf_check's codes in pf_check's order.  A cfg the
// caller names never falls back.
inline int dx_check(const MtCall& a, int cus, nf4_gemm_cfg* out, bool* launch) {
    *launch = false;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (a.M < 0 || a.N < 0 || a.K < 0 || a.nb < 0 || a.n2 < 0 || a.packed_len < 0) return NF4DQ_ERR_ARG;
    if (a.blocksize < 64 || a.blocksize > 4096 || (a.blocksize & (a.blocksize - 1))) return NF4DQ_ERR_ARG;
    if (!a.single && (a.blocksize2 < 4 || (a.blocksize2 & (a.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
    if (!a.x || !a.packed || !a.a2 || !a.y || (!a.single && (!a.a1 || !a.code2))) return NF4DQ_ERR_ARG;
    // 16-byte loads of g, 8-byte loads of the packed weight (16 under 4 waves), 8-byte stores of dx
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.packed, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.a2, 4)) return NF4DQ_ERR_ARG;
    if (a.blocksize != 64) return NF4DQ_ERR_SHAPE;
    if (!dx_shape(a.M ? a.M : 1, a.N, a.K)) return NF4DQ_ERR_SHAPE;  // (no rows: the weight's rules still hold)
    if (a.N > (int64_t(1) << 18) || a.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    if (a.packed_len != a.N * (a.K / 2)) return NF4DQ_ERR_SHAPE;
    if (a.packed_len >= (int64_t(1) << 31) || a.M * a.N * 2 >= (int64_t(1) << 31) || a.M * a.K * 2 >= (int64_t(1) << 31))
        return NF4DQ_ERR_TOO_LARGE;
    const int64_t nblk = a.N * a.K / 64;
    if (a.single ? a.n2 < nblk : (a.nb < nblk || a.n2 < (nblk + a.blocksize2 - 1) / a.blocksize2)) return NF4DQ_ERR_SHAPE;
    if (a.M == 0) return NF4DQ_OK;  // all else valid: nothing to do, nothing launched
    nf4_gemm_cfg c = a.cfg ? *a.cfg : dx_default_cfg(a.M, a.N, a.K, cus);
    if (a.cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_PF_DX;
    if (!valid_dx_cfg(c, a.M, a.N, a.K)) return NF4DQ_ERR_ARG;
    const PfPlan p = dx_plan(c, a.M, a.N, a.K);
    if (c.ksplit > 1 && (size_t)p.row_blocks * p.tiles * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = dx_workspace_need(a.M, a.N, a.K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (need && (!a.workspace || a.workspace_bytes < need || !mt_aligned(a.workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    *launch = true;
    return NF4DQ_OK;
}

}  // namespace nf4gemm
