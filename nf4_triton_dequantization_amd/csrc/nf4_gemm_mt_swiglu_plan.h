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

// The row-tiled family's rules (nf4_gemm_mt_plan.h) over 16 columns of h per wave (32 / 64 a
// workgroup), two planes per slice -- [ksplit][2][M][I]: the gate plane and the up plane -- and
// the row-tiled LDS layout with a second code2 table.
constexpr MtEntry kSgEntry{NF4DQ_GEMM_MT_SWIGLU, NF4DQ_GEMM_MT_MAX_M, 16u, 2, kSgTableBytes};
inline uint32_t sg_cols(const nf4_gemm_cfg& c) { return mt_entry_cols(kSgEntry, c); }
inline uint32_t sg_lds_bytes(int64_t M) { return mt_entry_lds(kSgEntry, M); }
inline bool valid_sg_cfg(const nf4_gemm_cfg& c, int64_t M, int64_t I, int64_t K) { return mt_entry_valid(kSgEntry, c, M, I, K); }

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
    c.ksplit = mt_entry_ksplit(cus, I / sg_cols(c), K);
    return c;
}
inline MtPlan sg_plan(const nf4_gemm_cfg& c, int64_t M, int64_t I, int64_t K) { return mt_entry_plan(kSgEntry, c, M, I, K, 1); }
inline size_t sg_workspace_need(int64_t M, int64_t I, int64_t K, const nf4_gemm_cfg& c) {
    return mt_entry_workspace(kSgEntry, M, I, K, c);
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
    if (!mt_entry_shape(kSgEntry, a.M, I, a.K)) return NF4DQ_ERR_SHAPE;
    if (I > (int64_t(1) << 18) || a.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    const int64_t nblk = I * a.K / 64;
    for (int i = 0; i < 2; ++i) {
        const nf4_gemm_bnb_mat& m = a.mats[i];
        if (m.packed_len != I * (a.K / 2)) return NF4DQ_ERR_SHAPE;
        if (m.packed_len >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
        if (a.single ? m.n2 < nblk : (m.nb < nblk || m.n2 < (nblk + m.blocksize2 - 1) / m.blocksize2)) return NF4DQ_ERR_SHAPE;
    }
    if (a.M * a.K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    return mt_entry_resolve(kSgEntry, a.cfg, sg_default_cfg(a.M, I, a.K, cus), a.M, I, a.K, 0, a.workspace, a.workspace_bytes, out);
}

}  // namespace nf4gemm
