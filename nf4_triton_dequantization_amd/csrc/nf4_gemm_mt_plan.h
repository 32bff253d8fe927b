// nf4_gemm_mt_plan.h -- the host-side plan of the row-tiled fused GEMM (33..128 rows,
// batched decode; nf4_gemm_bnb_mt / nf4_gemm_bnb_mt_single), plain C++17 (no HIP): argument
// validation with the status codes, cfg validity, the library's choice from (M, N, K, CU
// count), the launch geometry, the LDS bytes and the workspace need.  Pure arithmetic, shared
// by the launcher (nf4_gemm_mt.hip) and a CPU check (tests/plan/gemm_mt_plan_check.cpp).
//
// The decomposition.  A workgroup of `waves` waves owns 32 * waves output columns, ALL
// row tiles (16 rows each, 2 / 4 / 6 / 8 of them) and one K slice.  A wave owns two
// 16-column strips: it loads and decodes its weights itself (each weight is decoded once in
// the launch's lifetime per workgroup, whatever M is) and multiplies the decoded fragment
// with every row tile; an x fragment read from LDS feeds the two strips' MFMAs.  x goes
// through LDS one 128-deep chunk at a time, two buffers.  K slices meet in an fp32 slab of
// the caller's workspace: the slice drawing the last ticket sums them in slice order.
#pragma once

#include "nf4_gemm_plan.h"

namespace nf4gemm {

constexpr int kMtStrips = 2;               // 16-column strips per wave
constexpr int kMtKsplitMax = 16;           // K slices of one launch
constexpr uint32_t kMtRowBytes = 256;      // a staged x row: one 128-deep chunk, 16 slots of 16 bytes, rotated per row
constexpr uint32_t kMtTableBytes = 1024 + 64 + 16;  // behind the x buffers: code2, the NF4 codes, the reducer flag

// Row tiles the kernel is instantiated for: ceil(M / 16) rounded up to even.
inline int mt_row_tiles(int64_t M) {
    const int t = (int)((M + 15) / 16);
    return t + (t & 1);
}
inline uint32_t mt_xbuf_bytes(int64_t M) { return 16u * (uint32_t)mt_row_tiles(M) * kMtRowBytes; }
inline bool mt_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ---- the family's rules, once: every entry below and in nf4_gemm_mt_swiglu_plan.h,
// nf4_gemm_moe_plan.h, nf4_gemm_moe_swiglu_plan.h and nf4_gemm_moe_down_plan.h is these rules
// under its own MtEntry ---------------------------------------------------------------------

struct MtEntry {
    int kernel;            // the entry's cfg.kernel
    int64_t max_rows;      // rows of one workgroup: M, or the P pairs one expert may get
    uint32_t wave_cols;    // output columns per wave: a workgroup owns wave_cols * waves
    uint32_t planes;       // fp32 planes a K slice stores
    uint32_t table_bytes;  // dynamic LDS behind the two x buffers
};
inline uint32_t mt_entry_cols(const MtEntry& e, const nf4_gemm_cfg& c) { return e.wave_cols * (uint32_t)c.waves; }
// Dynamic LDS: two x buffers and the tables (one array: its base is 16-byte aligned).
inline uint32_t mt_entry_lds(const MtEntry& e, int64_t rows) { return 2u * mt_xbuf_bytes(rows) + e.table_bytes; }
// The shapes an entry takes: rows within its bound, N in 64s, K in 128-deep chunks.
inline bool mt_entry_shape(const MtEntry& e, int64_t rows, int64_t N, int64_t K) {
    return rows >= 1 && rows <= e.max_rows && N >= 64 && N % 64 == 0 && K >= (int64_t)kChunkK && K % kChunkK == 0;
}

// cfg fields: kernel = the entry's; waves = waves per workgroup (2 / 4); depth = K stage in
// 128-deep chunks (1); ksplit = K slices (1 .. min(K / 128, 16)); strips = 16-row weight strips
// per wave (2; 0 = 2).  The row-tile count follows from the rows.
inline bool mt_entry_valid(const MtEntry& e, const nf4_gemm_cfg& c, int64_t rows, int64_t N, int64_t K) {
    if (c.kernel != e.kernel || rows < 1 || rows > e.max_rows || N < 64 || K < (int64_t)kChunkK) return false;
    if (c.waves != 2 && c.waves != 4) return false;
    if (c.depth != 1 || (c.strips != 0 && c.strips != kMtStrips)) return false;
    if (N % mt_entry_cols(e, c)) return false;
    if (c.ksplit < 1 || c.ksplit > kMtKsplitMax || c.ksplit > K / kChunkK) return false;
    return mt_entry_lds(e, rows) <= kLdsPerCu;
}

// The K-slice rule: as many slices as keep `tiles` x slices workgroups within the `capacity` of
// workgroups the CUs hold at once, while a slice keeps at least kMtSliceChunks chunks.
constexpr int kMtSliceChunks = 6;
inline int mt_entry_ksplit(int64_t capacity, int64_t tiles, int64_t K) {
    const int64_t chunks = K / kChunkK;
    int64_t ks = tiles > 0 ? capacity / tiles : 1;
    if (ks > kMtKsplitMax) ks = kMtKsplitMax;
    if (ks > chunks / kMtSliceChunks) ks = chunks / kMtSliceChunks;
    return ks < 1 ? 1 : (int)ks;
}

// Launch geometry: grid = groups x column tiles x K slices (slice = block % ksplit, tile =
// block / ksplit % tiles, group = block / (ksplit * tiles); groups: the experts, 1 for a dense
// entry), cps chunks per slice (the last slices may be short or empty: they hand in zeros).
struct MtPlan {
    uint32_t grid, block, dyn, tiles, chunks, cps, row_tiles;
};
inline MtPlan mt_entry_plan(const MtEntry& e, const nf4_gemm_cfg& c, int64_t rows, int64_t N, int64_t K, int64_t groups) {
    MtPlan p{};
    p.tiles = (uint32_t)(N / mt_entry_cols(e, c));
    p.chunks = (uint32_t)(K / kChunkK);
    p.cps = (p.chunks + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.row_tiles = (uint32_t)mt_row_tiles(rows);
    p.grid = p.tiles * (uint32_t)groups * (uint32_t)c.ksplit;
    p.block = 64u * (uint32_t)c.waves;
    p.dyn = mt_entry_lds(e, rows);
    return p;
}

// Workspace: the fused GEMM's layout -- the header (the tickets among its counters, 0 between
// calls) and per K slice `planes` planes of rows * N floats, 0 between calls (the reducer clears
// what it read, so the other entries may use the same workspace).  Nothing for one slice, nothing
// for a shape the entry rejects.
inline size_t mt_entry_workspace(const MtEntry& e, int64_t rows, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    if (!mt_entry_shape(e, rows, N, K)) return 0;
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * e.planes * (size_t)rows * (size_t)N * 4u : 0;
}

// The tail of every *_check, behind the entry's own argument rules: the cfg the caller names
// (kernel 0 = the entry's) or `c`, the library's choice; strips 0 = 2; an invalid cfg never falls
// back: NF4DQ_ERR_ARG; then the tickets (groups x column tiles; groups 0: a dense entry, whose
// shape bounds keep them within the counters), the 32-bit slab index and the workspace.
inline int mt_entry_resolve(const MtEntry& e, const nf4_gemm_cfg* named, nf4_gemm_cfg c, int64_t rows, int64_t N, int64_t K,
                            int64_t groups, const void* workspace, size_t workspace_bytes, nf4_gemm_cfg* out) {
    if (named) c = *named;
    if (named && c.kernel == 0) c.kernel = e.kernel;
    if (c.strips == 0) c.strips = kMtStrips;
    if (!mt_entry_valid(e, c, rows, N, K)) return NF4DQ_ERR_ARG;
    if (c.ksplit > 1 && (size_t)(N / mt_entry_cols(e, c)) * (size_t)groups * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const size_t need = mt_entry_workspace(e, rows, N, K, c);
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;  // slab entries are indexed with 32 bits
    if (need && (!workspace || workspace_bytes < need || !mt_aligned(workspace, 16))) return NF4DQ_ERR_ARG;
    *out = c;
    return NF4DQ_OK;
}

// ---- nf4_gemm_bnb_mt / nf4_gemm_bnb_mt_single ----------------------------------------------

// Two 16-column strips per wave (64 / 128 columns a workgroup), one plane.
constexpr MtEntry kMtEntry{NF4DQ_GEMM_MT, NF4DQ_GEMM_MT_MAX_M, 16u * kMtStrips, 1, kMtTableBytes};
inline uint32_t mt_cols(const nf4_gemm_cfg& c) { return mt_entry_cols(kMtEntry, c); }
inline uint32_t mt_lds_bytes(int64_t M) { return mt_entry_lds(kMtEntry, M); }
inline bool valid_mt_cfg(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) { return mt_entry_valid(kMtEntry, c, M, N, K); }

// The library's choice: 128-column workgroups where N allows (half the x traffic of 64-column
// ones), and as many K slices as keep the grid within the CUs while a slice keeps at least
// kMtSliceChunks chunks -- every slice costs a slab of M * N floats written, read and cleared,
// and ONE workgroup per tile reads all of them (measured on MI355X at M = 64 / 96 / 128: the
// fastest of 2..16 slices is 5 at 4096^2, 2 at 14336x4096, 8 at 4096x14336; a grid beyond the
// CUs or twice the slices costs 15 - 40 % more, profiles/gemm_mt/sweep_slices.jsonl).
inline nf4_gemm_cfg mt_default_cfg(int64_t M, int64_t N, int64_t K, int cus) {
    (void)M;
    nf4_gemm_cfg c{NF4DQ_GEMM_MT, N % 128 == 0 ? 4 : 2, 1, 1, kMtStrips};
    c.ksplit = mt_entry_ksplit(cus, N / mt_cols(c), K);
    return c;
}
inline MtPlan mt_plan(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) { return mt_entry_plan(kMtEntry, c, M, N, K, 1); }
// (one ticket per column tile, slabs of M * N floats)
inline size_t mt_workspace_need(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg& c) {
    return mt_entry_workspace(kMtEntry, M, N, K, c);
}

// One call of nf4_gemm_bnb_mt (single == false) or nf4_gemm_bnb_mt_single (a1 / code2 unused,
// a2 / n2 = the fp32 absmax and its length).
struct MtCall {
    bool single;
    const void* x;
    int64_t M;
    const uint8_t* packed;
    int64_t packed_len;
    const uint8_t* a1;
    int64_t nb;
    const float* code2;
    const float* a2;
    int64_t n2;
    int32_t blocksize, blocksize2;
    void* y;
    int32_t dtype;
    int64_t N, K;
    void* workspace;
    size_t workspace_bytes;
    const nf4_gemm_cfg* cfg;
};

// Validates a call and answers what runs: NF4DQ_OK and *out, or the status code.  A cfg the
// caller names never falls back: invalid is NF4DQ_ERR_ARG.
inline int mt_check(const MtCall& a, int cus, nf4_gemm_cfg* out) {
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (a.M < 0 || a.N < 0 || a.K < 0 || a.nb < 0 || a.n2 < 0 || a.packed_len < 0) return NF4DQ_ERR_ARG;
    if (a.blocksize < 64 || a.blocksize > 4096 || (a.blocksize & (a.blocksize - 1))) return NF4DQ_ERR_ARG;
    if (!a.single && (a.blocksize2 < 4 || (a.blocksize2 & (a.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
    if (!a.x || !a.packed || !a.a2 || !a.y || (!a.single && (!a.a1 || !a.code2))) return NF4DQ_ERR_ARG;
    // 16-byte loads of x and the packed weight, 8-byte stores of y
    if (!mt_aligned(a.x, 16) || !mt_aligned(a.packed, 16) || !mt_aligned(a.y, 8) || !mt_aligned(a.a2, 4)) return NF4DQ_ERR_ARG;
    if (a.blocksize != 64) return NF4DQ_ERR_SHAPE;  // larger statistics blocks: the composite
    if (!mt_entry_shape(kMtEntry, a.M, a.N, a.K)) return NF4DQ_ERR_SHAPE;
    if (a.N > (int64_t(1) << 18) || a.K > (int64_t(1) << 24)) return NF4DQ_ERR_TOO_LARGE;
    if (a.packed_len != a.N * (a.K / 2)) return NF4DQ_ERR_SHAPE;
    if (a.packed_len >= (int64_t(1) << 31) || a.M * a.K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    const int64_t nblk = a.N * a.K / 64;
    if (a.single ? a.n2 < nblk : (a.nb < nblk || a.n2 < (nblk + a.blocksize2 - 1) / a.blocksize2)) return NF4DQ_ERR_SHAPE;
    return mt_entry_resolve(kMtEntry, a.cfg, mt_default_cfg(a.M, a.N, a.K, cus), a.M, a.N, a.K, 0, a.workspace, a.workspace_bytes, out);
}

}  // namespace nf4gemm
