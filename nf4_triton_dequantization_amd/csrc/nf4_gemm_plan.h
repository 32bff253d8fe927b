// nf4_gemm_plan.h -- the host-side plan of the fused GEMM, plain C++17 (no HIP): the
// constants host and kernels agree on, cfg validity, the library's choice of kernel and
// decomposition with its fallbacks, the workspace size and every family's launch
// geometry.  Pure arithmetic of (M, K, the weights, the CU count), shared by the dispatch
// (nf4_gemm.hip), the launchers (nf4_gemm_launch_*.hip) and a CPU check
// (tests/plan/gemm_plan_check.cpp) that pins the choices without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/nf4_dequant.h"
#include "nf4_fastdiv.h"

namespace nf4gemm {

constexpr uint32_t kChunkK = 128;   // K depth of a chunk: 128-deep, shared-activation, register-resident
constexpr uint32_t kSChunkK = 256;  // streaming, persistent
constexpr int kXR = 8;              // x staging: 16-byte pieces per thread and row tile
constexpr uint32_t kLdsX = 0;       // dynamic LDS: [x slice][zero block][partials]
constexpr int kVsMax = 16;          // chunks per wave covered by the vector-scale form
constexpr int kGroupMax = 8, kK128GroupMax = 8;  // weights of one launch
static_assert(kK128GroupMax == NF4DQ_GEMM_GROUP_MAX && kGroupMax == NF4DQ_GEMM_GROUP_MAX, "group sizes");
constexpr uint32_t kLdsPerCu = 160 * 1024;
constexpr uint32_t kStreamStatic = 256 * 32 * 8 + 1024;        // pair table, q/127 table
constexpr uint32_t kStreamLdsCap = kLdsPerCu - kStreamStatic;  // dynamic part

// Workspace: [64 KiB of uint32 ticket counters][256 B: the error word + spare]
// [ksplit * M * N / 2 64-bit slab entries].  The header has a fixed size so that no
// call's partials ever overlay another call's counters (those must stay 0 between
// calls): N <= 2^18.  The error word (kErrWord, sticky) is set by a reducer whose
// poll gave up (nf4_gemm_check_workspace reads it).
constexpr uint32_t kErrWord = 16384;  // uint32 index in the workspace header (byte 64 KiB)
constexpr size_t kCounterBytes = 64 * 1024;
constexpr size_t kHeaderBytes = kCounterBytes + 256;
static_assert(kErrWord * 4u == kCounterBytes, "the error word follows the counters");

// How a 64-block's scale is made (a compile-time mode of the kernel families that have it):
//  * kScaleRef: the reference repository's, (a1[i] / 127) * a2[row group], statistics
//    repeating (wrap) -- nf4_gemm_ref and its kin;
//  * kScaleBnb: bitsandbytes nested, code2[a1[i]] * a2[i >> sh2] + offset (two roundings)
//    with i = (flat 64-block) >> sh, no wrap -- nf4_gemm_bnb;
//  * kScaleBnbSingle: bitsandbytes with fp32 statistics, a2[i] -- nf4_gemm_bnb_single.
constexpr int kScaleRef = 0, kScaleBnb = 1, kScaleBnbSingle = 2;

// One weight of a launch (host view).
struct HostMat {
    const uint8_t* packed;
    int64_t packed_len;
    const uint8_t* a1;
    int64_t nb;
    const float* a2;  // kScaleBnbSingle: the fp32 absmax (nb = n2 = its length, a1 unused)
    int64_t n2;
    void* y;
    int64_t N;
    // bitsandbytes modes (nf4_gemm_bnb*); the reference entries leave the defaults
    int mode = kScaleRef;
    const float* code2 = nullptr;   // 256 fp32 (device)
    const float* offset = nullptr;  // 1 fp32 (device); null = 0
    int sh = 0, sh2 = 0;            // log2(blocksize / 64), log2(blocksize2)
};

// No row's absmax bytes or nested scales wrap around inside the row (what the
// persistent kernel, the GEMV and the vector-scale forms assume).
inline bool no_wrap_in_row(const HostMat& h, int64_t K) {
    if (h.mode != kScaleRef) return true;  // a flat stream of statistics: nothing repeats
    const int64_t bpr = K / 64, groups = (bpr + 3) / 4;
    if (bpr == 0) return false;  // K = 0: no row to speak of, and no cfg that needs this runs
    return (h.nb % bpr == 0 || h.nb >= h.N * bpr) && (h.n2 % groups == 0 || h.n2 >= h.N * groups);
}
inline bool no_wrap_in_row(const HostMat* mats, int count, int64_t K) {
    for (int i = 0; i < count; ++i)
        if (!no_wrap_in_row(mats[i], K)) return false;
    return true;
}

// code2 tables a launch keeps in LDS beside its usual ones: one per weight in a grouped
// nested bitsandbytes launch of the register-resident kernel (nf4_gemm_bnb_grouped), else 0.
inline int group_tables(const HostMat* mats, int count) {
    return count > 1 && mats[0].mode == kScaleBnb ? count : 0;
}

// ---- launch geometry, per family ---------------------------------------------
struct StreamPlan {
    uint32_t cps, xstride, zero_off, red_off, lds;
};

inline StreamPlan stream_plan(int64_t M, int64_t K, const nf4_gemm_cfg& c) {
    const uint32_t chunks = (uint32_t)(K / kSChunkK);
    const uint32_t mt = (uint32_t)((M + 15) / 16);
    StreamPlan p{};
    p.cps = (chunks + (uint32_t)c.ksplit - 1) / (uint32_t)c.ksplit;
    p.xstride = p.cps * 512u + 16u;  // +16 B: consecutive rows start 4 banks apart
    p.zero_off = kLdsX + (uint32_t)M * p.xstride;
    p.red_off = kLdsX;
    const uint32_t xend = p.zero_off + 128u, rend = p.red_off + (uint32_t)c.waves * mt * 1024u;
    p.lds = xend > rend ? xend : rend;
    return p;
}

inline bool stream_fits(int64_t M, int64_t K, const nf4_gemm_cfg& c) {
    const StreamPlan p = stream_plan(M, K, c);
    const int64_t xr = kXR * ((M + 15) / 16);
    return p.lds <= kStreamLdsCap && M * (int64_t)p.cps * 32 <= xr * 64 * c.waves;
}

// Strip groups (cfg.strips 16-column strips each) over all weights: the streaming grid
// is one workgroup per (strip group, K slice).
inline uint32_t strip_groups(const HostMat* mats, int count, const nf4_gemm_cfg& c) {
    uint32_t sg = 0;
    for (int i = 0; i < count; ++i) sg += (uint32_t)(mats[i].N / (16 * c.strips));
    return sg;
}

// Dynamic LDS of the persistent kernel: x slice, zero block, two partial-sum
// sets, the held outputs (16-bit finished values; fp32 partials when K is split).
inline uint32_t persist_dyn_bytes(int64_t M, int64_t K, const nf4_gemm_cfg& c, uint32_t groups_per_wg) {
    const uint32_t ks = c.ksplit > 1 ? (uint32_t)c.ksplit : 1u;
    const uint32_t xstride = (uint32_t)(K / ks) * 2u + 16u;
    const uint32_t ob = ks > 1 ? 64u : 32u;  // bytes per held row of a strip
    const uint32_t out = (groups_per_wg * (uint32_t)c.strips * (uint32_t)M * ob + 15u) & ~15u;
    return kLdsX + (uint32_t)M * xstride + 128u + 2u * (uint32_t)c.waves * 1024u + out;
}

// The persistent grid: as many workgroups as fit the CUs at once, G / ksplit per K
// slice, each walking per_wg of the launch's sg strip groups.
struct PersistGrid {
    uint32_t G, per_wg, dyn, zero_off, red_off, out_off;
};

inline PersistGrid persist_grid(int64_t M, int64_t K, const nf4_gemm_cfg& c, uint32_t sg, int cus) {
    const uint32_t ks = (uint32_t)c.ksplit;
    const uint32_t base = persist_dyn_bytes(M, K, c, 1) + kStreamStatic;
    const uint32_t per_cu = kLdsPerCu / base > 0 ? kLdsPerCu / base : 1u;
    PersistGrid g{};
    g.G = (uint32_t)cus * per_cu;
    if (g.G > sg * ks) g.G = sg * ks;
    g.G = g.G / ks * ks;
    if (g.G < ks) g.G = ks;
    g.per_wg = (sg + g.G / ks - 1) / (g.G / ks);
    g.dyn = persist_dyn_bytes(M, K, c, g.per_wg);
    g.zero_off = kLdsX + (uint32_t)M * ((uint32_t)(K / kSChunkK) / ks * 512u + 16u);
    g.red_off = g.zero_off + 128u;
    g.out_off = g.red_off + 2u * (uint32_t)c.waves * 1024u;
    return g;
}

// LDS bytes of the shared-activation kernel: x slice (16 MT rows) + scale table + LUT.
inline uint32_t xs_lds_bytes(int64_t M, int kc, int waves) {
    const uint32_t mt = M > 16 ? 2u : 1u;
    return 16u * mt * ((uint32_t)kc * 256u + 16u) + 16u * (uint32_t)waves * 2u * (uint32_t)kc * 4u + 64u;
}

// Register-resident kernel: grid = ksplit x (strip groups of T strips); T from
// the CUs the launch can hold at once (one 16-wave workgroup per CU), at most 64
// (ticket flags) and within LDS.
// (128-deep chunks keep no table in the reference mode; the nested bnb mode's code2 table is
// static there too)
constexpr uint32_t xr_lds_static(int kpw, int mode = kScaleRef) {  // pair table + q/127 or code2, static in the kernel
    return kpw >= 2 ? 256u * 32u * 8u + 1024u : mode == kScaleBnb ? 64u + 1024u : 64u;
}
// (tables: group_tables -- each weight's code2 and, in 32 bytes after them, the offsets)
inline uint32_t xr_lds_dynamic(int64_t M, int waves, uint32_t T, int tables = 0) {
    const uint32_t mt = M > 16 ? 2u : 1u;
    const uint32_t r = waves == 8 ? 2u : 1u;  // strips per reduction group (kernel's R; depth is even)
    const uint32_t tab = tables > 0 ? (uint32_t)tables * 1024u + 32u : 0u;
    return 2u * r * (uint32_t)waves * mt * 1024u + 64u + 256u + T * mt * 1024u + tab;  // partials, codes, flags, held
}
inline uint32_t xr_lds_bytes(int64_t M, int waves, int kpw, uint32_t T, int mode = kScaleRef, int tables = 0) {
    return xr_lds_static(kpw, mode) + xr_lds_dynamic(M, waves, T, tables);
}

inline uint32_t xr_per_wg(int64_t M, int64_t strips, const nf4_gemm_cfg& c, int cus, int mode = kScaleRef,
                          int tables = 0) {
    const uint32_t wg_per_cu = c.waves == 16 || c.strips >= 2 ? 1u : 2u;  // the pair table leaves room for one
    uint32_t P = (uint32_t)cus * wg_per_cu / (uint32_t)c.ksplit;          // workgroups per K slice
    if (P < 1) P = 1;
    uint32_t T = (uint32_t)((strips + P - 1) / P);
    while (T > 1 && (T > 64 || xr_lds_bytes(M, c.waves, c.strips, T, mode, tables) > kLdsPerCu)) T = (T + 1) / 2;
    return T < 1 ? 1u : T;
}

// 128-deep kernel: the slice's scale table, kept in LDS (the vector-scale form) when
// it is small and absmax does not wrap inside a row of any weight.
inline uint32_t k128_scale_bytes(int64_t K, const nf4_gemm_cfg& c) {
    const uint32_t ks = (uint32_t)c.ksplit, nt = c.strips > 1 ? (uint32_t)c.strips : 1u;
    return 16u * nt * 2u * (((uint32_t)(K / kChunkK) + ks - 1) / ks) * 4u;
}
inline bool k128_vector_scales(uint32_t scale_bytes, bool no_wrap) { return no_wrap && scale_bytes <= 48u * 1024u; }

// GEMV: cfg.strips workgroups per CU (0 = 1), at most one row group (cfg.depth rows) per wave.
inline uint32_t gemv_grid(uint32_t row_groups, const nf4_gemm_cfg& c, int cus) {
    const uint32_t W = (uint32_t)c.waves, need = (row_groups + W - 1) / W;
    uint32_t G = (uint32_t)cus * (c.strips > 0 ? (uint32_t)c.strips : 1u);
    if (G > need) G = need;
    return G < 1 ? 1u : G;
}
// GEMV LDS: the x staging (2 K bytes) beside the 64 KiB pair table and the q/127 table.
inline uint32_t gemv_lds_bytes(int64_t K) { return (uint32_t)(K * 2); }

// Grid, block and dynamic LDS of one launch of cfg over `count` weights: what every
// launcher launches with (and the CPU check prints).
struct LaunchShape {
    uint32_t grid, block, dyn;
};

inline LaunchShape launch_shape(const nf4_gemm_cfg& c, int64_t M, int64_t K, const HostMat* mats, int count, int cus) {
    LaunchShape l{0, 64u * (uint32_t)c.waves, 0};
    const uint32_t ks = (uint32_t)c.ksplit;
    uint32_t rows = 0, cgs = 0;
    for (int i = 0; i < count; ++i) rows += (uint32_t)mats[i].N;
    switch (c.kernel) {
        case NF4DQ_GEMM_STREAM:
            l.grid = strip_groups(mats, count, c) * ks;
            l.dyn = stream_plan(M, K, c).lds;
            break;
        case NF4DQ_GEMM_PERSIST: {
            const PersistGrid g = persist_grid(M, K, c, strip_groups(mats, count, c), cus);
            l.grid = g.G;
            l.dyn = g.dyn;
            break;
        }
        case NF4DQ_GEMM_XS:  // one 16-column strip per wave; a weight's last group may be partial
            for (int i = 0; i < count; ++i) cgs += ((uint32_t)mats[i].N + 16u * c.waves - 1u) / (16u * c.waves);
            l.grid = cgs * ks;
            l.dyn = xs_lds_bytes(M, c.depth, c.waves);
            break;
        case NF4DQ_GEMM_XR: {
            const int tables = count > 0 ? group_tables(mats, count) : 0;
            const uint32_t per_wg = xr_per_wg(M, rows / 16u, c, cus, count > 0 ? mats[0].mode : kScaleRef, tables);
            l.grid = (rows / 16u + per_wg - 1) / per_wg * ks;
            l.dyn = xr_lds_dynamic(M, c.waves, per_wg, tables);
            break;
        }
        case NF4DQ_GEMM_K128: {
            const uint32_t nt = c.strips > 1 ? (uint32_t)c.strips : 1u, scl = k128_scale_bytes(K, c);
            for (int i = 0; i < count; ++i) cgs += (uint32_t)mats[i].N / (16u * nt);
            l.grid = cgs * ks;
            l.dyn = k128_vector_scales(scl, no_wrap_in_row(mats, count, K)) ? scl : 0u;
            break;
        }
        case NF4DQ_GEMM_GEMV:
            l.grid = gemv_grid(rows / (uint32_t)c.depth, c, cus);
            l.dyn = gemv_lds_bytes(K);
            break;
    }
    return l;
}

// ---- cfg validity ----------------------------------------------------------
// (N: one weight's columns.)
inline bool valid_gemm_cfg(const nf4_gemm_cfg& c, int64_t M, int64_t N, int64_t K) {
    if (c.kernel == NF4DQ_GEMM_PERSIST) {
        if (K % kSChunkK || M > 16) return false;
        if (c.waves != 4 && c.waves != 8 && c.waves != 16) return false;
        if (c.depth != 2 && c.depth != 4) return false;
        if (c.strips != 1 && c.strips != 2 && c.strips != 4) return false;
        if (c.waves % c.strips || N % (16 * c.strips) || c.ksplit < 1 || c.ksplit > 16) return false;
        const int64_t chunks = K / kSChunkK, parts = c.waves / c.strips;
        if (chunks % c.ksplit) return false;
        const int64_t cps = chunks / c.ksplit;  // chunks per K slice
        if (cps % parts || (cps / parts) % c.depth) return false;
        if (M * cps * 32 > (int64_t)kXR * 64 * c.waves) return false;
        return persist_dyn_bytes(M, K, c, 1) + kStreamStatic <= kLdsPerCu;
    }
    if (c.kernel == NF4DQ_GEMM_STREAM) {
        if (K % kSChunkK) return false;
        if (c.waves != 4 && c.waves != 8 && c.waves != 16) return false;
        if (c.depth != 2 && c.depth != 4 && c.depth != 8) return false;
        if (c.waves == 16 && (M > 16 || c.depth == 8)) return false;
        if (c.strips != 1 && c.strips != 2 && c.strips != 4) return false;
        if (c.waves % c.strips || N % (16 * c.strips)) return false;
        if (c.ksplit < 1 || c.ksplit > K / kSChunkK) return false;
        return stream_fits(M, K, c);
    }
    if (c.kernel == NF4DQ_GEMM_XR) {
        if (c.waves != 8 && c.waves != 16) return false;
        if (c.depth != 2 && c.depth != 4) return false;
        if (c.strips != 1 && c.strips != 2 && c.strips != 4) return false;  // 128-deep chunks per wave
        if (c.strips == 4 && (c.waves != 8 || K % 512)) return false;          // two 256-deep chunks per wave
        if (c.strips == 4 && c.depth == 4 && M > 16) return false;             // 64 x VGPRs + a 4-deep ring spill
        // x + a 4-deep ring spill within 16 waves' 128 registers (8 waves: 256)
        if (M > 16 && c.strips == 2 && c.depth == 4 && c.waves == 16) return false;
        if (c.strips >= 2 && K % 256) return false;                 // 256-deep chunks
        const int64_t chunks = K / kChunkK, per = (int64_t)c.waves * c.strips;
        return c.ksplit >= 1 && c.ksplit == (chunks + per - 1) / per && c.ksplit <= 1024;
    }
    // NF4DQ_GEMM_SK (the balanced stream-K kernel, rounds 4-5) was never the library's
    // choice -- 13.1-15.1 vs 10.6 us on 14336x4096 at M = 1,
    // profiles/r04/gemm/sk_depth_vs_persist.jsonl -- and was removed in round 6: its
    // number is rejected like any unknown kernel (git history holds the source)
    if (c.kernel == NF4DQ_GEMM_GEMV) {
        if (M != 1 || K % 2048 || K > 16384 || c.ksplit != 1) return false;
        if (c.waves != 8 && c.waves != 16) return false;
        if (c.depth != 1 && c.depth != 2 && c.depth != 4) return false;
        return c.strips >= 0 && c.strips <= 2 && N % c.depth == 0;
    }
    if (c.kernel == NF4DQ_GEMM_XS) {
        if (c.waves != 4 && c.waves != 8) return false;
        if (c.depth != 2 && c.depth != 4 && c.depth != 8) return false;
        if (c.strips != 0 && c.strips != 1) return false;
        const int64_t chunks = K / kChunkK;
        return c.ksplit == (chunks + c.depth - 1) / c.depth && c.ksplit <= 256;
    }
    if (c.kernel != NF4DQ_GEMM_K128) return false;
    if (c.waves != 4 && c.waves != 8) return false;
    if (c.strips != 0 && c.strips != 1 && c.strips != 2 && c.strips != 4) return false;  // strips per wave
    if (M > 16 ? (c.depth != 1 && c.depth != 2) : (c.depth != 1 && c.depth != 2 && c.depth != 4)) return false;
    return c.ksplit >= 1 && c.ksplit <= K / kChunkK && c.ksplit <= 64;
}

// An empty weight (N == 0) of a group: the kernels that number column groups per weight
// take it (it owns none); it cannot own strip groups or rows.
inline bool takes_empty_weight(int kernel) {
    return kernel == NF4DQ_GEMM_K128 || kernel == NF4DQ_GEMM_XS || kernel == NF4DQ_GEMM_XR;
}

// Whether a valid cfg can run on these weights: NF4DQ_OK, or the code a caller who named
// the cfg gets (the library's own choice moves on to the next one instead, library_choice).
// The persistent kernel and the GEMV need absmax not to wrap inside a row; the
// persistent kernel also one ticket per strip group within the header and its held
// outputs within the LDS at the grid `cus` gives.
inline int cfg_runs(const nf4_gemm_cfg& c, int64_t M, int64_t K, const HostMat* mats, int count, int cus) {
    if (c.kernel != NF4DQ_GEMM_PERSIST && c.kernel != NF4DQ_GEMM_GEMV) return NF4DQ_OK;
    if (!no_wrap_in_row(mats, count, K)) return NF4DQ_ERR_ARG;
    if (c.kernel == NF4DQ_GEMM_GEMV) return NF4DQ_OK;
    const uint32_t sg = strip_groups(mats, count, c);
    if (c.ksplit > 1 && sg * 4u > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    return persist_grid(M, K, c, sg, cus).dyn + kStreamStatic > kLdsPerCu ? NF4DQ_ERR_TOO_LARGE : NF4DQ_OK;
}

// ---- the library's choice --------------------------------------------------
// Defaults, from tools/sweep_gemm.py on MI355X (Llama-3-8B shapes and the grouped
// q/k/v and gate/up column totals, M = 1..32; re-checked in round 4,
// profiles/r04/gemm/sweep_gemm_m1_12.jsonl, sweep_gemm_m16_32.jsonl: the default is
// the fastest or within 2 % of it except where noted below).  N = all columns of the
// launch (a grouped launch passes the sum).
//  * M = 1, N <= 4096, K % 2048 == 0: the decode GEMV (round 6, gemv_choice below).
//  * M <= 8: the persistent kernel whenever x[M][K] fits its LDS (the streaming
//    kernel if absmax wraps inside a row), strips by width.
//  * 8 < M <= 16: the persistent kernel with K slices; the register-resident
//    kernel for N <= 1024.
//  * 16 < M <= 32: the register-resident kernel (two K slices at K = 4096; 16 waves
//    and no slices for the widest launches at M <= 24); the 128-deep and
//    shared-activation kernels where K % 256 != 0 or N < 1024.
inline nf4_gemm_cfg k128_cfg(int64_t M, int64_t N, int64_t K, int waves, int depth, int ksplit, int strips) {
    nf4_gemm_cfg c{NF4DQ_GEMM_K128, waves, depth, ksplit, strips};
    if (M > 16 && c.depth > 2) c.depth = 2;
    while (c.strips > 1 && N % (16 * c.strips)) c.strips /= 2;
    if (c.ksplit > K / kChunkK) c.ksplit = (int)(K / kChunkK);
    if (c.ksplit < 1) c.ksplit = 1;
    return c;
}

// The 128-deep decomposition for a shape no other family takes: what nonpersist_cfg ends
// with (after its streaming, register-resident and shared-activation choices), and what the
// bnb plan substitutes for a family without the mode (bnb_choice).
inline nf4_gemm_cfg k128_tail_cfg(int64_t M, int64_t N, int64_t K) {
    if (M <= 16) {
        if (K >= 8192) return k128_cfg(M, N, K, 8, 1, 2, 2);
        if (N < 4096) return k128_cfg(M, N, K, 4, 2, 4, 1);
        return k128_cfg(M, N, K, 8, 2, 1, 1);
    }
    if (K >= 8192) return k128_cfg(M, N, K, 8, 1, 4, 4);
    if (N < 4096) return k128_cfg(M, N, K, 4, 2, 4, 1);
    if (N <= 4096) return k128_cfg(M, N, K, 8, 1, 2, 2);
    if (N < 8192) return k128_cfg(M, N, K, 4, 1, 4, 2);
    return k128_cfg(M, N, K, N >= 16384 ? 4 : 8, 1, 1, 4);
}

// The library's choice when the persistent kernel is not used (or cannot run:
// absmax wrapping inside a row, held outputs beyond its LDS).
inline nf4_gemm_cfg nonpersist_cfg(int64_t M, int64_t N, int64_t K) {
    const bool k256 = K % kSChunkK == 0;
    if (k256 && M <= 8) {
        nf4_gemm_cfg c{NF4DQ_GEMM_STREAM, 8, 2, 1, 1};
        if (M > 4) c = nf4_gemm_cfg{NF4DQ_GEMM_STREAM, 8, 2, 4, 4};
        else if (M > 1) c = nf4_gemm_cfg{NF4DQ_GEMM_STREAM, 8, 2, 2, 2};
        while (c.strips > 1 && N % (16 * c.strips)) c.strips /= 2;
        if (c.ksplit > K / kSChunkK) c.ksplit = (int)(K / kSChunkK);
        while (c.ksplit < K / kSChunkK && !stream_fits(M, K, c)) ++c.ksplit;
        if (valid_gemm_cfg(c, M, N, K)) return c;
        return k128_cfg(M, N, K, 8, 2, 1, 1);
    }
    if (M <= 16) {
        if (k256 && K < 8192 && N > 4096) {
            nf4_gemm_cfg c{NF4DQ_GEMM_STREAM, 8, 2, 2, 4};
            while (c.strips > 1 && N % (16 * c.strips)) c.strips /= 2;
            while (c.ksplit < K / kSChunkK && !stream_fits(M, K, c)) ++c.ksplit;
            if (valid_gemm_cfg(c, M, N, K)) return c;
        }
        return k128_tail_cfg(M, N, K);
    }
    if (K % kSChunkK == 0 && N >= 1024) {
        // the register-resident kernel with pair-table lookups, 8 waves x 256-deep
        // chunks: per launch at M = 32 (profiles/r02/sweep_gemm_xr.jsonl) 20.4 vs 21.7 us
        // on 14336x4096, 11.9 vs 12.3 on 4096^2, 23.5 vs 24.6 on 4096x14336, 13.8 vs 14.2
        // on grouped q/k/v (6144), 31.4 vs 37.2 on grouped gate/up (28672); from N = 1024
        // since round 4 (7.7 vs 8.6-9.0 us at M = 24 / 32, profiles/r04/gemm/sweep_gemm_m16_32.jsonl)
        if (M <= 24 && N >= 24576) {
            // the widest launches (grouped gate/up) at M <= 24: 16 waves span K = 4096,
            // no split-K hand-off: 26.0 vs 27.6 us (profiles/r04/gemm/xr_no_handoff_m24_m32.jsonl)
            const nf4_gemm_cfg w{NF4DQ_GEMM_XR, 16, 2, (int)((K / kChunkK + 31) / 32), 2};
            if (valid_gemm_cfg(w, M, N, K)) return w;
        }
        const nf4_gemm_cfg c{NF4DQ_GEMM_XR, 8, 2, (int)((K / kChunkK + 15) / 16), 2};
        if (valid_gemm_cfg(c, M, N, K)) return c;
    }
    if (K >= 8192) return k128_tail_cfg(M, N, K);
    if (N >= 6144) {
        // wide launches (gate/up, grouped q/k/v): the shared-activation kernel,
        // 10-13 % faster than the 128-deep one at M = 24 / 32 (profiles/r02/sweep_gemm_xs.jsonl)
        const int waves = N >= 12288 ? 8 : 4, kc = N >= 12288 ? 8 : 4;
        const nf4_gemm_cfg c{NF4DQ_GEMM_XS, waves, kc, (int)((K / kChunkK + kc - 1) / kc), 1};
        if (valid_gemm_cfg(c, M, N, K)) return c;
    }
    return k128_tail_cfg(M, N, K);
}

inline nf4_gemm_cfg default_gemm_cfg(int64_t M, int64_t N, int64_t K) {
    if (K % kSChunkK == 0 && M <= 8) {
        const int strips = N >= 16384 ? 1 : N >= 8192 ? 4 : N > 4096 ? 2 : 1;
        const nf4_gemm_cfg c{NF4DQ_GEMM_PERSIST, 8, 2, 1, strips};
        if (valid_gemm_cfg(c, M, N, K)) return c;
    } else if (K % kSChunkK == 0 && M <= 16) {
        if (N <= 1024) {
            // too few strips to cover the CUs with slices of the persistent kernel: the
            // register-resident kernel, 6.6 vs 7.7 us on 1024x4096 at M = 12
            // (profiles/r04/gemm/sweep_gemm_m1_12.jsonl)
            const nf4_gemm_cfg c{NF4DQ_GEMM_XR, 8, 2, (int)((K / kChunkK + 15) / 16), 2};
            if (valid_gemm_cfg(c, M, N, K)) return c;
        }
        // persistent with K slices: the fewest slices whose x fits, while the
        // (strip group, slice) pairs still cover every CU
        for (int strips = 2; strips <= 4; strips *= 2)
            for (int ks = 2; ks <= 16; ++ks) {
                const nf4_gemm_cfg c{NF4DQ_GEMM_PERSIST, 8, 2, ks, strips};
                if (N / (16 * strips) * ks >= 256 && valid_gemm_cfg(c, M, N, K)) return c;
            }
    }
    return nonpersist_cfg(M, N, K);
}

// M = 1: the decode GEMV (nf4_gemm_launch_gemv.hip) where it beats the persistent kernel:
// up to 4096 columns (profiles/r06/gemm/s29_gemv_ab.jsonl, s30_gemv_ab.jsonl, one box each:
// 4096^2 5.77-5.99 vs 6.33 us, 4096 x 14336 10.25-10.61 vs 11.16-11.62); wider launches
// stay persistent (14336 x 4096: 11.6 vs 10.5; grouped q/k/v 7.6 vs 7.3).  N = all columns
// of the launch.
inline bool gemv_choice(int64_t M, int64_t N, int64_t K) { return M == 1 && K % 2048 == 0 && K <= 16384 && N <= 4096; }

// What a call runs.  `first` is the cfg the entry validates and sizes the workspace by:
// the caller's, or default_gemm_cfg of the column total.  `cfg` is the one launch that
// runs -- unless `per_weight`: the library's persistent choice cannot run here
// (cfg_runs), so every weight gets a launch of its own with nonpersist_cfg of its own N.
struct Choice {
    nf4_gemm_cfg first, cfg;
    bool per_weight;
};

inline Choice library_choice(int64_t M, int64_t K, const HostMat* mats, int count, int cus) {
    int64_t ntot = 0;
    bool empty = false;
    for (int i = 0; i < count; ++i) {
        ntot += mats[i].N;
        empty = empty || mats[i].N == 0;
    }
    Choice ch{default_gemm_cfg(M, ntot, K), {}, false};
    ch.cfg = ch.first;
    const nf4_gemm_cfg gv{NF4DQ_GEMM_GEMV, 16, 1, 1, 0};
    if (gemv_choice(M, ntot, K) && !empty && cfg_runs(gv, M, K, mats, count, cus) == NF4DQ_OK) ch.cfg = gv;
    else if (ch.first.kernel == NF4DQ_GEMM_PERSIST && cfg_runs(ch.first, M, K, mats, count, cus) != NF4DQ_OK)
        ch.per_weight = true;
    return ch;
}

// The cfg of the launch that covers weight m: the one launch's, or the weight's own.
inline nf4_gemm_cfg launch_cfg(const Choice& ch, int64_t M, int64_t K, const HostMat& m) {
    return ch.per_weight ? nonpersist_cfg(M, m.N, K) : ch.cfg;
}

// The caller's cfg: it never falls back (the entry answers cfg_runs' code instead);
// kernel == 0 with other fields set takes only the kernel number from the default.
inline Choice explicit_choice(nf4_gemm_cfg c, int64_t M, int64_t ntot, int64_t K) {
    if (c.kernel == 0) c.kernel = default_gemm_cfg(M, ntot, K).kernel;
    return Choice{c, c, false};
}

// ---- workspace ---------------------------------------------------------------
// Bytes a launch of cfg over ntot columns needs: the header and the split-K slab
// (an 8-byte entry per 2 columns), nothing without K slices.
inline size_t slab_need(int64_t M, int64_t ntot, const nf4_gemm_cfg& c) {
    return c.ksplit > 1 ? kHeaderBytes + (size_t)c.ksplit * (size_t)M * (size_t)ntot * 4u : 0;
}
// ... and nothing for a shape the entries reject.
inline size_t workspace_need(int64_t M, int64_t ntot, int64_t K, const nf4_gemm_cfg& c) {
    return M <= 0 || ntot <= 0 || K <= 0 || ntot % 64 || K % kChunkK ? 0 : slab_need(M, ntot, c);
}

// What the size entries answer without a cfg: the library's choice, or the next one if
// that cannot run (a caller cannot know) -- the larger need.
inline size_t library_workspace(int64_t M, int64_t N, int64_t K) {
    const size_t a = workspace_need(M, N, K, default_gemm_cfg(M, N, K));
    const size_t b = workspace_need(M, N, K, nonpersist_cfg(M, N, K));
    return a > b ? a : b;
}

// ---- bitsandbytes semantics (nf4_gemm_bnb / nf4_gemm_bnb_single) ---------------
// The families that have the bnb scale modes: the ones the library chooses for model
// shapes (decode GEMV, persistent, register-resident) and the 128-deep kernel, which
// takes every accepted shape.  The streaming and shared-activation kernels do not.
inline bool bnb_has_mode(int kernel) {
    return kernel == NF4DQ_GEMM_K128 || kernel == NF4DQ_GEMM_XR || kernel == NF4DQ_GEMM_PERSIST ||
           kernel == NF4DQ_GEMM_GEMV;
}
// Statistics blocks above 64 (sh > 0) go through the 128-deep kernel alone: the others'
// statistic loads assume one byte per 64-block.
inline bool bnb_cfg_ok(const nf4_gemm_cfg& c, const HostMat& h) {
    return bnb_has_mode(c.kernel) && (h.sh == 0 || c.kernel == NF4DQ_GEMM_K128);
}

// What a bnb call runs without a cfg: the reference plan's launch for (M, N, K) -- same
// family, same decomposition -- or the 128-deep substitute where that family lacks the
// mode or the weight's blocksize.  One weight, one launch.
inline Choice bnb_choice(int64_t M, int64_t K, const HostMat& h, int cus) {
    const Choice ref = library_choice(M, K, &h, 1, cus);
    nf4_gemm_cfg c = launch_cfg(ref, M, K, h);
    if (!bnb_cfg_ok(c, h) || !valid_gemm_cfg(c, M, h.N, K)) c = k128_tail_cfg(M, h.N, K);
    return Choice{c, c, false};
}

// What nf4_gemm_bnb_workspace_bytes answers without a cfg.  The blocksize and the CU count
// are not known there: the largest need of what bnb_choice can come to.
inline size_t bnb_library_workspace(int64_t M, int64_t N, int64_t K) {
    size_t w = workspace_need(M, N, K, k128_tail_cfg(M, N, K));
    const nf4_gemm_cfg cs[2] = {default_gemm_cfg(M, N, K), nonpersist_cfg(M, N, K)};
    for (const nf4_gemm_cfg& c : cs) {
        const size_t wc = bnb_has_mode(c.kernel) ? workspace_need(M, N, K, c) : 0;
        w = wc > w ? wc : w;
    }
    return w;
}

// ---- grouped bitsandbytes semantics (nf4_gemm_bnb_grouped) -----------------------
// The families with the grouped form of the bnb modes: the ones the reference grouped plan
// chooses for model shapes (persistent, register-resident) and the 128-deep catch-all.  The
// decode GEMV, the streaming and the shared-activation kernels do not have it.
inline bool bnb_grouped_has_mode(int kernel) {
    return kernel == NF4DQ_GEMM_K128 || kernel == NF4DQ_GEMM_XR || kernel == NF4DQ_GEMM_PERSIST;
}
// A cfg can take the group: a family with the grouped mode; above blocksize 64 (sh > 0 in
// any weight) the 128-deep kernel alone.
inline bool bnb_grouped_cfg_ok(const nf4_gemm_cfg& c, const HostMat* mats, int count) {
    if (!bnb_grouped_has_mode(c.kernel)) return false;
    for (int i = 0; i < count; ++i)
        if (mats[i].sh != 0 && c.kernel != NF4DQ_GEMM_K128) return false;
    return true;
}

// What a grouped bnb call runs without a cfg: ONE launch over the column total -- the
// reference grouped plan's (same family, same decomposition) where that family has the
// grouped mode and every weight has blocksize 64; the persistent kernel where the reference
// plan picks the decode GEMV (its choice there before the GEMV existed: default_gemm_cfg);
// the 128-deep substitute (k128_tail_cfg of the column total) where it picks the streaming
// or shared-activation kernel or a weight has a larger blocksize.  Only where the persistent
// cfg cannot run (cfg_runs) every weight gets bnb_choice's launch of its own (per_weight).
inline Choice bnb_grouped_choice(int64_t M, int64_t K, const HostMat* mats, int count, int cus) {
    int64_t ntot = 0;
    bool empty = false;
    for (int i = 0; i < count; ++i) {
        ntot += mats[i].N;
        empty = empty || mats[i].N == 0;
    }
    const Choice ref = library_choice(M, K, mats, count, cus);
    nf4_gemm_cfg c = ref.cfg.kernel == NF4DQ_GEMM_GEMV ? ref.first : ref.cfg;
    if (ref.cfg.kernel == NF4DQ_GEMM_GEMV && c.kernel != NF4DQ_GEMM_PERSIST) {
        // K / 256 chunks do not split over 8 waves' rings (K = 2048, 14336): 4 waves' do
        const nf4_gemm_cfg p4{NF4DQ_GEMM_PERSIST, 4, 2, 1, 1};
        if (valid_gemm_cfg(p4, M, 64, K)) c = p4;
    }
    bool ok = bnb_grouped_cfg_ok(c, mats, count) && !(empty && !takes_empty_weight(c.kernel));
    for (int i = 0; i < count && ok; ++i) ok = mats[i].N == 0 || valid_gemm_cfg(c, M, mats[i].N, K);
    if (!ok) c = k128_tail_cfg(M, ntot, K);
    Choice ch{c, c, false};
    ch.per_weight = c.kernel == NF4DQ_GEMM_PERSIST && cfg_runs(c, M, K, mats, count, cus) != NF4DQ_OK;
    return ch;
}

// What nf4_gemm_bnb_grouped_workspace_bytes answers: a named cfg's need over the column
// total; without one (the CU count is not known here) the largest need of what
// bnb_grouped_choice can come to, the per-weight fallback's launches included.
template <class Mat>
inline size_t bnb_grouped_workspace(int64_t M, int64_t K, const Mat* mats, int count, const nf4_gemm_cfg* cfgp) {
    if (count <= 0 || count > kGroupMax || !mats || M <= 0 || K <= 0 || K % kChunkK) return 0;
    int64_t ntot = 0;
    for (int i = 0; i < count; ++i) {
        if (mats[i].N < 0 || mats[i].N % 64) return 0;
        ntot += mats[i].N;
    }
    if (ntot <= 0) return 0;
    if (cfgp) {
        nf4_gemm_cfg cfg = *cfgp;
        if (cfg.kernel == 0) cfg.kernel = default_gemm_cfg(M, ntot, K).kernel;
        return workspace_need(M, ntot, K, cfg);
    }
    size_t w = workspace_need(M, ntot, K, k128_tail_cfg(M, ntot, K));
    const nf4_gemm_cfg d = default_gemm_cfg(M, ntot, K);
    const size_t wd = bnb_grouped_has_mode(d.kernel) ? workspace_need(M, ntot, K, d) : 0;
    w = wd > w ? wd : w;
    for (int i = 0; i < count; ++i) {
        const size_t wi = bnb_library_workspace(M, mats[i].N, K);
        w = wi > w ? wi : w;
    }
    return w;
}

// Grouped: the cfg's need over the column total; the library's persistent choice may
// fall back to per-weight launches, so the largest of their needs as well.
template <class Mat>
inline size_t grouped_workspace(int64_t M, int64_t K, const Mat* mats, int count, const nf4_gemm_cfg* cfgp) {
    if (count <= 0 || !mats || M <= 0 || K <= 0 || K % kChunkK) return 0;
    int64_t ntot = 0;
    for (int i = 0; i < count; ++i) ntot += mats[i].N;
    if (ntot <= 0) return 0;
    nf4_gemm_cfg cfg = cfgp ? *cfgp : default_gemm_cfg(M, ntot, K);
    if (cfg.kernel == 0) cfg.kernel = default_gemm_cfg(M, ntot, K).kernel;
    size_t w = slab_need(M, ntot, cfg);  // (no shape guard on the column total here, as ever)
    if (cfgp || cfg.kernel != NF4DQ_GEMM_PERSIST) return w;
    for (int i = 0; i < count; ++i) {
        const size_t wi = workspace_need(M, mats[i].N, K, nonpersist_cfg(M, mats[i].N, K));
        w = wi > w ? wi : w;
    }
    return w;
}

}  // namespace nf4gemm
