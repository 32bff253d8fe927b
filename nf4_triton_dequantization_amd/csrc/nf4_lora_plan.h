// nf4_lora_plan.h -- the host-side plan of the fused adapter launch (nf4_lora_add:
// y_i = base_i + scale_i * B_i (A_i x) for up to NF4DQ_LORA_GROUP_MAX adapters over one x), plain
// C++17 (no HIP): argument validation with the status codes, cfg validity, the library's choice,
// the launch geometry and the LDS bytes.  Pure arithmetic, shared by the launcher (nf4_lora.hip)
// and a CPU check (tests/plan/lora_plan_check.cpp).  The rules, the geometry and the default-cfg
// rule are written over the fields nf4_lora_mat and nf4_lora_stack share (A, B, base, y, N, r)
// and a `slots` multiplier, so that the routed launch's plan (nf4_lora_routed_plan.h) adds its
// own rules to these and repeats none.
//
// Anatomy the numbers describe: the grid is (adapter, tile of tile_n columns), flattened, adapter
// i owning the blocks [tile0[i], tile0[i + 1]).  A workgroup of `waves` waves forms its adapter's
// whole t = rn(x A^T) in LDS -- row blocks of 16 * mb rows, the K / 32 chunks split into `waves`
// contiguous ranges, the waves' fp32 partials summed in wave order -- as [m_pad][ts] 16-bit values,
// zero beyond r up to the MFMA depth of 32; then wave w takes the 16-column strips w, w + waves, ..
// of the tile.  mb and rt (r tiles of 16, a power of two covering the group's largest r) choose the
// kernel instantiation.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/nf4_dequant.h"

namespace nf4lora {

constexpr uint32_t kLdsPerCu = 160 * 1024;
constexpr int64_t kMaxDim = int64_t(1) << 22;  // K and N: every element index fits 32 bits
constexpr uint32_t kMaxWaves = 4;
constexpr uint32_t kPartPad = 4;  // floats between rows of a wave's partials: the four lane groups of a store land 16 banks apart

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline bool valid_cfg(const nf4_lora_cfg& c) {
    const bool tile = c.tile_n == 16 || c.tile_n == 32 || c.tile_n == 64 || c.tile_n == 128 || c.tile_n == 256;
    return tile && (c.waves == 1 || c.waves == 2 || c.waves == 4);
}

// The library's choice.  Every workgroup repeats the shrink, so the tile width trades redundancy
// against parallelism in the expand: the narrowest of 64 / 128 / 256 columns (one strip per wave
// at least) whose tiles, `slots` times over, fit the CUs in one round, 256 when none does.
inline nf4_lora_cfg default_cfg(int64_t n_sum, int cus, int64_t slots = 1) {
    nf4_lora_cfg c{256, (int32_t)kMaxWaves};
    for (int32_t t : {64, 128, 256}) {
        if (slots * ((n_sum + t - 1) / t) <= (int64_t)(cus > 0 ? cus : 1)) { c.tile_n = t; break; }
    }
    return c;
}

struct LoraPlan {
    uint32_t grid, block, dyn;      // workgroups, threads, dynamic LDS bytes
    uint32_t tile_n, waves;
    uint32_t mb, rt;                // row tiles per row block (1 | 2), r tiles of the instantiation (1 | 2 | 4 | 8)
    uint32_t row_blocks, m_pad;     // row blocks of 16 * mb rows; rows of t in LDS
    uint32_t ts;                    // elements between rows of t: the largest r padded to 32, + 8
    uint32_t t_bytes, part_bytes;   // t, then the waves' fp32 partials of one row block, rows of 16 * rt + kPartPad floats
    uint32_t tile0[NF4DQ_LORA_GROUP_MAX + 1];
};

// Geometry of a validated call, over nf4_lora_mat or nf4_lora_stack; every matrix owns `slots`
// times its column tiles.
template <class Mat>
inline LoraPlan plan(const nf4_lora_cfg& c, int64_t M, const Mat* mats, int32_t count, uint32_t slots = 1) {
    LoraPlan p{};
    p.tile_n = (uint32_t)c.tile_n;
    p.waves = (uint32_t)c.waves;
    p.block = 64u * p.waves;
    int32_t r_max = 8;
    uint32_t at = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (mats[i].r > r_max) r_max = mats[i].r;
        p.tile0[i] = at;
        at += slots * (uint32_t)((mats[i].N + c.tile_n - 1) / c.tile_n);
    }
    for (int32_t i = count; i <= NF4DQ_LORA_GROUP_MAX; ++i) p.tile0[i] = at;
    p.grid = at;
    const uint32_t rtiles = ((uint32_t)r_max + 15u) / 16u;
    p.rt = rtiles <= 1 ? 1 : rtiles <= 2 ? 2 : rtiles <= 4 ? 4 : 8;
    p.mb = M <= 16 ? 1 : 2;
    p.row_blocks = ((uint32_t)M + 16u * p.mb - 1) / (16u * p.mb);
    p.m_pad = p.row_blocks * 16u * p.mb;
    p.ts = (((uint32_t)r_max + 31u) & ~31u) + 8u;
    p.t_bytes = p.m_pad * p.ts * 2u;
    p.part_bytes = p.waves * 16u * p.mb * (16u * p.rt + kPartPad) * 4u;
    p.dyn = p.t_bytes + p.part_bytes;
    return p;
}

// What a launch adds to the shared rules; each answers true where a rule of its class is broken.
// nf4_lora_add adds none.
struct NoOwnRules {
    bool call_arg() const { return false; }
    bool call_shape() const { return false; }
    bool arg(const nf4_lora_mat&) const { return false; }
    bool shape(const nf4_lora_mat&) const { return false; }
    bool too_large(const nf4_lora_mat&) const { return false; }
};

// The rules of a call, over nf4_lora_mat or nf4_lora_stack: NF4DQ_OK or the status code.  Every
// NF4DQ_ERR_ARG rule comes before every NF4DQ_ERR_SHAPE rule, the size limits last; `own` rules
// answer with their class.  Needs nothing of the device.
template <class Mat, class Own>
inline int validate_mats(const void* x, int64_t M, int64_t K, const Mat* mats, int32_t count, int32_t dtype,
                         const nf4_lora_cfg* cfg, const Own& own) {
    if (!x || !mats || own.call_arg()) return NF4DQ_ERR_ARG;  // routed: a null adapter_ids, adapters outside 1..64
    if (dtype != NF4DQ_F16 && dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (count < 1 || count > NF4DQ_LORA_GROUP_MAX) return NF4DQ_ERR_ARG;
    for (int32_t i = 0; i < count; ++i) {
        const Mat& m = mats[i];
        if (!m.A || !m.B || !m.y || own.arg(m)) return NF4DQ_ERR_ARG;  // routed: a null scale
        if (m.r < 8 || m.r > NF4DQ_LORA_MAX_R) return NF4DQ_ERR_ARG;
    }
    if (cfg && !valid_cfg(*cfg)) return NF4DQ_ERR_ARG;
    if (M < 1 || M > NF4DQ_LORA_MAX_M || K < 32 || K % 32) return NF4DQ_ERR_SHAPE;
    if (!aligned16(x) || own.call_shape()) return NF4DQ_ERR_SHAPE;  // routed: ids not 4-byte aligned
    for (int32_t i = 0; i < count; ++i) {
        const Mat& m = mats[i];
        if (m.N < 16 || m.N % 16 || m.r % 8) return NF4DQ_ERR_SHAPE;
        if (!aligned16(m.A) || !aligned16(m.B) || !aligned16(m.base) || !aligned16(m.y)) return NF4DQ_ERR_SHAPE;
        if (own.shape(m)) return NF4DQ_ERR_SHAPE;  // routed: scale not 4-byte aligned, a stride no multiple of 8 or below one adapter
    }
    if (K > kMaxDim) return NF4DQ_ERR_TOO_LARGE;
    for (int32_t i = 0; i < count; ++i)
        if (mats[i].N > kMaxDim || own.too_large(mats[i])) return NF4DQ_ERR_TOO_LARGE;  // routed: a stride above kMaxStride
    return NF4DQ_OK;
}

// What runs for a call that validated with `rc`: NF4DQ_OK and *out, or rc.  A cfg the caller
// names never falls back; `cus` matters only without one.  dyn(cfg): the plan's LDS bytes.
template <class Mat, class Dyn>
inline int choose_cfg(int rc, const nf4_lora_cfg* named, const Mat* mats, int32_t count, int cus, int64_t slots, Dyn dyn,
                      nf4_lora_cfg* out) {
    if (rc != NF4DQ_OK) return rc;
    int64_t n_sum = 0;
    for (int32_t i = 0; i < count; ++i) n_sum += mats[i].N;
    const nf4_lora_cfg c = named ? *named : default_cfg(n_sum, cus, slots);
    if (dyn(c) > kLdsPerCu) return NF4DQ_ERR_TOO_LARGE;  // unreachable within the limits above
    *out = c;
    return NF4DQ_OK;
}

struct LoraCall {
    const void* x;
    int64_t M, K;
    const nf4_lora_mat* mats;
    int32_t count;
    int32_t dtype;
    const nf4_lora_cfg* cfg;
};

// Validates a call: NF4DQ_OK or the status code.
inline int validate(const LoraCall& a) { return validate_mats(a.x, a.M, a.K, a.mats, a.count, a.dtype, a.cfg, NoOwnRules{}); }

// Validates a call and answers what runs: NF4DQ_OK and *out, or validate's status code.
inline int check(const LoraCall& a, int cus, nf4_lora_cfg* out) {
    return choose_cfg(validate(a), a.cfg, a.mats, a.count, cus, 1,
                      [&](const nf4_lora_cfg& c) { return plan(c, a.M, a.mats, a.count).dyn; }, out);
}

}  // namespace nf4lora
