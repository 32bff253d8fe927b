// nf4_lora_routed_plan.h -- the host-side plan of the routed adapter launch (nf4_lora_add_routed:
// y_i[m] = base_i[m] + scale_i[a] * B_i[a] (A_i[a] x[m]) with a = adapter_ids[m], for up to
// NF4DQ_LORA_GROUP_MAX stacks of `adapters` adapters over one x and one id vector), plain C++17
// (no HIP): argument validation with the status codes, cfg validity, the library's choice, the
// launch geometry and the LDS bytes.  Pure arithmetic, shared by the launcher
// (nf4_lora_routed.hip) and a CPU check (tests/plan/lora_routed_plan_check.cpp).  The cfg, its
// validity and the limits are nf4_lora_plan.h's.
//
// Anatomy the numbers describe: the grid is (stack, slot, tile of tile_n columns), flattened,
// stack i owning the blocks [tile0[i], tile0[i + 1]) = slots * tiles_i of them, slot-major
// (block tile0[i] + slot * tiles_i + tile), with slots = min(adapters, M): the host knows M and
// the number of adapters but not the routing, and no more than min(adapters, M) adapters can be
// present.  A workgroup takes the slot-th smallest adapter present in the ids; it forms
// t = rn(x A^T) for that adapter's rows only -- listed in LDS, ascending -- exactly as
// nf4_lora_add's workgroup does for all rows, then expands its tile and scatters the rows.  The
// t image and the partials are sized from M (one adapter may own every row); the row list of
// m_pad 32-bit entries follows them.
#pragma once

#include "nf4_lora_plan.h"

namespace nf4lora {

constexpr int64_t kMaxStride = int64_t(1) << 40;  // elements between adapters of a stack: 63 strides in bytes fit 64 bits with room

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The library's choice.  Every workgroup repeats its adapter's shrink, and up to `slots`
// adapters are live per tile: the narrowest of 64 / 128 / 256 columns whose slots * tiles fit the
// CUs in one round, 256 when none does.  The rule counts every slot as live and has not been swept:
// where most slots are idle (all rows on one adapter of 64) it picks 256 columns where
// nf4_lora_add's rule picks 64 (DESIGN section 4b "The multi-adapter tail").
inline nf4_lora_cfg routed_default_cfg(int64_t M, int32_t adapters, int64_t n_sum, int cus) {
    const int64_t slots = M < adapters ? M : adapters;
    nf4_lora_cfg c{256, (int32_t)kMaxWaves};
    for (int32_t t : {64, 128, 256}) {
        if (slots * ((n_sum + t - 1) / t) <= (int64_t)(cus > 0 ? cus : 1)) { c.tile_n = t; break; }
    }
    return c;
}

struct RoutedPlan {
    uint32_t grid, block, dyn;      // workgroups, threads, dynamic LDS bytes
    uint32_t tile_n, waves;
    uint32_t slots;                 // min(adapters, M): adapters that can be present
    uint32_t mb, rt;                // row tiles per row block (1 | 2), r tiles of the instantiation (1 | 2 | 4 | 8)
    uint32_t m_pad;                 // rows of t in LDS: M rounded up to 16 * mb
    uint32_t ts;                    // elements between rows of t: the largest r padded to 32, + 8
    uint32_t t_bytes, part_bytes;   // t, then the waves' fp32 partials of one row block, rows of 16 * rt + kPartPad floats
    uint32_t list_bytes;            // then the row list, m_pad 32-bit entries
    uint32_t tile0[NF4DQ_LORA_GROUP_MAX + 1];
};

// Geometry of a validated call.
inline RoutedPlan routed_plan(const nf4_lora_cfg& c, int64_t M, int32_t adapters, const nf4_lora_stack* st, int32_t count) {
    RoutedPlan p{};
    p.tile_n = (uint32_t)c.tile_n;
    p.waves = (uint32_t)c.waves;
    p.block = 64u * p.waves;
    p.slots = (uint32_t)(M < adapters ? M : adapters);
    int32_t r_max = 8;
    uint32_t at = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (st[i].r > r_max) r_max = st[i].r;
        p.tile0[i] = at;
        at += p.slots * (uint32_t)((st[i].N + c.tile_n - 1) / c.tile_n);
    }
    for (int32_t i = count; i <= NF4DQ_LORA_GROUP_MAX; ++i) p.tile0[i] = at;
    p.grid = at;
    const uint32_t rtiles = ((uint32_t)r_max + 15u) / 16u;
    p.rt = rtiles <= 1 ? 1 : rtiles <= 2 ? 2 : rtiles <= 4 ? 4 : 8;
    p.mb = M <= 16 ? 1 : 2;
    p.m_pad = (((uint32_t)M + 16u * p.mb - 1) / (16u * p.mb)) * 16u * p.mb;
    p.ts = (((uint32_t)r_max + 31u) & ~31u) + 8u;
    p.t_bytes = p.m_pad * p.ts * 2u;
    p.part_bytes = p.waves * 16u * p.mb * (16u * p.rt + kPartPad) * 4u;
    p.list_bytes = p.m_pad * 4u;
    p.dyn = p.t_bytes + p.part_bytes + p.list_bytes;
    return p;
}

struct RoutedCall {
    const void* x;
    const void* adapter_ids;
    int64_t M, K;
    int32_t adapters;
    const nf4_lora_stack* stacks;
    int32_t count;
    int32_t dtype;
    const nf4_lora_cfg* cfg;
};

// Validates a call: NF4DQ_OK or the status code.  Every NF4DQ_ERR_ARG rule comes before every
// NF4DQ_ERR_SHAPE rule, the size limits last.  Needs nothing of the device.
inline int routed_validate(const RoutedCall& a) {
    if (!a.x || !a.adapter_ids || !a.stacks) return NF4DQ_ERR_ARG;
    if (a.dtype != NF4DQ_F16 && a.dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (a.count < 1 || a.count > NF4DQ_LORA_GROUP_MAX) return NF4DQ_ERR_ARG;
    if (a.adapters < 1 || a.adapters > NF4DQ_LORA_MAX_ADAPTERS) return NF4DQ_ERR_ARG;
    for (int32_t i = 0; i < a.count; ++i) {
        const nf4_lora_stack& s = a.stacks[i];
        if (!s.A || !s.B || !s.scale || !s.y) return NF4DQ_ERR_ARG;
        if (s.r < 8 || s.r > NF4DQ_LORA_MAX_R) return NF4DQ_ERR_ARG;
    }
    if (a.cfg && !valid_cfg(*a.cfg)) return NF4DQ_ERR_ARG;
    if (a.M < 1 || a.M > NF4DQ_LORA_MAX_M || a.K < 32 || a.K % 32) return NF4DQ_ERR_SHAPE;
    if (!aligned16(a.x) || !aligned4(a.adapter_ids)) return NF4DQ_ERR_SHAPE;
    for (int32_t i = 0; i < a.count; ++i) {
        const nf4_lora_stack& s = a.stacks[i];
        if (s.N < 16 || s.N % 16 || s.r % 8) return NF4DQ_ERR_SHAPE;
        if (!aligned16(s.A) || !aligned16(s.B) || !aligned16(s.base) || !aligned16(s.y) || !aligned4(s.scale)) return NF4DQ_ERR_SHAPE;
        if (s.a_stride % 8 || s.b_stride % 8) return NF4DQ_ERR_SHAPE;
        // (K and N may still be above the size limit here: the quotients cannot overflow)
        if (s.a_stride / s.r < a.K || s.b_stride / s.r < s.N) return NF4DQ_ERR_SHAPE;
    }
    if (a.K > kMaxDim) return NF4DQ_ERR_TOO_LARGE;
    for (int32_t i = 0; i < a.count; ++i)
        if (a.stacks[i].N > kMaxDim || a.stacks[i].a_stride > kMaxStride || a.stacks[i].b_stride > kMaxStride) return NF4DQ_ERR_TOO_LARGE;
    return NF4DQ_OK;
}

// Validates a call and answers what runs: NF4DQ_OK and *out, or routed_validate's status code.
// A cfg the caller names never falls back; `cus` matters only without one.
inline int routed_check(const RoutedCall& a, int cus, nf4_lora_cfg* out) {
    const int rc = routed_validate(a);
    if (rc != NF4DQ_OK) return rc;
    int64_t n_sum = 0;
    for (int32_t i = 0; i < a.count; ++i) n_sum += a.stacks[i].N;
    const nf4_lora_cfg c = a.cfg ? *a.cfg : routed_default_cfg(a.M, a.adapters, n_sum, cus);
    if (routed_plan(c, a.M, a.adapters, a.stacks, a.count).dyn > kLdsPerCu) return NF4DQ_ERR_TOO_LARGE;  // unreachable within the limits above
    *out = c;
    return NF4DQ_OK;
}

}  // namespace nf4lora
