// nf4_lora_routed_plan.h -- the host-side plan of the routed adapter launch (nf4_lora_add_routed:
// y_i[m] = base_i[m] + scale_i[a] * B_i[a] (A_i[a] x[m]) with a = adapter_ids[m], for up to
// NF4DQ_LORA_GROUP_MAX stacks of `adapters` adapters over one x and one id vector), plain C++17
// (no HIP), shared by the launcher (nf4_lora_routed.hip) and a CPU check
// (tests/plan/lora_routed_plan_check.cpp).  The cfg, its validity, the limits, the per-matrix
// rules, the geometry and the default-cfg rule are nf4_lora_plan.h's; here are only the routed
// launch's own: `adapters`, the ids and scale alignment, the strides, the slots and the row list.
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

inline int64_t routed_slots(int64_t M, int32_t adapters) { return M < adapters ? M : adapters; }

// The library's choice: nf4_lora_add's rule with up to `slots` adapters live per tile.  The rule
// counts every slot as live and has not been swept: where most slots are idle (all rows on one
// adapter of 64) it picks 256 columns where nf4_lora_add's rule picks 64 (DESIGN section 4b "The
// multi-adapter tail").
inline nf4_lora_cfg routed_default_cfg(int64_t M, int32_t adapters, int64_t n_sum, int cus) {
    return default_cfg(n_sum, cus, routed_slots(M, adapters));
}

struct RoutedPlan : LoraPlan {  // row_blocks: those of all M rows (a workgroup runs its own adapter's)
    uint32_t slots;       // min(adapters, M): adapters that can be present
    uint32_t list_bytes;  // behind t and the partials, the row list: m_pad 32-bit entries
};

// Geometry of a validated call.
inline RoutedPlan routed_plan(const nf4_lora_cfg& c, int64_t M, int32_t adapters, const nf4_lora_stack* st, int32_t count) {
    const uint32_t slots = (uint32_t)routed_slots(M, adapters);
    RoutedPlan p{plan(c, M, st, count, slots), slots, 0};
    p.list_bytes = p.m_pad * 4u;
    p.dyn += p.list_bytes;
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

// The routed launch's rules beside the shared ones, by class (nf4_lora_plan.h: validate_mats).
struct RoutedRules {
    const RoutedCall& a;
    bool call_arg() const { return !a.adapter_ids || a.adapters < 1 || a.adapters > NF4DQ_LORA_MAX_ADAPTERS; }
    bool call_shape() const { return !aligned4(a.adapter_ids); }
    bool arg(const nf4_lora_stack& s) const { return !s.scale; }
    bool shape(const nf4_lora_stack& s) const {
        if (!aligned4(s.scale) || s.a_stride % 8 || s.b_stride % 8) return true;
        // (K and N may still be above the size limit here: the quotients cannot overflow)
        return s.a_stride / s.r < a.K || s.b_stride / s.r < s.N;
    }
    bool too_large(const nf4_lora_stack& s) const { return s.a_stride > kMaxStride || s.b_stride > kMaxStride; }
};

// Validates a call: NF4DQ_OK or the status code.
inline int routed_validate(const RoutedCall& a) {
    return validate_mats(a.x, a.M, a.K, a.stacks, a.count, a.dtype, a.cfg, RoutedRules{a});
}

// Validates a call and answers what runs: NF4DQ_OK and *out, or routed_validate's status code.
inline int routed_check(const RoutedCall& a, int cus, nf4_lora_cfg* out) {
    return choose_cfg(routed_validate(a), a.cfg, a.stacks, a.count, cus, routed_slots(a.M, a.adapters),
                      [&](const nf4_lora_cfg& c) { return routed_plan(c, a.M, a.adapters, a.stacks, a.count).dyn; }, out);
}

}  // namespace nf4lora
