// nf4_lora_routed.hip -- the routed adapter launch of a Linear4bit (nf4_lora_add_routed: row m of
// the batch takes adapter adapter_ids[m] of each stack): the kernel's arguments and the C entry.
// The plan -- validation, cfg, geometry, LDS -- is nf4_lora_routed_plan.h; the kernel (lora_kernel
// with ROUTED = true), shared with nf4_lora_add, and the launch helpers are nf4_lora_dev.h.
//
// One workgroup per (stack, slot, tile of tile_n columns).  Every wave reads the M ids (two per
// lane, in-bounds repeats past M), ORs the ids present into one 64-bit set and takes the slot-th
// smallest as its adapter; two ballots give that adapter's rows, which wave 0 lists in LDS in
// ascending order by popcount prefix.  A slot beyond the adapters present returns before any load
// of x, A, B or scale; slot 0's workgroups first store the rows without an adapter (base, or
// zeros) when base != y.  From there the workgroup is nf4_lora_add's over its listed rows: the x
// rows gathered through the list, the y rows scattered through it.
#include "nf4_lora_dev.h"
#include "nf4_lora_routed_plan.h"

namespace {

using namespace nf4lora;

struct RoutedStack {
    const char* A;
    const char* B;
    const float* scale;
    const uint16_t* base;
    uint16_t* y;
    uint64_t a_bytes, b_bytes;  // bytes between adapters
    uint32_t N, r;
    uint32_t tile0;  // the stack's first workgroup
    uint32_t tiles;  // column tiles of the stack
};

struct RoutedArgs {
    const char* x;
    const int32_t* ids;
    uint32_t M, K, S, nmat, tile_n;  // nmat: stacks
    uint32_t ts, t_bytes, part_bytes;
    RoutedStack m[NF4DQ_LORA_GROUP_MAX];
};

}  // namespace

extern "C" int nf4_lora_add_routed(const void* x, const void* adapter_ids, int64_t M, int64_t K, int32_t adapters,
                                   const void* stacks, int32_t count, int32_t dtype, const void* cfg, void* hip_stream) {
    const nf4_lora_stack* hs = reinterpret_cast<const nf4_lora_stack*>(stacks);
    const RoutedCall call{x, adapter_ids, M, K, adapters, hs, count, dtype, reinterpret_cast<const nf4_lora_cfg*>(cfg)};
    int rc = routed_validate(call);  // every rule answers before any device work
    if (rc) return rc;
    nf4_lora_cfg c{};
    rc = routed_check(call, call.cfg ? 0 : device_cus(), &c);
    if (rc) return rc;
    const RoutedPlan p = routed_plan(c, M, adapters, hs, count);
    RoutedArgs A{};
    A.x = reinterpret_cast<const char*>(x);
    A.ids = reinterpret_cast<const int32_t*>(adapter_ids);
    A.M = (uint32_t)M;
    A.K = (uint32_t)K;
    A.S = (uint32_t)adapters;
    A.nmat = (uint32_t)count;
    A.tile_n = p.tile_n;
    A.ts = p.ts;
    A.t_bytes = p.t_bytes;
    A.part_bytes = p.part_bytes;
    for (int32_t i = 0; i < count; ++i)
        A.m[i] = RoutedStack{reinterpret_cast<const char*>(hs[i].A), reinterpret_cast<const char*>(hs[i].B), hs[i].scale,
                             reinterpret_cast<const uint16_t*>(hs[i].base), reinterpret_cast<uint16_t*>(hs[i].y),
                             (uint64_t)hs[i].a_stride * 2u, (uint64_t)hs[i].b_stride * 2u, (uint32_t)hs[i].N, (uint32_t)hs[i].r,
                             p.tile0[i], (p.tile0[i + 1] - p.tile0[i]) / p.slots};
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return lora_dispatch(dtype, p, [&](auto dt, auto mb, auto rt) {
        return lora_launch<lora_kernel<decltype(dt)::value, decltype(mb)::value, decltype(rt)::value, true, RoutedArgs>>(p, A, st);
    });
}
