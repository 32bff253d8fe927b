// nf4_lora.hip -- the fused adapter launch of a Linear4bit (nf4_lora_add: y_i = base_i +
// scale_i * B_i (A_i x) for up to NF4DQ_LORA_GROUP_MAX adapters over one x): the kernel's
// arguments and the C entry.  The plan -- validation, cfg, geometry, LDS -- is nf4_lora_plan.h; the
// kernel (lora_kernel with ROUTED = false: one workgroup per (adapter, tile of tile_n columns),
// over all M rows), shared with the routed launch, and the launch helpers are nf4_lora_dev.h.
#include "nf4_lora_dev.h"

namespace {

using namespace nf4lora;

struct LoraMat {
    const char* A;
    const char* B;
    const uint16_t* base;
    uint16_t* y;
    uint32_t N, r;
    float scale;
    uint32_t tile0;  // the adapter's first workgroup
};

struct LoraArgs {
    const char* x;
    uint32_t M, K, nmat, tile_n;
    uint32_t row_blocks, ts, t_bytes;
    LoraMat m[NF4DQ_LORA_GROUP_MAX];
};

}  // namespace

extern "C" int nf4_lora_add(const void* x, int64_t M, int64_t K, const void* mats, int32_t count, int32_t dtype,
                            const void* cfg, void* hip_stream) {
    const nf4_lora_mat* hm = reinterpret_cast<const nf4_lora_mat*>(mats);
    const LoraCall call{x, M, K, hm, count, dtype, reinterpret_cast<const nf4_lora_cfg*>(cfg)};
    int rc = validate(call);  // every rule answers before any device work
    if (rc) return rc;
    nf4_lora_cfg c{};
    rc = check(call, call.cfg ? 0 : device_cus(), &c);
    if (rc) return rc;
    const LoraPlan p = plan(c, M, hm, count);
    LoraArgs A{};
    A.x = reinterpret_cast<const char*>(x);
    A.M = (uint32_t)M;
    A.K = (uint32_t)K;
    A.nmat = (uint32_t)count;
    A.tile_n = p.tile_n;
    A.row_blocks = p.row_blocks;
    A.ts = p.ts;
    A.t_bytes = p.t_bytes;
    for (int32_t i = 0; i < count; ++i)
        A.m[i] = LoraMat{reinterpret_cast<const char*>(hm[i].A), reinterpret_cast<const char*>(hm[i].B),
                         reinterpret_cast<const uint16_t*>(hm[i].base), reinterpret_cast<uint16_t*>(hm[i].y),
                         (uint32_t)hm[i].N, (uint32_t)hm[i].r, hm[i].scale, p.tile0[i]};
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return lora_dispatch(dtype, p, [&](auto dt, auto mb, auto rt) {
        return lora_launch<lora_kernel<decltype(dt)::value, decltype(mb)::value, decltype(rt)::value, false, LoraArgs>>(p, A, st);
    });
}
