// lora_routed_plan_check.cpp -- what the host plan of the routed adapter launch
// (nf4_lora_routed_plan.h) decides, one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..}      routed_check's status for a call built to break one rule (ok_*: none)
//   {"k":"plan","c":[cus,M,K,S],"N":[..],"r":[..],"named":0/1,"rc":..,"cfg":[tile_n,waves],
//    "geo":[grid,block,dyn,slots,mb,rt,m_pad,ts,t_bytes,part_bytes,list_bytes],"tile0":[count + 1 entries]}
// tests/test_lora_routed_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_lora_routed_plan.h"

using namespace nf4lora;

static void* fake(uintptr_t a) { return reinterpret_cast<void*>(a); }  // never dereferenced

static const int64_t kK = 256;

static nf4_lora_stack stack(int64_t N, int32_t r, int64_t K = kK) {
    nf4_lora_stack s{};
    s.A = fake(0x2000);
    s.B = fake(0x3000);
    s.scale = reinterpret_cast<const float*>(fake(0x5000));
    s.base = fake(0x4000);
    s.y = fake(0x4000);
    s.N = N;
    s.a_stride = (int64_t)r * K;
    s.b_stride = N * r;
    s.r = r;
    return s;
}

static RoutedCall good(const nf4_lora_stack* s, int32_t count) {
    return RoutedCall{fake(0x1000), fake(0x6000), 8, kK, 4, s, count, NF4DQ_BF16, nullptr};
}

static void err(const char* name, const RoutedCall& a) {
    nf4_lora_cfg c{};
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d}\n", name, routed_check(a, 256, &c));
}

static void errors() {
    nf4_lora_stack m[NF4DQ_LORA_GROUP_MAX + 1];
    for (auto& e : m) e = stack(128, 16);
    RoutedCall a = good(m, 1);
    err("ok_plain", a);
    a = good(m, NF4DQ_LORA_GROUP_MAX);
    err("ok_full_group", a);
    a = good(m, 1); a.x = nullptr; err("arg_null_x", a);
    a = good(m, 1); a.adapter_ids = nullptr; err("arg_null_ids", a);
    a = good(m, 1); a.stacks = nullptr; err("arg_null_stacks", a);
    a = good(m, 1); a.dtype = NF4DQ_F32; err("arg_dtype_f32", a);
    a = good(m, 1); a.dtype = 7; err("arg_dtype_unknown", a);
    a = good(m, 0); err("arg_count_0", a);
    a = good(m, NF4DQ_LORA_GROUP_MAX + 1); err("arg_count_9", a);
    a = good(m, 1); a.adapters = 0; err("arg_adapters_0", a);
    a = good(m, 1); a.adapters = -1; err("arg_adapters_negative", a);
    a = good(m, 1); a.adapters = NF4DQ_LORA_MAX_ADAPTERS + 1; err("arg_adapters_65", a);
    a = good(m, 1); a.adapters = NF4DQ_LORA_MAX_ADAPTERS; err("ok_adapters_64", a);
    a = good(m, 1); a.adapters = 1; err("ok_adapters_1", a);
    {
        nf4_lora_stack b[2] = {stack(128, 16), stack(128, 16)};
        b[1].A = nullptr; a = good(b, 2); err("arg_null_A", a);
        b[1] = stack(128, 16); b[1].B = nullptr; a = good(b, 2); err("arg_null_B", a);
        b[1] = stack(128, 16); b[1].scale = nullptr; a = good(b, 2); err("arg_null_scale", a);
        b[1] = stack(128, 16); b[1].y = nullptr; a = good(b, 2); err("arg_null_y", a);
        b[1] = stack(128, 16); b[1].base = nullptr; a = good(b, 2); err("ok_null_base", a);
        b[1] = stack(128, 16); b[1].r = 0; a = good(b, 2); err("arg_r_0", a);
        b[1] = stack(128, 16); b[1].r = 4; a = good(b, 2); err("arg_r_4", a);
        b[1] = stack(128, 136); a = good(b, 2); err("arg_r_136", a);
        b[1] = stack(128, 128); a = good(b, 2); err("ok_r_128", a);
        b[1] = stack(128, 8); a = good(b, 2); err("ok_r_8", a);
        b[1] = stack(128, 16); b[1].r = 12; a = good(b, 2); err("shape_r_12", a);
        b[1] = stack(120, 16); a = good(b, 2); err("shape_n_120", a);
        b[1] = stack(0, 16); a = good(b, 2); err("shape_n_0", a);
        b[1] = stack(16, 16); a = good(b, 2); err("ok_n_16", a);
        b[1] = stack(128, 16); b[1].A = fake(0x2008); a = good(b, 2); err("shape_misaligned_A", a);
        b[1] = stack(128, 16); b[1].B = fake(0x3002); a = good(b, 2); err("shape_misaligned_B", a);
        b[1] = stack(128, 16); b[1].base = fake(0x4004); a = good(b, 2); err("shape_misaligned_base", a);
        b[1] = stack(128, 16); b[1].y = fake(0x4008); a = good(b, 2); err("shape_misaligned_y", a);
        b[1] = stack(128, 16); b[1].scale = reinterpret_cast<const float*>(fake(0x5002)); a = good(b, 2); err("shape_misaligned_scale", a);
        b[1] = stack(128, 16); b[1].a_stride += 4; a = good(b, 2); err("shape_a_stride_odd", a);
        b[1] = stack(128, 16); b[1].b_stride += 4; a = good(b, 2); err("shape_b_stride_odd", a);
        b[1] = stack(128, 16); b[1].a_stride -= 8; a = good(b, 2); err("shape_a_stride_small", a);
        b[1] = stack(128, 16); b[1].b_stride -= 8; a = good(b, 2); err("shape_b_stride_small", a);
        b[1] = stack(128, 16); b[1].a_stride = 0; a = good(b, 2); err("shape_a_stride_0", a);
        b[1] = stack(128, 16); b[1].b_stride = -2048; a = good(b, 2); err("shape_b_stride_negative", a);
        b[1] = stack(128, 16); b[1].a_stride += 8; b[1].b_stride += 4096; a = good(b, 2); err("ok_strides_padded", a);
        b[1] = stack(128, 16); b[1].a_stride = (int64_t(1) << 40) + 8; a = good(b, 2); err("too_large_a_stride", a);
        b[1] = stack(128, 16); b[1].b_stride = (int64_t(1) << 40) + 8; a = good(b, 2); err("too_large_b_stride", a);
        b[1] = stack(128, 16); b[1].a_stride = int64_t(1) << 40; a = good(b, 2); err("ok_a_stride_2_40", a);
        // every ARG rule answers before every SHAPE rule
        b[0] = stack(120, 16); b[0].r = 12; b[1] = stack(128, 16); b[1].r = 4; a = good(b, 2); a.M = 0; err("arg_r_before_shapes", a);
        b[0] = stack(120, 16); b[1] = stack(128, 16); a = good(b, 2); a.adapters = 65; err("arg_adapters_before_shapes", a);
        b[0] = stack(128, 16); b[1] = stack(int64_t(1) << 23, 16); a = good(b, 2); err("too_large_n", a);
        b[1] = stack((int64_t(1) << 23) + 8, 16); a = good(b, 2); err("shape_before_too_large", a);
        b[1] = stack(int64_t(1) << 23, 16); b[1].b_stride += 4; a = good(b, 2); err("shape_stride_before_too_large", a);
    }
    a = good(m, 1); a.M = 0; err("shape_m_0", a);
    a = good(m, 1); a.M = -1; err("shape_m_negative", a);
    a = good(m, 1); a.M = 129; err("shape_m_129", a);
    a = good(m, 1); a.M = 128; err("ok_m_128", a);
    a = good(m, 1); a.K = 0; err("shape_k_0", a);
    a = good(m, 1); a.K = 48; err("shape_k_48", a);
    a = good(m, 1); a.K = 32; err("ok_k_32", a);
    a = good(m, 1); a.K = 512; err("shape_k_beyond_a_stride", a);
    {
        nf4_lora_stack b = stack(128, 16, int64_t(1) << 23);
        a = good(&b, 1); a.K = int64_t(1) << 23; err("too_large_k", a);
    }
    a = good(m, 1); a.x = fake(0x1004); err("shape_misaligned_x", a);
    a = good(m, 1); a.adapter_ids = fake(0x6002); err("shape_misaligned_ids", a);
    a = good(m, 1); a.adapter_ids = fake(0x6004); err("ok_ids_4_byte_aligned", a);
    for (int32_t t : {0, 8, 48, 512, -16}) {
        nf4_lora_cfg c{t, 4};
        a = good(m, 1); a.cfg = &c;
        char name[64];
        snprintf(name, sizeof name, "arg_cfg_tile_%d", (int)t);
        err(name, a);
    }
    for (int32_t w : {0, 3, 8, -1}) {
        nf4_lora_cfg c{64, w};
        a = good(m, 1); a.cfg = &c;
        char name[64];
        snprintf(name, sizeof name, "arg_cfg_waves_%d", (int)w);
        err(name, a);
    }
    {
        nf4_lora_cfg c{48, 4};
        a = good(m, 1); a.cfg = &c; a.M = 129; err("arg_cfg_before_shapes", a);
    }
}

static void plan_line(int cus, int64_t M, int64_t K, int32_t S, const std::vector<nf4_lora_stack>& m, const nf4_lora_cfg* named) {
    RoutedCall a{fake(0x1000), fake(0x6000), M, K, S, m.data(), (int32_t)m.size(), NF4DQ_F16, named};
    nf4_lora_cfg c{};
    const int rc = routed_check(a, cus, &c);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%lld,%d],\"N\":[", cus, (long long)M, (long long)K, (int)S);
    for (size_t i = 0; i < m.size(); ++i) printf("%s%lld", i ? "," : "", (long long)m[i].N);
    printf("],\"r\":[");
    for (size_t i = 0; i < m.size(); ++i) printf("%s%d", i ? "," : "", (int)m[i].r);
    printf("],\"named\":%d,\"rc\":%d", named ? 1 : 0, rc);
    if (rc == NF4DQ_OK) {
        const RoutedPlan p = routed_plan(c, M, S, m.data(), (int32_t)m.size());
        printf(",\"cfg\":[%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u],\"tile0\":[", (int)c.tile_n, (int)c.waves, p.grid,
               p.block, p.dyn, p.slots, p.mb, p.rt, p.m_pad, p.ts, p.t_bytes, p.part_bytes, p.list_bytes);
        for (size_t i = 0; i <= m.size(); ++i) printf("%s%u", i ? "," : "", p.tile0[i]);
        printf("]");
    }
    printf("}\n");
}

static void plans() {
    for (int cus : {256, 64, 1})
        for (int64_t M : {1, 5, 16, 17, 64, 65, 128})
            for (int64_t K : {32, 96, 4096, 14336})
                for (int32_t S : {1, 3, 8, 64}) {
                    const std::vector<std::vector<nf4_lora_stack>> groups = {
                        {stack(16, 8, K)}, {stack(80, 24, K)}, {stack(144, 40, K)}, {stack(4096, 16, K)}, {stack(4096, 64, K)},
                        {stack(14336, 16, K)}, {stack(1024, 128, K)}, {stack(4096, 16, K), stack(1024, 16, K), stack(1024, 16, K)},
                        {stack(80, 8, K), stack(144, 128, K), stack(16, 24, K)},
                        {stack(64, 8, K), stack(64, 8, K), stack(64, 8, K), stack(64, 8, K), stack(64, 8, K), stack(64, 8, K),
                         stack(64, 8, K), stack(64, 8, K)}};
                    for (const auto& g : groups) {
                        plan_line(cus, M, K, S, g, nullptr);
                        if (cus != 256) continue;
                        for (int32_t t : {16, 32, 64, 128, 256})
                            for (int32_t w : {1, 2, 4}) {
                                nf4_lora_cfg c{t, w};
                                plan_line(cus, M, K, S, g, &c);
                            }
                    }
                }
}

int main() {
    errors();
    plans();
    return 0;
}
