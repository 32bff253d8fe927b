// lora_plan_check.cpp -- what the host plan of the fused adapter launch (nf4_lora_plan.h) decides,
// one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..}      check's status for a call built to break one rule (ok_*: none)
//   {"k":"plan","c":[cus,M,K],"N":[..],"r":[..],"named":0/1,"rc":..,"cfg":[tile_n,waves],
//    "geo":[grid,block,dyn,mb,rt,row_blocks,m_pad,ts,t_bytes,part_bytes],"tile0":[count + 1 entries]}
// tests/test_lora_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_lora_plan.h"

using namespace nf4lora;

static void* fake(uintptr_t a) { return reinterpret_cast<void*>(a); }  // never dereferenced

static nf4_lora_mat mat(int64_t N, int32_t r) {
    nf4_lora_mat m{};
    m.A = fake(0x2000);
    m.B = fake(0x3000);
    m.base = fake(0x4000);
    m.y = fake(0x4000);
    m.N = N;
    m.r = r;
    m.scale = 0.5f;
    return m;
}

static LoraCall good(const nf4_lora_mat* m, int32_t count) {
    return LoraCall{fake(0x1000), 8, 256, m, count, NF4DQ_BF16, nullptr};
}

static void err(const char* name, const LoraCall& a) {
    nf4_lora_cfg c{};
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d}\n", name, check(a, 256, &c));
}

static void errors() {
    nf4_lora_mat m[NF4DQ_LORA_GROUP_MAX + 1];
    for (auto& e : m) e = mat(128, 16);
    LoraCall a = good(m, 1);
    err("ok_plain", a);
    a = good(m, NF4DQ_LORA_GROUP_MAX);
    err("ok_full_group", a);
    a = good(m, 1); a.x = nullptr; err("arg_null_x", a);
    a = good(m, 1); a.mats = nullptr; err("arg_null_mats", a);
    a = good(m, 1); a.dtype = NF4DQ_F32; err("arg_dtype_f32", a);
    a = good(m, 1); a.dtype = 7; err("arg_dtype_unknown", a);
    a = good(m, 0); err("arg_count_0", a);
    a = good(m, NF4DQ_LORA_GROUP_MAX + 1); err("arg_count_9", a);
    {
        nf4_lora_mat b[2] = {mat(128, 16), mat(128, 16)};
        b[1].A = nullptr; a = good(b, 2); err("arg_null_A", a);
        b[1] = mat(128, 16); b[1].B = nullptr; a = good(b, 2); err("arg_null_B", a);
        b[1] = mat(128, 16); b[1].y = nullptr; a = good(b, 2); err("arg_null_y", a);
        b[1] = mat(128, 16); b[1].base = nullptr; a = good(b, 2); err("ok_null_base", a);
        b[1] = mat(128, 0); a = good(b, 2); err("arg_r_0", a);
        b[1] = mat(128, 4); a = good(b, 2); err("arg_r_4", a);
        b[1] = mat(128, 136); a = good(b, 2); err("arg_r_136", a);
        b[1] = mat(128, 128); a = good(b, 2); err("ok_r_128", a);
        b[1] = mat(128, 8); a = good(b, 2); err("ok_r_8", a);
        b[1] = mat(128, 12); a = good(b, 2); err("shape_r_12", a);
        b[1] = mat(120, 16); a = good(b, 2); err("shape_n_120", a);
        b[1] = mat(0, 16); a = good(b, 2); err("shape_n_0", a);
        b[1] = mat(16, 16); a = good(b, 2); err("ok_n_16", a);
        b[1] = mat(128, 16); b[1].A = fake(0x2008); a = good(b, 2); err("shape_misaligned_A", a);
        b[1] = mat(128, 16); b[1].B = fake(0x3002); a = good(b, 2); err("shape_misaligned_B", a);
        b[1] = mat(128, 16); b[1].base = fake(0x4004); a = good(b, 2); err("shape_misaligned_base", a);
        b[1] = mat(128, 16); b[1].y = fake(0x4008); a = good(b, 2); err("shape_misaligned_y", a);
        // every ARG rule answers before every SHAPE rule
        b[0] = mat(120, 12); b[1] = mat(128, 4); a = good(b, 2); a.M = 0; err("arg_r_before_shapes", a);
        b[0] = mat(128, 16); b[1] = mat(int64_t(1) << 23, 16); a = good(b, 2); err("too_large_n", a);
        b[1] = mat((int64_t(1) << 23) + 8, 16); a = good(b, 2); err("shape_before_too_large", a);
    }
    a = good(m, 1); a.M = 0; err("shape_m_0", a);
    a = good(m, 1); a.M = -1; err("shape_m_negative", a);
    a = good(m, 1); a.M = 129; err("shape_m_129", a);
    a = good(m, 1); a.M = 128; err("ok_m_128", a);
    a = good(m, 1); a.K = 0; err("shape_k_0", a);
    a = good(m, 1); a.K = 48; err("shape_k_48", a);
    a = good(m, 1); a.K = 32; err("ok_k_32", a);
    a = good(m, 1); a.K = int64_t(1) << 23; err("too_large_k", a);
    a = good(m, 1); a.x = fake(0x1004); err("shape_misaligned_x", a);
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

static void plan_line(int cus, int64_t M, int64_t K, const std::vector<nf4_lora_mat>& m, const nf4_lora_cfg* named) {
    LoraCall a{fake(0x1000), M, K, m.data(), (int32_t)m.size(), NF4DQ_F16, named};
    nf4_lora_cfg c{};
    const int rc = check(a, cus, &c);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%lld],\"N\":[", cus, (long long)M, (long long)K);
    for (size_t i = 0; i < m.size(); ++i) printf("%s%lld", i ? "," : "", (long long)m[i].N);
    printf("],\"r\":[");
    for (size_t i = 0; i < m.size(); ++i) printf("%s%d", i ? "," : "", (int)m[i].r);
    printf("],\"named\":%d,\"rc\":%d", named ? 1 : 0, rc);
    if (rc == NF4DQ_OK) {
        const LoraPlan p = plan(c, M, m.data(), (int32_t)m.size());
        printf(",\"cfg\":[%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u,%u,%u,%u],\"tile0\":[", (int)c.tile_n, (int)c.waves, p.grid,
               p.block, p.dyn, p.mb, p.rt, p.row_blocks, p.m_pad, p.ts, p.t_bytes, p.part_bytes);
        for (size_t i = 0; i <= m.size(); ++i) printf("%s%u", i ? "," : "", p.tile0[i]);
        printf("]");
    }
    printf("}\n");
}

static void plans() {
    const std::vector<std::vector<nf4_lora_mat>> groups = {
        {mat(16, 8)}, {mat(80, 24)}, {mat(192, 32)}, {mat(4096, 16)}, {mat(4096, 64)}, {mat(14336, 16)}, {mat(1024, 128)},
        {mat(4096, 16), mat(1024, 16), mat(1024, 16)}, {mat(14336, 64), mat(14336, 64)},
        {mat(80, 8), mat(192, 128), mat(16, 24)},
        {mat(64, 8), mat(64, 8), mat(64, 8), mat(64, 8), mat(64, 8), mat(64, 8), mat(64, 8), mat(64, 8)}};
    for (int cus : {256, 64, 1})
        for (int64_t M : {1, 5, 16, 17, 32, 33, 128})
            for (int64_t K : {32, 96, 384, 4096, 14336})
                for (const auto& g : groups) {
                    plan_line(cus, M, K, g, nullptr);
                    if (cus != 256) continue;
                    for (int32_t t : {16, 32, 64, 128, 256})
                        for (int32_t w : {1, 2, 4}) {
                            nf4_lora_cfg c{t, w};
                            plan_line(cus, M, K, g, &c);
                        }
                }
}

int main() {
    errors();
    plans();
    return 0;
}
