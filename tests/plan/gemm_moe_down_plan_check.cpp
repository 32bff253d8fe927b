// gemm_moe_down_plan_check.cpp -- what the host plan of the fused expert down projection with the
// routed sum (nf4_gemm_moe_down_plan.h) decides, one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..,"launch":0/1}   down_check's status for a call built to break one rule
//   {"k":"plan","c":[cus,P,E,N,K],"named":0/1,"rc":..,"cfg":[kernel,waves,depth,ksplit,strips],
//    "moe":[the same five fields of moe_default_cfg / of the named cfg under the expert GEMM's id],
//    "geo":[grid,block,dyn,tiles,chunks,cps,row_tiles,tickets],"mgeo":[moe_plan's same eight],
//    "counters":..,"slab":..,"scratch_at":..,"need":..,"ws":..}
//       need = what the launcher checks the workspace against (bisected over workspace_bytes),
//       ws = down_workspace_need, what the size entry answers
// tests/test_gemm_moe_down_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_moe_down_plan.h"

using namespace nf4gemm;

static uint8_t* fake(uintptr_t a) { return reinterpret_cast<uint8_t*>(a); }  // never dereferenced

static nf4_moe_experts stack(bool single, int32_t E, int64_t N, int64_t K) {
    const int64_t nblk = N * K / 64;
    nf4_moe_experts e{};
    e.packed = fake(0x2000);
    e.packed_stride = N * (K / 2);
    e.absmax_q = single ? nullptr : fake(0x3000);
    e.nb_stride = single ? 0 : nblk;
    e.code2 = single ? nullptr : reinterpret_cast<const float*>(fake(0x4000));
    e.code2_stride = 0;
    e.absmax2 = reinterpret_cast<const float*>(fake(0x5000));
    e.n2_stride = single ? nblk : (nblk + 255) / 256;
    e.offset = single ? nullptr : reinterpret_cast<const float*>(fake(0x7000));
    e.N = N;
    e.K = K;
    e.experts = E;
    e.single = single ? 1 : 0;
    e.blocksize = 64;
    e.blocksize2 = single ? 0 : 256;
    return e;
}

static DownCall good(const nf4_moe_experts* e, int64_t P, int32_t topk) {
    DownCall a{};
    a.m.x = fake(0x1000);
    a.m.ids = fake(0x8000);
    a.m.P = P;
    a.m.x_div = 1;
    a.m.ex = e;
    a.m.y = fake(0x6000);
    a.m.dtype = NF4DQ_BF16;
    a.m.workspace = fake(0x100000);
    a.m.workspace_bytes = size_t(1) << 31;
    a.m.cfg = nullptr;
    a.topk = topk;
    a.rw = fake(0x9000);
    a.rw_dtype = NF4DQ_F32;
    return a;
}

static void err(const char* name, const DownCall& a) {
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = down_check(a, 256, &c, &launch);
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d,\"launch\":%d}\n", name, rc, launch ? 1 : 0);
}

static void errors() {
    const int64_t P = 64, N = 128, K = 1024;
    const int32_t E = 8;
    nf4_moe_experts e = stack(false, E, N, K);
    auto fresh = [&]() {
        e = stack(false, E, N, K);
        return good(&e, P, 2);
    };
    DownCall a = fresh();
    err("ok_", a);
    a = fresh(), a.rw_dtype = NF4DQ_BF16;
    err("ok_rw_out_dtype", a);
    a = fresh(), a.m.dtype = NF4DQ_F16, a.rw_dtype = NF4DQ_F16, a.rw = fake(0x9002);
    err("ok_rw_f16_2_byte_aligned", a);
    a = fresh(), a.rw_dtype = NF4DQ_F16;
    err("arg_rw_other_16_bit_dtype", a);
    a = fresh(), a.rw_dtype = 7;
    err("arg_rw_dtype", a);
    a = fresh(), a.rw = nullptr;
    err("arg_null_rw", a);
    a = fresh(), a.rw = fake(0x9002);
    err("arg_misaligned_rw_f32", a);
    a = fresh(), a.rw_dtype = NF4DQ_BF16, a.rw = fake(0x9001);
    err("arg_misaligned_rw_16", a);
    a = fresh(), a.topk = 0;
    err("arg_topk_0", a);
    a = fresh(), a.topk = -1;
    err("arg_topk_negative", a);
    a = fresh(), a.topk = 3;
    err("arg_topk_not_dividing", a);
    a = fresh(), a.topk = 128;
    err("arg_topk_beyond_p", a);
    a = fresh(), a.topk = 64;
    err("ok_topk_p", a);
    a = fresh(), a.topk = 1;
    err("ok_topk_1", a);
    // the expert GEMM's rules, with its codes
    a = fresh(), a.m.dtype = NF4DQ_F32;
    err("arg_dtype", a);
    a = fresh(), a.m.ex = nullptr;
    err("arg_null_experts", a);
    a = fresh(), a.m.y = nullptr;
    err("arg_null_y", a);
    a = fresh(), a.m.y = fake(0x6004);
    err("arg_misaligned_y", a);
    a = fresh(), a.m.x = fake(0x1008);
    err("arg_misaligned_x", a);
    a = fresh(), a.m.x_div = 0;
    err("arg_x_div_0", a);
    a = fresh(), a.m.P = 0, a.topk = 0, a.rw = nullptr, a.m.x = nullptr, a.m.y = nullptr, a.m.ids = nullptr, a.m.workspace = nullptr;
    err("ok_p0_nothing", a);
    a = fresh(), a.m.P = 129, a.topk = 1;
    err("shape_p129", a);
    a = fresh(), e.blocksize = 128;
    err("shape_blocksize_128", a);
    e = stack(false, E, 96, K), a = good(&e, P, 2);
    err("shape_n96", a);
    e = stack(false, E, N, 1088), a = good(&e, P, 2);
    err("shape_k1088", a);
    e = stack(false, E, int64_t(1) << 19, 128), a = good(&e, P, 2);
    err("too_large_n", a);
    // the order: a rule of the expert GEMM answers before topk does
    a = fresh(), a.topk = 0, a.m.P = 129;
    err("shape_before_topk", a);
    a = fresh(), a.topk = 0, a.rw_dtype = 7, a.m.P = 129;
    err("arg_rw_dtype_first", a);
    // cfgs: this entry's id or 0, never another family's; one slice still needs the workspace
    const nf4_gemm_cfg one{NF4DQ_GEMM_MOE_DOWN, 4, 1, 1, 2}, four{NF4DQ_GEMM_MOE_DOWN, 4, 1, 4, 2}, k0{0, 2, 1, 8, 0};
    const nf4_gemm_cfg moe{NF4DQ_GEMM_MOE, 4, 1, 1, 2}, bad{NF4DQ_GEMM_MOE_DOWN, 4, 1, 9, 2}, w3{NF4DQ_GEMM_MOE_DOWN, 3, 1, 1, 2};
    a = fresh(), a.m.cfg = &one;
    err("ok_cfg_one_slice", a);
    a = fresh(), a.m.cfg = &k0;
    err("ok_cfg_kernel_0", a);
    a = fresh(), a.m.cfg = &moe;
    err("arg_cfg_expert_gemm_id", a);
    a = fresh(), a.m.cfg = &bad;
    err("arg_cfg_ksplit", a);
    a = fresh(), a.m.cfg = &w3;
    err("arg_cfg_waves", a);
    a = fresh(), a.m.cfg = &one, a.m.workspace = nullptr;
    err("arg_one_slice_no_workspace", a);
    a = fresh(), a.m.cfg = &four, a.m.workspace = nullptr;
    err("arg_no_workspace", a);
    a = fresh(), a.m.cfg = &four, a.m.workspace = fake(0x100008);
    err("arg_misaligned_workspace", a);
    a = fresh(), a.m.cfg = &four, a.m.workspace_bytes = kHeaderBytes + 4 * P * N * 4 + P * N * 2 - 1;
    err("arg_short_workspace", a);
    a = fresh(), a.m.cfg = &four, a.m.workspace_bytes = kHeaderBytes + 4 * P * N * 4 + P * N * 2;
    err("ok_exact_workspace", a);
    a = fresh(), a.m.cfg = &one, a.m.workspace_bytes = kHeaderBytes + P * N * 2 - 1;
    err("arg_short_workspace_one_slice", a);
    a = fresh(), a.m.cfg = &one, a.m.workspace_bytes = kHeaderBytes + P * N * 2;
    err("ok_exact_workspace_one_slice", a);
    // the tickets: (experts + 1) x column tiles words among the 16384 of the header, one slice included.
    // 127 experts x 128 tiles of 64 columns: 128 * 128 = 16384 fit; 128 experts: 129 * 128 do not
    const nf4_gemm_cfg narrow{NF4DQ_GEMM_MOE_DOWN, 2, 1, 1, 2};
    e = stack(false, 127, 8192, 256), a = good(&e, P, 2), a.m.cfg = &narrow;
    err("ok_tickets_fill_the_header", a);
    e = stack(false, 128, 8192, 256), a = good(&e, P, 2), a.m.cfg = &narrow;
    err("too_large_tickets_one_slice", a);
    e = stack(false, 128, 8192, 256), a = good(&e, P, 2), a.m.cfg = &narrow, a.m.workspace = nullptr;
    err("too_large_tickets_before_workspace", a);
}

// The smallest workspace_bytes down_check accepts: what the launcher needs.
static size_t launcher_need(DownCall a, int cus) {
    nf4_gemm_cfg c{};
    bool launch = false;
    a.m.workspace_bytes = 0;
    if (down_check(a, cus, &c, &launch) == NF4DQ_OK) return 0;
    size_t lo = 0, hi = size_t(1) << 33;  // lo rejected, hi accepted
    a.m.workspace_bytes = hi;
    if (down_check(a, cus, &c, &launch) != NF4DQ_OK) return ~size_t(0);
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        a.m.workspace_bytes = mid;
        (down_check(a, cus, &c, &launch) == NF4DQ_OK ? hi : lo) = mid;
    }
    return hi;
}

static void plan(int cus, int64_t P, int32_t E, int64_t N, int64_t K, const nf4_gemm_cfg* named) {
    const nf4_moe_experts e = stack(false, E, N, K);
    DownCall a = good(&e, P, P % 2 ? 1 : 2);
    a.m.cfg = named;
    a.m.workspace_bytes = size_t(1) << 33;
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = down_check(a, cus, &c, &launch);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%d,%lld,%lld],\"named\":%d,\"rc\":%d", cus, (long long)P, E, (long long)N,
           (long long)K, named ? 1 : 0, rc);
    if (rc == NF4DQ_OK && launch) {
        nf4_gemm_cfg m = named ? *named : moe_default_cfg(P, E, N, K, cus);
        if (named) m.kernel = NF4DQ_GEMM_MOE, m.strips = kMtStrips;
        const MoePlan p = down_plan(c, P, E, N, K), q = moe_plan(m, P, E, N, K);
        printf(",\"cfg\":[%d,%d,%d,%d,%d],\"moe\":[%d,%d,%d,%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u,%u],"
               "\"mgeo\":[%u,%u,%u,%u,%u,%u,%u,%u],\"counters\":%zu,\"slab\":%zu,\"scratch_at\":%zu,\"need\":%zu,\"ws\":%zu",
               c.kernel, c.waves, c.depth, c.ksplit, c.strips, m.kernel, m.waves, m.depth, m.ksplit, m.strips, p.grid,
               p.block, p.dyn, p.tiles, p.chunks, p.cps, p.row_tiles, p.tickets, q.grid, q.block, q.dyn, q.tiles, q.chunks,
               q.cps, q.row_tiles, q.tickets, down_counters(p), down_slab_bytes(P, N, c), down_scratch_offset(P, N, c),
               launcher_need(a, cus), down_workspace_need(P, N, K, c));
    }
    printf("}\n");
}

int main() {
    errors();
    // Mixtral-8x7B's w2 (and w1 / w3's shape): 8 experts, top-2; 1, 4, 16 and 64 tokens
    const int64_t shapes[][2] = {{4096, 14336}, {14336, 4096}};
    for (int cus : {256, 64})
        for (const auto& s : shapes)
            for (int64_t P : {2, 8, 32, 128}) plan(cus, P, 8, s[0], s[1], nullptr);
    // the tests' small shapes and every cfg of the family over them
    const int64_t small[][3] = {{4, 128, 256}, {4, 128, 384}, {4, 192, 768}};
    for (const auto& s : small)
        for (int64_t P : {1, 2, 12, 34, 96, 128}) {
            const int32_t E = (int32_t)s[0];
            plan(256, P, E, s[1], s[2], nullptr);
            for (int waves : {1, 2, 3, 4, 8})
                for (int depth : {1, 2})
                    for (int strips : {0, 1, 2, 4})
                        for (int ks = 0; ks <= 18; ++ks) {
                            const nf4_gemm_cfg c{NF4DQ_GEMM_MOE_DOWN, waves, depth, ks, strips};
                            const nf4_gemm_cfg m{NF4DQ_GEMM_MOE, waves, depth, ks, strips};
                            if (valid_down_cfg(c, P, s[1], s[2]) != valid_moe_cfg(m, P, s[1], s[2])) return 2;
                            if (valid_down_cfg(c, P, s[1], s[2])) plan(256, P, E, s[1], s[2], &c);
                        }
        }
    return 0;
}
