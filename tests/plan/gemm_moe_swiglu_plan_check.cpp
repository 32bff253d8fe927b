// gemm_moe_swiglu_plan_check.cpp -- what the fused expert SwiGLU launch's host plan
// (nf4_gemm_moe_swiglu_plan.h) decides, one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..,"launch":0/1}   msg_check's status for a call built to break one rule
//   {"k":"plan","c":[cus,P,E,I,K],"named":0/1,"rc":..,"cfg":[kernel,waves,depth,ksplit,strips],
//    "geo":[grid,block,dyn,tiles,chunks,cps,row_tiles,tickets],"need":..,"ws":..}
//       the launch of the library's choice (named 0) or of a named cfg (named 1), which then is
//       also "asked":[kernel,waves,depth,ksplit,strips]; need = what the launcher checks the
//       workspace against (found by bisecting msg_check's answer over workspace_bytes), ws =
//       msg_workspace_need, what the size entry answers
//   {"k":"cfgs","c":[cus,P,E,I,K],"valid":..,"lds_max":..}   over every cfg of the family's grid
// tests/test_gemm_moe_swiglu_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_moe_swiglu_plan.h"

using namespace nf4gemm;

static uint8_t* fake(uintptr_t a) { return reinterpret_cast<uint8_t*>(a); }  // never dereferenced

// which: 0 the gate stack (blocksize2 256, one shared table), 1 the up stack (blocksize2 16, a
// table per expert, padded packed stride) -- the stacks need not agree in these
static nf4_moe_experts stack(bool single, int which, int32_t E, int64_t I, int64_t K) {
    const int64_t nblk = I * K / 64;
    const int32_t bs2 = which ? 16 : 256;
    nf4_moe_experts e{};
    e.packed = fake(0x2000 + 0x100000 * which);
    e.packed_stride = I * (K / 2) + 4096 * which;
    e.absmax_q = single ? nullptr : fake(0x3000);
    e.nb_stride = single ? 0 : nblk;
    e.code2 = single ? nullptr : reinterpret_cast<const float*>(fake(0x4000));
    e.code2_stride = single ? 0 : 256 * which;
    e.absmax2 = reinterpret_cast<const float*>(fake(0x5000));
    e.n2_stride = single ? nblk : (nblk + bs2 - 1) / bs2;
    e.offset = single ? nullptr : reinterpret_cast<const float*>(fake(0x7000));
    e.N = I;
    e.K = K;
    e.experts = E;
    e.single = single ? 1 : 0;
    e.blocksize = 64;
    e.blocksize2 = single ? 0 : bs2;
    return e;
}

struct Pair {
    nf4_moe_experts ex[2];
};
static Pair pair(bool single, int32_t E, int64_t I, int64_t K) { return Pair{{stack(single, 0, E, I, K), stack(single, 1, E, I, K)}}; }

static MsgCall good(const Pair* p, int64_t P) {
    MsgCall a{};
    a.x = fake(0x1000);
    a.ids = fake(0x8000);
    a.P = P;
    a.x_div = 2;
    a.ex = p->ex;
    a.act = NF4DQ_ACT_SILU;
    a.h = fake(0x6000);
    a.dtype = NF4DQ_BF16;
    a.workspace = fake(0x100000);
    a.workspace_bytes = size_t(1) << 31;
    a.cfg = nullptr;
    return a;
}

static void err(const char* name, const MsgCall& a) {
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = msg_check(a, 256, &c, &launch);
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d,\"launch\":%d}\n", name, rc, launch ? 1 : 0);
}

static void errors() {
    const int64_t P = 64, I = 128, K = 1024;
    const int32_t E = 8;
    char name[96];
    for (bool single : {false, true}) {
        const char* tag = single ? "s" : "n";
        Pair pr = pair(single, E, I, K);
        auto fresh = [&]() {
            pr = pair(single, E, I, K);
            return good(&pr, P);
        };
        auto put = [&](const char* what, const MsgCall& a) {
            snprintf(name, sizeof name, "%s_%s", what, tag);
            err(name, a);
        };
        MsgCall a = fresh();
        put("ok", a);
        a.dtype = NF4DQ_F32;
        put("arg_dtype", a);
        a = fresh(), a.act = 1;
        put("arg_act", a);
        a = fresh(), a.ex = nullptr;
        put("arg_null_stacks", a);
        a = fresh(), a.P = -1;
        put("arg_negative_p", a);
        a = fresh(), a.x = nullptr;
        put("arg_null_x", a);
        a = fresh(), a.ids = nullptr;
        put("arg_null_ids", a);
        a = fresh(), a.h = nullptr;
        put("arg_null_h", a);
        a = fresh(), a.x = fake(0x1008);
        put("arg_misaligned_x", a);
        a = fresh(), a.h = fake(0x6002);
        put("arg_misaligned_h", a);
        a = fresh(), a.ids = fake(0x8002);
        put("arg_misaligned_ids", a);
        a = fresh(), a.x_div = 0;
        put("arg_x_div_0", a);
        a = fresh(), a.P = 0;
        put("ok_p0_nothing", a);
        a = fresh(), a.P = 0, a.x = nullptr, a.h = nullptr, a.ids = nullptr;
        put("ok_p0_null_tensors", a);
        a = fresh(), a.P = 129;
        put("shape_p129", a);
        a = fresh(), a.P = 128;
        put("ok_p128", a);
        a = fresh(), a.P = 1;
        put("ok_p1", a);
        a = fresh(), a.x_div = 1000;
        put("ok_x_div_beyond_p", a);
        pr = pair(single, E, 96, K), a = good(&pr, P);
        put("shape_i96", a);
        pr = pair(single, E, I, 1088), a = good(&pr, P);
        put("shape_k1088", a);
        pr = pair(single, E, 0, K), a = good(&pr, P);
        put("shape_i0", a);
        pr = pair(single, E, int64_t(1) << 19, 128), a = good(&pr, P);
        put("too_large_i", a);
        // every per-stack rule on the gate stack (g) and on the up stack (u)
        for (int w = 0; w < 2; ++w) {
            auto putw = [&](const char* what, const MsgCall& c) {
                snprintf(name, sizeof name, "%s_%c_%s", what, w ? 'u' : 'g', tag);
                err(name, c);
            };
            a = fresh(), pr.ex[w].packed = nullptr;
            putw("arg_null_packed", a);
            a = fresh(), pr.ex[w].absmax2 = nullptr;
            putw("arg_null_stats", a);
            a = fresh(), pr.ex[w].packed = fake(0x2004);
            putw("arg_misaligned_packed", a);
            a = fresh(), pr.ex[w].packed_stride += 8;
            putw("arg_misaligned_packed_stride", a);
            a = fresh(), pr.ex[w].experts = 0;
            putw("arg_experts_0", a);
            a = fresh(), pr.ex[w].experts = 257;
            putw("arg_experts_257", a);
            a = fresh(), pr.ex[w].blocksize = 96;
            putw("arg_blocksize", a);
            a = fresh(), pr.ex[w].packed_stride = -16;
            putw("arg_negative_stride", a);
            a = fresh(), pr.ex[w].blocksize = 128;
            putw("shape_blocksize_128", a);
            a = fresh(), pr.ex[w].packed_stride = I * (K / 2) - 16;
            putw("shape_packed_stride", a);
            a = fresh(), pr.ex[w].packed_stride += 4096;
            putw("ok_padded_packed_stride", a);
            a = fresh(), pr.ex[w].n2_stride -= 1;
            putw("shape_short_stats", a);
            // the two-stack mismatches: this stack alone has the other value, consistent in itself
            a = fresh(), pr.ex[w] = stack(single, w, E, 192, K);
            putw("shape_stacks_differ_in_n", a);
            a = fresh(), pr.ex[w] = stack(single, w, E, I, 2048);
            putw("shape_stacks_differ_in_k", a);
            a = fresh(), pr.ex[w] = stack(single, w, 4, I, K);
            putw("shape_stacks_differ_in_experts", a);
            a = fresh(), pr.ex[w] = stack(!single, w, E, I, K);
            putw("shape_stacks_differ_in_single", a);
        }
        a = fresh(), pr.ex[0].experts = pr.ex[1].experts = 256;
        put("ok_experts_256", a);
        const nf4_gemm_cfg one{NF4DQ_GEMM_MOE_SWIGLU, 4, 1, 1, 2}, bad{NF4DQ_GEMM_MOE_SWIGLU, 4, 1, 9, 2}, k0{0, 2, 1, 8, 0};
        const nf4_gemm_cfg four{NF4DQ_GEMM_MOE_SWIGLU, 4, 1, 4, 2}, moe{NF4DQ_GEMM_MOE, 4, 1, 1, 2}, sg{NF4DQ_GEMM_MT_SWIGLU, 4, 1, 1, 2};
        a = fresh(), a.cfg = &four, a.workspace = nullptr;
        put("arg_no_workspace", a);
        a = fresh(), a.cfg = &four, a.workspace = fake(0x100008);
        put("arg_misaligned_workspace", a);
        a = fresh(), a.cfg = &four, a.workspace_bytes = kHeaderBytes + 4 * 2 * P * I * 4 - 1;
        put("arg_short_workspace", a);
        a = fresh(), a.cfg = &four, a.workspace_bytes = kHeaderBytes + 4 * 2 * P * I * 4;
        put("ok_exact_workspace", a);
        a = fresh(), a.cfg = &one, a.workspace = nullptr, a.workspace_bytes = 0;
        put("ok_one_slice_no_workspace", a);
        a = fresh(), a.cfg = &bad;
        put("arg_cfg_ksplit", a);
        a = fresh(), a.cfg = &moe;
        put("arg_cfg_expert_gemm", a);
        a = fresh(), a.cfg = &sg;
        put("arg_cfg_dense_swiglu", a);
        a = fresh(), a.cfg = &k0;
        put("ok_cfg_kernel_0", a);
        // 256 experts x 256 column tiles of 32: 65536 tickets, the header holds 16384
        const nf4_gemm_cfg two{NF4DQ_GEMM_MOE_SWIGLU, 2, 1, 2, 2}, narrow{NF4DQ_GEMM_MOE_SWIGLU, 2, 1, 1, 2};
        pr = pair(single, 256, 8192, 256), a = good(&pr, P), a.cfg = &two;
        put("too_large_tickets", a);
        pr = pair(single, 256, 8192, 256), a = good(&pr, P), a.cfg = &narrow;
        put("ok_one_slice_draws_no_ticket", a);
        // 16 slices x 2 planes x 128 pairs x 2^18 columns x 4 bytes = 2^32
        const nf4_gemm_cfg sixteen{NF4DQ_GEMM_MOE_SWIGLU, 4, 1, 16, 2}, eight{NF4DQ_GEMM_MOE_SWIGLU, 4, 1, 8, 2};
        pr = pair(single, 1, int64_t(1) << 18, 2048), a = good(&pr, 128), a.cfg = &sixteen, a.workspace_bytes = size_t(1) << 40;
        put("too_large_workspace", a);
        pr = pair(single, 1, int64_t(1) << 18, 2048), a = good(&pr, 128), a.cfg = &eight, a.workspace_bytes = size_t(1) << 40;
        put("ok_half_that_workspace", a);
    }
    Pair pr = pair(false, 8, I, K);
    MsgCall a = good(&pr, P);
    for (int w = 0; w < 2; ++w) {
        auto putw = [&](const char* what) {
            snprintf(name, sizeof name, "%s_%c", what, w ? 'u' : 'g');
            err(name, a);
        };
        pr = pair(false, 8, I, K), pr.ex[w].absmax_q = nullptr;
        putw("arg_null_a1");
        pr = pair(false, 8, I, K), pr.ex[w].code2 = nullptr;
        putw("arg_null_code2");
        pr = pair(false, 8, I, K), pr.ex[w].blocksize2 = 3;
        putw("arg_blocksize2");
        pr = pair(false, 8, I, K), pr.ex[w].offset = reinterpret_cast<const float*>(fake(0x7002));
        putw("arg_misaligned_offset");
        pr = pair(false, 8, I, K), pr.ex[w].nb_stride -= 1;
        putw("shape_short_nb");
        pr = pair(false, 8, I, K), pr.ex[w].code2_stride = 255;
        putw("shape_code2_stride");
        pr = pair(false, 8, I, K), pr.ex[w].code2_stride = 256;
        putw("ok_code2_stride");
        pr = pair(false, 8, I, K), pr.ex[w].offset = nullptr;
        putw("ok_null_offset");
    }
}

// The smallest workspace_bytes msg_check accepts: what the launcher needs.
static size_t launcher_need(MsgCall a, int cus) {
    nf4_gemm_cfg c{};
    bool launch = false;
    a.workspace_bytes = 0;
    if (msg_check(a, cus, &c, &launch) == NF4DQ_OK) return 0;
    size_t lo = 0, hi = size_t(1) << 33;  // lo rejected, hi accepted
    a.workspace_bytes = hi;
    if (msg_check(a, cus, &c, &launch) != NF4DQ_OK) return ~size_t(0);
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        a.workspace_bytes = mid;
        (msg_check(a, cus, &c, &launch) == NF4DQ_OK ? hi : lo) = mid;
    }
    return hi;
}

static void plan(int cus, int64_t P, int32_t E, int64_t I, int64_t K, const nf4_gemm_cfg* named) {
    const Pair pr = pair(false, E, I, K);
    MsgCall a = good(&pr, P);
    a.cfg = named;
    a.workspace_bytes = size_t(1) << 33;
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = msg_check(a, cus, &c, &launch);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%d,%lld,%lld],\"named\":%d,\"rc\":%d", cus, (long long)P, E, (long long)I,
           (long long)K, named ? 1 : 0, rc);
    if (named) printf(",\"asked\":[%d,%d,%d,%d,%d]", named->kernel, named->waves, named->depth, named->ksplit, named->strips);
    if (rc == NF4DQ_OK && launch) {
        const MoePlan p = msg_plan(c, P, E, I, K);
        printf(",\"cfg\":[%d,%d,%d,%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u,%u],\"need\":%zu,\"ws\":%zu", c.kernel, c.waves,
               c.depth, c.ksplit, c.strips, p.grid, p.block, p.dyn, p.tiles, p.chunks, p.cps, p.row_tiles, p.tickets,
               launcher_need(a, cus), msg_workspace_need(P, I, K, c));
    }
    printf("}\n");
}

int main() {
    errors();
    // Mixtral-8x7B: 8 experts, top-2; w1 / w3 14336x4096; 1, 4, 16 and 64 tokens
    for (int cus : {256, 64})
        for (int64_t P : {2, 8, 32, 128}) plan(cus, P, 8, 14336, 4096, nullptr);
    // the tests' small shapes and every cfg of the family over them
    const int64_t small[][3] = {{4, 192, 768}, {4, 192, 1152}, {2, 64, 256}, {2, 128, 640}, {2, 64, 384}, {8, 128, 4096}};
    for (const auto& s : small)
        for (int64_t P : {1, 2, 16, 17, 33, 100, 128}) {
            const int32_t E = (int32_t)s[0];
            plan(256, P, E, s[1], s[2], nullptr);
            int valid = 0;
            uint32_t lds_max = 0;
            for (int waves : {1, 2, 3, 4, 8})
                for (int depth : {1, 2})
                    for (int strips : {0, 1, 2, 4})
                        for (int ks = 0; ks <= 18; ++ks) {
                            const nf4_gemm_cfg c{NF4DQ_GEMM_MOE_SWIGLU, waves, depth, ks, strips};
                            if (!valid_msg_cfg(c, P, s[1], s[2])) continue;
                            ++valid;
                            const MoePlan p = msg_plan(c, P, E, s[1], s[2]);
                            lds_max = p.dyn > lds_max ? p.dyn : lds_max;
                            plan(256, P, E, s[1], s[2], &c);
                        }
            printf("{\"k\":\"cfgs\",\"c\":[256,%lld,%d,%lld,%lld],\"valid\":%d,\"lds_max\":%u}\n", (long long)P, E,
                   (long long)s[1], (long long)s[2], valid, lds_max);
        }
    return 0;
}
