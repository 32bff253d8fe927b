// gemm_moe_rb_plan_check.cpp -- what the host plan of the expert GEMM in row blocks
// (nf4_gemm_moe_rb_plan.h) decides, one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..,"launch":0/1}   moe_rb_check's status for a call built to break one rule
//   {"k":"plan","c":[cus,P,E,N,K],"named":0/1,"rc":..,"cfg":[kernel,waves,depth,ksplit,strips],
//    "geo":[grid,block,dyn,tiles,chunks,cps,row_tiles,tickets,row_blocks],"lds":..,"need":..,"ws":..}
//       the launch of the library's choice (named 0) or of a named cfg (named 1); lds =
//       moe_lds_bytes(min(P, 128)), the expert GEMM's own; need = what the launcher checks the
//       workspace against (found by bisecting moe_rb_check's answer over workspace_bytes), ws =
//       moe_rb_workspace_need, what the size entry answers
//   {"k":"cfgs","c":[cus,P,E,N,K],"valid":..,"lds_max":..}   over every cfg of the family's grid
// tests/test_gemm_moe_rb_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_moe_rb_plan.h"

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

static MoeCall good(const nf4_moe_experts* e, int64_t P) {
    MoeCall a{};
    a.x = fake(0x1000);
    a.ids = fake(0x8000);
    a.P = P;
    a.x_div = 2;
    a.ex = e;
    a.y = fake(0x6000);
    a.dtype = NF4DQ_BF16;
    a.workspace = fake(0x100000);
    a.workspace_bytes = size_t(1) << 31;
    a.cfg = nullptr;
    return a;
}

static void err(const char* name, const MoeCall& a) {
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_rb_check(a, 256, &c, &launch);
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d,\"launch\":%d}\n", name, rc, launch ? 1 : 0);
}

// nf4_gemm_bnb_moe's rules in its order (gemm_moe_plan_check.cpp), at 300 pairs: three row blocks.
static void errors() {
    const int64_t P = 300, N = 128, K = 1024;
    const int32_t E = 8;
    for (bool single : {false, true}) {
        const char* tag = single ? "s_" : "n_";
        char name[64];
        nf4_moe_experts e = stack(single, E, N, K);
        auto fresh = [&]() {
            e = stack(single, E, N, K);
            return good(&e, P);
        };
        auto put = [&](const char* what, const MoeCall& a) {
            snprintf(name, sizeof name, "%s%s", what, tag);
            err(name, a);
        };
        MoeCall a = fresh();
        put("ok_", a);
        a.dtype = NF4DQ_F32;
        put("arg_dtype_", a);
        a = fresh(), a.ex = nullptr;
        put("arg_null_experts_", a);
        a = fresh(), a.P = -1;
        put("arg_negative_p_", a);
        a = fresh(), a.x = nullptr;
        put("arg_null_x_", a);
        a = fresh(), a.ids = nullptr;
        put("arg_null_ids_", a);
        a = fresh(), e.packed = nullptr;
        put("arg_null_packed_", a);
        a = fresh(), e.absmax2 = nullptr;
        put("arg_null_stats_", a);
        a = fresh(), a.y = nullptr;
        put("arg_null_y_", a);
        a = fresh(), a.x = fake(0x1008);
        put("arg_misaligned_x_", a);
        a = fresh(), e.packed = fake(0x2004);
        put("arg_misaligned_packed_", a);
        a = fresh(), e.packed_stride += 8;
        put("arg_misaligned_packed_stride_", a);
        a = fresh(), a.y = fake(0x6002);
        put("arg_misaligned_y_", a);
        a = fresh(), a.ids = fake(0x8002);
        put("arg_misaligned_ids_", a);
        a = fresh(), a.x_div = 0;
        put("arg_x_div_0_", a);
        a = fresh(), e.experts = 0;
        put("arg_experts_0_", a);
        a = fresh(), e.experts = 257;
        put("arg_experts_257_", a);
        a = fresh(), e.experts = 256;
        put("ok_experts_256_", a);
        a = fresh(), e.blocksize = 96;
        put("arg_blocksize_", a);
        a = fresh(), e.packed_stride = -16;
        put("arg_negative_stride_", a);
        a = fresh(), e.blocksize = 128;
        put("shape_blocksize_128_", a);
        a = fresh(), a.P = 0;
        put("ok_p0_nothing_", a);
        a = fresh(), a.P = 0, a.x = nullptr, a.y = nullptr, a.ids = nullptr;
        put("ok_p0_null_tensors_", a);
        a = fresh(), a.P = 1025;
        put("shape_p1025_", a);
        a = fresh(), a.P = 1024;
        put("ok_p1024_", a);
        a = fresh(), a.P = 129;
        put("ok_p129_", a);
        a = fresh(), a.P = 128;
        put("ok_p128_", a);
        a = fresh(), a.P = 1;
        put("ok_p1_", a);
        a = fresh(), a.x_div = 5000;
        put("ok_x_div_beyond_p_", a);
        e = stack(single, E, 96, K), a = good(&e, P);
        put("shape_n96_", a);
        e = stack(single, E, N, 1088), a = good(&e, P);
        put("shape_k1088_", a);
        e = stack(single, E, 0, K), a = good(&e, P);
        put("shape_n0_", a);
        a = fresh(), e.packed_stride -= 16;
        put("shape_packed_stride_", a);
        a = fresh(), e.packed_stride += 4096;
        put("ok_padded_packed_stride_", a);
        a = fresh(), e.n2_stride -= 1;
        put("shape_short_stats_", a);
        e = stack(single, E, int64_t(1) << 19, 128), a = good(&e, P);
        put("too_large_n_", a);
        // x is indexed with 32 bits: P * K * 2 bytes below 2^31 for the P of THIS call
        e = stack(single, E, 64, int64_t(1) << 20), a = good(&e, 1024);
        put("too_large_x_", a);
        e = stack(single, E, 64, int64_t(1) << 20), a = good(&e, 1023);
        put("ok_x_below_2g_", a);
        const nf4_gemm_cfg one{NF4DQ_GEMM_MOE_RB, 4, 1, 1, 2}, bad{NF4DQ_GEMM_MOE_RB, 4, 1, 9, 2}, k0{0, 2, 1, 8, 0};
        const nf4_gemm_cfg four{NF4DQ_GEMM_MOE_RB, 4, 1, 4, 2}, mt{NF4DQ_GEMM_MT, 4, 1, 1, 2}, moe{NF4DQ_GEMM_MOE, 4, 1, 1, 2};
        a = fresh(), a.cfg = &four, a.workspace = nullptr;
        put("arg_no_workspace_", a);
        a = fresh(), a.cfg = &four, a.workspace = fake(0x100008);
        put("arg_misaligned_workspace_", a);
        a = fresh(), a.cfg = &four, a.workspace_bytes = kHeaderBytes + 4 * P * N * 4 - 1;
        put("arg_short_workspace_", a);
        a = fresh(), a.cfg = &four, a.workspace_bytes = kHeaderBytes + 4 * P * N * 4;
        put("ok_exact_workspace_", a);
        a = fresh(), a.cfg = &one, a.workspace = nullptr, a.workspace_bytes = 0;
        put("ok_one_slice_no_workspace_", a);
        a = fresh(), a.cfg = &bad;
        put("arg_cfg_ksplit_", a);
        a = fresh(), a.cfg = &mt;
        put("arg_cfg_other_family_", a);
        a = fresh(), a.cfg = &moe;
        put("arg_cfg_moe_", a);
        a = fresh(), a.P = 64, a.cfg = &moe;  // ... within nf4_gemm_bnb_moe's own domain too
        put("arg_cfg_moe_64_pairs_", a);
        a = fresh(), a.cfg = &k0;
        put("ok_cfg_kernel_0_", a);
        // 256 experts x 16 column tiles of 64 x 3 row blocks = 12288 tickets fit the header's 16384;
        // 5 row blocks (20480) do not; nf4_gemm_bnb_moe's own case, 256 x 128 tiles, at one block
        const nf4_gemm_cfg two{NF4DQ_GEMM_MOE_RB, 2, 1, 2, 2}, narrow{NF4DQ_GEMM_MOE_RB, 2, 1, 1, 2};
        e = stack(single, 256, 1024, 256), a = good(&e, 300), a.cfg = &two;
        put("ok_tickets_3_blocks_", a);
        e = stack(single, 256, 1024, 256), a = good(&e, 513), a.cfg = &two;
        put("too_large_tickets_5_blocks_", a);
        e = stack(single, 256, 1024, 256), a = good(&e, 513), a.cfg = &narrow;
        put("ok_one_slice_draws_no_ticket_", a);
        e = stack(single, 256, 8192, 256), a = good(&e, 64), a.cfg = &two;
        put("too_large_tickets_1_block_", a);
        // the slab: ksplit * P * N floats below 2^32 bytes -- 16 x 1024 x 65536 x 4 = 2^32
        const nf4_gemm_cfg sixteen{NF4DQ_GEMM_MOE_RB, 4, 1, 16, 2}, fifteen{NF4DQ_GEMM_MOE_RB, 4, 1, 15, 2};
        e = stack(single, 1, 65536, 2048), a = good(&e, 1024), a.cfg = &sixteen, a.workspace_bytes = size_t(1) << 33;
        put("too_large_slab_", a);
        e = stack(single, 1, 65536, 2048), a = good(&e, 1024), a.cfg = &fifteen, a.workspace_bytes = size_t(1) << 33;
        put("ok_slab_below_4g_", a);
    }
    nf4_moe_experts e = stack(false, 8, N, K);
    MoeCall a = good(&e, P);
    e.absmax_q = nullptr;
    err("arg_null_a1", a);
    e = stack(false, 8, N, K), e.code2 = nullptr;
    err("arg_null_code2", a);
    e = stack(false, 8, N, K), e.blocksize2 = 3;
    err("arg_blocksize2", a);
    e = stack(false, 8, N, K), e.nb_stride -= 1;
    err("shape_short_nb", a);
    e = stack(false, 8, N, K), e.code2_stride = 255;
    err("shape_code2_stride", a);
    e = stack(false, 8, N, K), e.code2_stride = 256;
    err("ok_code2_stride", a);
    e = stack(false, 8, N, K), e.offset = nullptr;
    err("ok_null_offset", a);
}

// The smallest workspace_bytes moe_rb_check accepts: what the launcher needs.
static size_t launcher_need(MoeCall a, int cus) {
    nf4_gemm_cfg c{};
    bool launch = false;
    a.workspace_bytes = 0;
    if (moe_rb_check(a, cus, &c, &launch) == NF4DQ_OK) return 0;
    size_t lo = 0, hi = size_t(1) << 33;  // lo rejected, hi accepted
    a.workspace_bytes = hi;
    if (moe_rb_check(a, cus, &c, &launch) != NF4DQ_OK) return ~size_t(0);
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        a.workspace_bytes = mid;
        (moe_rb_check(a, cus, &c, &launch) == NF4DQ_OK ? hi : lo) = mid;
    }
    return hi;
}

static void plan(int cus, int64_t P, int32_t E, int64_t N, int64_t K, const nf4_gemm_cfg* named) {
    const nf4_moe_experts e = stack(false, E, N, K);
    MoeCall a = good(&e, P);
    a.cfg = named;
    a.workspace_bytes = size_t(1) << 33;
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_rb_check(a, cus, &c, &launch);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%d,%lld,%lld],\"named\":%d,\"rc\":%d", cus, (long long)P, E, (long long)N,
           (long long)K, named ? 1 : 0, rc);
    if (rc == NF4DQ_OK && launch) {
        const MoeRbPlan p = moe_rb_plan(c, P, E, N, K);
        printf(",\"cfg\":[%d,%d,%d,%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u,%u,%u],\"lds\":%u,\"need\":%zu,\"ws\":%zu", c.kernel,
               c.waves, c.depth, c.ksplit, c.strips, p.grid, p.block, p.dyn, p.tiles, p.chunks, p.cps, p.row_tiles, p.tickets,
               p.row_blocks, moe_lds_bytes(P < 128 ? P : 128), launcher_need(a, cus), moe_rb_workspace_need(P, N, K, c));
    }
    printf("}\n");
}

int main() {
    errors();
    // Mixtral-8x7B: 8 experts, top-2; w1 / w3 14336x4096, w2 4096x14336; 128, 256 and 512 tokens
    // (and 65 tokens, the first count past nf4_gemm_bnb_moe, and that entry's own 2 .. 128 pairs)
    const int64_t shapes[][2] = {{14336, 4096}, {4096, 14336}};
    for (int cus : {256, 64})
        for (const auto& s : shapes)
            for (int64_t P : {2, 8, 32, 128, 130, 256, 512, 1024}) plan(cus, P, 8, s[0], s[1], nullptr);
    // a stack of 256 experts at top-8, and a chip large enough that the rule does split K
    for (int64_t P : {256, 1024}) plan(256, P, 256, 1024, 4096, nullptr);
    for (int64_t P : {130, 256, 512, 1024}) plan(4096, P, 8, 4096, 14336, nullptr);
    // the tests' small shapes and every cfg of the family over them
    const int64_t small[][3] = {{4, 64, 256}, {4, 128, 256}, {256, 64, 256}, {4, 192, 768}, {2, 64, 4096}};
    for (const auto& s : small)
        for (int64_t P : {1, 100, 128, 129, 130, 256, 257, 300, 1024}) {
            const int32_t E = (int32_t)s[0];
            plan(256, P, E, s[1], s[2], nullptr);
            int valid = 0;
            uint32_t lds_max = 0;
            for (int waves : {1, 2, 3, 4, 8})
                for (int depth : {1, 2})
                    for (int strips : {0, 1, 2, 4})
                        for (int ks = 0; ks <= 18; ++ks) {
                            const nf4_gemm_cfg c{NF4DQ_GEMM_MOE_RB, waves, depth, ks, strips};
                            if (!valid_moe_rb_cfg(c, P, s[1], s[2])) continue;
                            ++valid;
                            const MoeRbPlan p = moe_rb_plan(c, P, E, s[1], s[2]);
                            lds_max = p.dyn > lds_max ? p.dyn : lds_max;
                            plan(256, P, E, s[1], s[2], &c);
                        }
            printf("{\"k\":\"cfgs\",\"c\":[256,%lld,%d,%lld,%lld],\"valid\":%d,\"lds_max\":%u}\n", (long long)P, E,
                   (long long)s[1], (long long)s[2], valid, lds_max);
        }
    return 0;
}
