// gemm_mt_plan_check.cpp -- what the row-tiled fused GEMM's host plan (nf4_gemm_mt_plan.h)
// decides, one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..}     mt_check's status for a call built to break one rule
//   {"k":"plan","c":[cus,M,N,K],"named":0/1,"rc":..,"cfg":[kernel,waves,depth,ksplit,strips],
//    "geo":[grid,block,dyn,tiles,chunks,cps,row_tiles],"need":..,"ws":..}
//       the launch of the library's choice (named 0) or of a named cfg (named 1); need = what
//       the launcher checks the workspace against (found by bisecting mt_check's answer over
//       workspace_bytes), ws = mt_workspace_need, what the size entry answers
//   {"k":"cfgs","c":[cus,M,N,K],"valid":..,"lds_max":..}   over every cfg of the family's grid
// tests/test_gemm_mt_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_mt_plan.h"

using namespace nf4gemm;

static uint8_t* fake(uintptr_t a) { return reinterpret_cast<uint8_t*>(a); }  // never dereferenced

static MtCall good(bool single, int64_t M, int64_t N, int64_t K) {
    const int64_t nblk = N * K / 64;
    MtCall a{};
    a.single = single;
    a.x = fake(0x1000);
    a.M = M;
    a.packed = fake(0x2000);
    a.packed_len = N * (K / 2);
    a.a1 = single ? nullptr : fake(0x3000);
    a.nb = nblk;
    a.code2 = single ? nullptr : reinterpret_cast<const float*>(fake(0x4000));
    a.a2 = reinterpret_cast<const float*>(fake(0x5000));
    a.n2 = single ? nblk : (nblk + 255) / 256;
    a.blocksize = 64;
    a.blocksize2 = single ? 1 : 256;
    a.y = fake(0x6000);
    a.dtype = NF4DQ_BF16;
    a.N = N;
    a.K = K;
    a.workspace = fake(0x100000);
    a.workspace_bytes = size_t(1) << 31;
    a.cfg = nullptr;
    return a;
}

static void err(const char* name, const MtCall& a) {
    nf4_gemm_cfg c{};
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d}\n", name, mt_check(a, 256, &c));
}

static void errors() {
    const int64_t M = 64, N = 128, K = 1024;
    for (bool single : {false, true}) {
        const char* tag = single ? "s_" : "n_";
        char name[64];
        auto put = [&](const char* what, const MtCall& a) {
            snprintf(name, sizeof name, "%s%s", what, tag);
            err(name, a);
        };
        MtCall a = good(single, M, N, K);
        put("ok_", a);
        a.dtype = NF4DQ_F32;
        put("arg_dtype_", a);
        a = good(single, M, N, K), a.M = -1;
        put("arg_negative_m_", a);
        a = good(single, M, N, K), a.x = nullptr;
        put("arg_null_x_", a);
        a = good(single, M, N, K), a.packed = nullptr;
        put("arg_null_packed_", a);
        a = good(single, M, N, K), a.a2 = nullptr;
        put("arg_null_stats_", a);
        a = good(single, M, N, K), a.y = nullptr;
        put("arg_null_y_", a);
        a = good(single, M, N, K), a.x = fake(0x1008);
        put("arg_misaligned_x_", a);
        a = good(single, M, N, K), a.blocksize = 96;
        put("arg_blocksize_", a);
        a = good(single, M, N, K), a.blocksize = 128, a.nb /= 2, a.n2 = single ? a.nb : a.n2;
        put("shape_blocksize_128_", a);
        a = good(single, M, N, K), a.M = 0;
        put("shape_m0_", a);
        a = good(single, M, N, K), a.M = 129;
        put("shape_m129_", a);
        a = good(single, 128, N, K);
        put("ok_m128_", a);
        a = good(single, 1, N, K);
        put("ok_m1_", a);
        a = good(single, M, 96, K);
        put("shape_n96_", a);
        a = good(single, M, N, 1088);
        put("shape_k1088_", a);
        a = good(single, M, N, K), a.packed_len -= 1;
        put("shape_packed_len_", a);
        a = good(single, M, N, K), a.n2 -= 1;
        put("shape_short_stats_", a);
        a = good(single, M, int64_t(1) << 19, 128);
        put("too_large_n_", a);
        const nf4_gemm_cfg one{NF4DQ_GEMM_MT, 4, 1, 1, 2}, bad{NF4DQ_GEMM_MT, 4, 1, 9, 2}, k0{0, 2, 1, 8, 0};
        const nf4_gemm_cfg four{NF4DQ_GEMM_MT, 4, 1, 4, 2};
        a = good(single, M, N, K), a.cfg = &four, a.workspace = nullptr;
        put("arg_no_workspace_", a);
        a = good(single, M, N, K), a.cfg = &four, a.workspace = fake(0x100008);
        put("arg_misaligned_workspace_", a);
        a = good(single, M, N, K), a.cfg = &four, a.workspace_bytes = kHeaderBytes + 4 * M * N * 4 - 1;
        put("arg_short_workspace_", a);
        a = good(single, M, N, K), a.cfg = &four, a.workspace_bytes = kHeaderBytes + 4 * M * N * 4;
        put("ok_exact_workspace_", a);
        a = good(single, M, N, K), a.cfg = &one, a.workspace = nullptr, a.workspace_bytes = 0;
        put("ok_one_slice_no_workspace_", a);
        a = good(single, M, N, K), a.cfg = &bad;
        put("arg_cfg_ksplit_", a);
        a = good(single, M, N, K), a.cfg = &k0;
        put("ok_cfg_kernel_0_", a);
    }
    MtCall a = good(false, M, N, K);
    a.a1 = nullptr;
    err("arg_null_a1", a);
    a = good(false, M, N, K), a.code2 = nullptr;
    err("arg_null_code2", a);
    a = good(false, M, N, K), a.blocksize2 = 3;
    err("arg_blocksize2", a);
    a = good(false, M, N, K), a.nb -= 1;
    err("shape_short_nb", a);
}

// The smallest workspace_bytes mt_check accepts: what the launcher needs.
static size_t launcher_need(MtCall a, int cus) {
    nf4_gemm_cfg c{};
    a.workspace_bytes = 0;
    if (mt_check(a, cus, &c) == NF4DQ_OK) return 0;
    size_t lo = 0, hi = size_t(1) << 33;  // lo rejected, hi accepted
    a.workspace_bytes = hi;
    if (mt_check(a, cus, &c) != NF4DQ_OK) return ~size_t(0);
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        a.workspace_bytes = mid;
        (mt_check(a, cus, &c) == NF4DQ_OK ? hi : lo) = mid;
    }
    return hi;
}

static void plan(int cus, int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* named) {
    MtCall a = good(false, M, N, K);
    a.cfg = named;
    a.workspace_bytes = size_t(1) << 33;
    nf4_gemm_cfg c{};
    const int rc = mt_check(a, cus, &c);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%lld,%lld],\"named\":%d,\"rc\":%d", cus, (long long)M, (long long)N,
           (long long)K, named ? 1 : 0, rc);
    if (rc == NF4DQ_OK) {
        const MtPlan p = mt_plan(c, M, N, K);
        printf(",\"cfg\":[%d,%d,%d,%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u],\"need\":%zu,\"ws\":%zu", c.kernel, c.waves,
               c.depth, c.ksplit, c.strips, p.grid, p.block, p.dyn, p.tiles, p.chunks, p.cps, p.row_tiles,
               launcher_need(a, cus), mt_workspace_need(M, N, K, c));
    }
    printf("}\n");
}

int main() {
    errors();
    // the Llama-3-8B shapes [N, K]: 4096^2, gate/up 14336x4096, down 4096x14336, grouped q/k/v and gate/up
    const int64_t shapes[][2] = {{4096, 4096}, {14336, 4096}, {4096, 14336}, {6144, 4096}, {28672, 4096}};
    for (int cus : {256, 64})
        for (const auto& s : shapes)
            for (int64_t M : {33, 64, 128}) plan(cus, M, s[0], s[1], nullptr);
    // the tests' small shapes and every cfg of the family over them
    const int64_t small[][2] = {{192, 768}, {64, 128}, {64, 384}, {64, 4096}, {128, 256}, {256, 1024}};
    for (const auto& s : small)
        for (int64_t M : {1, 16, 17, 33, 100, 128}) {
            plan(256, M, s[0], s[1], nullptr);
            int valid = 0;
            uint32_t lds_max = 0;
            for (int waves : {1, 2, 3, 4, 8})
                for (int depth : {1, 2})
                    for (int strips : {0, 1, 2, 4})
                        for (int ks = 0; ks <= 18; ++ks) {
                            const nf4_gemm_cfg c{NF4DQ_GEMM_MT, waves, depth, ks, strips};
                            if (!valid_mt_cfg(c, M, s[0], s[1])) continue;
                            ++valid;
                            const MtPlan p = mt_plan(c, M, s[0], s[1]);
                            lds_max = p.dyn > lds_max ? p.dyn : lds_max;
                            plan(256, M, s[0], s[1], &c);
                        }
            printf("{\"k\":\"cfgs\",\"c\":[256,%lld,%lld,%lld],\"valid\":%d,\"lds_max\":%u}\n", (long long)M,
                   (long long)s[0], (long long)s[1], valid, lds_max);
        }
    return 0;
}
