// gemm_mt_swiglu_plan_check.cpp -- what the host plan of the fused gate/up SwiGLU launch
// (nf4_gemm_mt_swiglu_plan.h) decides, one compact JSON line each, integers only:
//   {"k":"err","name":..,"rc":..}     sg_check's status for a call built to break one rule
//   {"k":"plan","c":[cus,M,I,K],"named":0/1,"rc":..,"cfg":[kernel,waves,depth,ksplit,strips],
//    "geo":[grid,block,dyn,tiles,chunks,cps,row_tiles],"need":..,"ws":..}
//       the launch of the library's choice (named 0) or of a named cfg (named 1); need = what
//       the launcher checks the workspace against (found by bisecting sg_check's answer over
//       workspace_bytes), ws = sg_workspace_need, what the size entry answers
//   {"k":"cfgs","c":[cus,M,I,K],"valid":..,"lds_max":..}   over every cfg of the family's grid
// tests/test_gemm_mt_swiglu_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_mt_swiglu_plan.h"

using namespace nf4gemm;

static uint8_t* fake(uintptr_t a) { return reinterpret_cast<uint8_t*>(a); }  // never dereferenced

// A call and the two descriptors it points at (gate, up with different blocksize2).
struct Call {
    nf4_gemm_bnb_mat m[2];
    SgCall a;
    Call(const Call& o) { *this = o; }
    Call& operator=(const Call& o) {
        m[0] = o.m[0], m[1] = o.m[1], a = o.a, a.mats = m;
        return *this;
    }
    Call(bool single, int64_t M, int64_t I, int64_t K) {
        const int64_t nblk = I * K / 64;
        for (int i = 0; i < 2; ++i) {
            const int bs2 = i ? 64 : 256;
            m[i] = nf4_gemm_bnb_mat{};
            m[i].packed = fake(0x2000 + 0x10000 * i);
            m[i].packed_len = I * (K / 2);
            m[i].absmax_q = single ? nullptr : fake(0x3000);
            m[i].nb = single ? 0 : nblk;
            m[i].code2 = single ? nullptr : reinterpret_cast<const float*>(fake(0x4000));
            m[i].absmax2 = reinterpret_cast<const float*>(fake(0x5000));
            m[i].n2 = single ? nblk : (nblk + bs2 - 1) / bs2;
            m[i].offset = nullptr;
            m[i].blocksize = 64;
            m[i].blocksize2 = single ? 0 : bs2;
            m[i].y = nullptr;  // ignored
            m[i].N = I;
        }
        a = SgCall{single, fake(0x1000), M, K, m, NF4DQ_ACT_SILU, fake(0x6000), NF4DQ_BF16, fake(0x100000), size_t(1) << 31, nullptr};
    }
};

static void err(const char* name, const Call& c) {
    nf4_gemm_cfg out{};
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d}\n", name, sg_check(c.a, 256, &out));
}

static void errors() {
    const int64_t M = 64, I = 128, K = 1024;
    for (bool single : {false, true}) {
        const char* tag = single ? "s_" : "n_";
        char name[64];
        auto put = [&](const char* what, const Call& c) {
            snprintf(name, sizeof name, "%s%s", what, tag);
            err(name, c);
        };
        const Call good(single, M, I, K);
        Call c = good;
        put("ok_", c);
        c.a.dtype = NF4DQ_F32;
        put("arg_dtype_", c);
        c = good, c.a.act = 1;
        put("arg_act_", c);
        c = good, c.a.M = -1;
        put("arg_negative_m_", c);
        c = good, c.a.x = nullptr;
        put("arg_null_x_", c);
        c = good, c.a.h = nullptr;
        put("arg_null_h_", c);
        c = good, c.a.mats = nullptr;
        put("arg_null_mats_", c);
        c = good, c.a.x = fake(0x1008);
        put("arg_misaligned_x_", c);
        c = good, c.a.h = fake(0x6004);
        put("arg_misaligned_h_", c);
        for (int i = 0; i < 2; ++i) {  // every per-weight rule on the gate and on the up weight
            const char* wn = i ? "up_" : "gate_";
            auto putw = [&](const char* what, const Call& cc) {
                snprintf(name, sizeof name, "%s%s%s", what, wn, tag);
                err(name, cc);
            };
            c = good, c.m[i].packed = nullptr;
            putw("arg_null_packed_", c);
            c = good, c.m[i].absmax2 = nullptr;
            putw("arg_null_stats_", c);
            c = good, c.m[i].packed = fake(0x2008);
            putw("arg_misaligned_packed_", c);
            c = good, c.m[i].blocksize = 96;
            putw("arg_blocksize_", c);
            c = good, c.m[i].blocksize = 128, c.m[i].nb /= 2, c.m[i].n2 = single ? c.m[i].n2 / 2 : c.m[i].n2;
            putw("shape_blocksize_128_", c);
            c = good, c.m[i].N = I + 64;
            putw("shape_n_differ_", c);
            c = good, c.m[i].packed_len -= 1;
            putw("shape_packed_len_", c);
            c = good, c.m[i].n2 -= 1;
            putw("shape_short_stats_", c);
        }
        c = Call(single, 0, I, K);
        put("shape_m0_", c);
        c = Call(single, 129, I, K);
        put("shape_m129_", c);
        c = Call(single, 128, I, K);
        put("ok_m128_", c);
        c = Call(single, 1, I, K);
        put("ok_m1_", c);
        c = Call(single, M, 96, K);
        put("shape_i96_", c);
        c = Call(single, M, 0, K);
        put("shape_i0_", c);
        c = Call(single, M, I, 1088);
        put("shape_k1088_", c);
        c = Call(single, M, I, 64);
        put("shape_k64_", c);
        c = Call(single, M, int64_t(1) << 19, 128);
        put("too_large_i_", c);
        c = Call(single, 128, int64_t(1) << 18, 16384);  // packed_len 2^31
        put("too_large_packed_", c);
        const nf4_gemm_cfg one{NF4DQ_GEMM_MT_SWIGLU, 4, 1, 1, 2}, bad{NF4DQ_GEMM_MT_SWIGLU, 4, 1, 9, 2}, k0{0, 2, 1, 8, 0};
        const nf4_gemm_cfg four{NF4DQ_GEMM_MT_SWIGLU, 4, 1, 4, 2}, mt{NF4DQ_GEMM_MT, 4, 1, 1, 2};
        c = good, c.a.cfg = &four, c.a.workspace = nullptr;
        put("arg_no_workspace_", c);
        c = good, c.a.cfg = &four, c.a.workspace = fake(0x100008);
        put("arg_misaligned_workspace_", c);
        c = good, c.a.cfg = &four, c.a.workspace_bytes = kHeaderBytes + 4 * 2 * M * I * 4 - 1;
        put("arg_short_workspace_", c);
        c = good, c.a.cfg = &four, c.a.workspace_bytes = kHeaderBytes + 4 * 2 * M * I * 4;
        put("ok_exact_workspace_", c);
        c = good, c.a.cfg = &one, c.a.workspace = nullptr, c.a.workspace_bytes = 0;
        put("ok_one_slice_no_workspace_", c);
        c = good, c.a.cfg = &bad;
        put("arg_cfg_ksplit_", c);
        c = good, c.a.cfg = &mt;
        put("arg_cfg_parent_family_", c);
        c = good, c.a.cfg = &k0;
        put("ok_cfg_kernel_0_", c);
        // 16 slices of two planes of 128 x 2^18 floats: 2^32 bytes and the header
        const nf4_gemm_cfg wide{NF4DQ_GEMM_MT_SWIGLU, 4, 1, 16, 2};
        c = Call(single, 128, int64_t(1) << 18, 2048), c.a.cfg = &wide, c.a.workspace_bytes = size_t(1) << 40;
        put("too_large_workspace_", c);
    }
    const Call good(false, M, I, K);
    for (int i = 0; i < 2; ++i) {
        char name[64];
        Call c = good;
        c.m[i].absmax_q = nullptr;
        snprintf(name, sizeof name, "arg_null_a1_%d", i), err(name, c);
        c = good, c.m[i].code2 = nullptr;
        snprintf(name, sizeof name, "arg_null_code2_%d", i), err(name, c);
        c = good, c.m[i].blocksize2 = 3;
        snprintf(name, sizeof name, "arg_blocksize2_%d", i), err(name, c);
        c = good, c.m[i].nb -= 1;
        snprintf(name, sizeof name, "shape_short_nb_%d", i), err(name, c);
    }
}

// The smallest workspace_bytes sg_check accepts: what the launcher needs.
static size_t launcher_need(Call c, int cus) {
    nf4_gemm_cfg out{};
    c.a.workspace_bytes = 0;
    if (sg_check(c.a, cus, &out) == NF4DQ_OK) return 0;
    size_t lo = 0, hi = size_t(1) << 33;  // lo rejected, hi accepted
    c.a.workspace_bytes = hi;
    if (sg_check(c.a, cus, &out) != NF4DQ_OK) return ~size_t(0);
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        c.a.workspace_bytes = mid;
        (sg_check(c.a, cus, &out) == NF4DQ_OK ? hi : lo) = mid;
    }
    return hi;
}

static void plan(int cus, int64_t M, int64_t I, int64_t K, const nf4_gemm_cfg* named) {
    Call c(false, M, I, K);
    c.a.cfg = named;
    c.a.workspace_bytes = size_t(1) << 33;
    nf4_gemm_cfg out{};
    const int rc = sg_check(c.a, cus, &out);
    printf("{\"k\":\"plan\",\"c\":[%d,%lld,%lld,%lld],\"named\":%d,\"rc\":%d", cus, (long long)M, (long long)I,
           (long long)K, named ? 1 : 0, rc);
    if (rc == NF4DQ_OK) {
        const MtPlan p = sg_plan(out, M, I, K);
        printf(",\"cfg\":[%d,%d,%d,%d,%d],\"geo\":[%u,%u,%u,%u,%u,%u,%u],\"need\":%zu,\"ws\":%zu", out.kernel, out.waves,
               out.depth, out.ksplit, out.strips, p.grid, p.block, p.dyn, p.tiles, p.chunks, p.cps, p.row_tiles,
               launcher_need(c, cus), sg_workspace_need(M, I, K, out));
    }
    printf("}\n");
}

int main() {
    errors();
    // the MLP shapes [I, K] of Llama-3-8B and Llama-2-7B, and two small-I ones where K slices fit the CUs
    const int64_t shapes[][2] = {{14336, 4096}, {11008, 4096}, {4096, 4096}, {1024, 8192}};
    for (int cus : {256, 64})
        for (const auto& s : shapes)
            for (int64_t M : {1, 33, 64, 128}) plan(cus, M, s[0], s[1], nullptr);
    // the tests' small shapes and every cfg of the family over them
    const int64_t small[][2] = {{64, 128}, {128, 256}, {192, 1152}, {64, 4096}, {192, 768}, {256, 1024}};
    for (const auto& s : small)
        for (int64_t M : {1, 16, 17, 33, 100, 128}) {
            plan(256, M, s[0], s[1], nullptr);
            int valid = 0;
            uint32_t lds_max = 0;
            for (int waves : {1, 2, 3, 4, 8})
                for (int depth : {1, 2})
                    for (int strips : {0, 1, 2, 4})
                        for (int ks = 0; ks <= 18; ++ks) {
                            const nf4_gemm_cfg c{NF4DQ_GEMM_MT_SWIGLU, waves, depth, ks, strips};
                            if (!valid_sg_cfg(c, M, s[0], s[1])) continue;
                            ++valid;
                            const MtPlan p = sg_plan(c, M, s[0], s[1]);
                            lds_max = p.dyn > lds_max ? p.dyn : lds_max;
                            plan(256, M, s[0], s[1], &c);
                        }
            printf("{\"k\":\"cfgs\",\"c\":[256,%lld,%lld,%lld],\"valid\":%d,\"lds_max\":%u}\n", (long long)M,
                   (long long)s[0], (long long)s[1], valid, lds_max);
        }
    return 0;
}
