// gemm_bnb_grouped_plan_check.cpp -- what the fused GEMM's host plan (nf4_gemm_plan.h) decides
// for nf4_gemm_bnb_grouped, over groups of weights that share x, one compact JSON line each,
// integers only:
//   c      the case: [cus, M, K, sh, group]   (sh = log2(blocksize / 64) of every weight;
//          group 0 = q/k/v (4096, 1024, 1024), 1 = gate/up (14336, 14336), 2 = (64, 192, 64))
//   ref    the launch the reference grouped plan runs for the group: [kernel, waves, depth,
//          ksplit, strips]; refpw: 1 if that plan falls back to per-weight launches
//   first  what the reference plan chose before the decode GEMV (default_gemm_cfg of the total)
//   bnb    the launch bnb_grouped_choice runs, nested mode; bnbs: single mode; pw / pws: their
//          per-weight fallback flags
//   v      bnb / bnbs valid for every weight, accepted by the entry (bnb_grouped_cfg_ok) and able
//          to run (cfg_runs), or a per-weight fallback whose every launch is
//   need   the most either call checks the workspace against, the per-weight fallback's launches
//          included;  ws  the size entry's answer without a cfg
//   shape  grid, block, dynamic LDS of the nested launch, of the single one, and of the
//          reference-mode launch of the same cfg;  lds  static + dynamic LDS of the nested launch;
//          tables  the code2 tables the nested launch adds to the dynamic LDS
// and one first line {"mat": [sizeof, offsetof ...]} of nf4_gemm_bnb_mat.
// tests/test_gemm_bnb_grouped_plan_cpu.py builds this for the host (no GPU, no HIP) and checks
// the lines.
#include <stddef.h>
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_plan.h"

using namespace nf4gemm;

static void put(const char* key, const nf4_gemm_cfg& c) {
    printf(",\"%s\":[%d,%d,%d,%d,%d]", key, c.kernel, c.waves, c.depth, c.ksplit, c.strips);
}

static uint32_t static_lds(const nf4_gemm_cfg& c, int mode, int64_t M) {
    if (c.kernel == NF4DQ_GEMM_PERSIST) return kStreamStatic;
    if (c.kernel == NF4DQ_GEMM_XR) return xr_lds_static(c.strips, mode);
    // 128-deep: the 16 codes + flag, the code2 table, the waves' partial tiles [waves][row tiles][64] x 16 B
    return 80u + 1024u + (uint32_t)c.waves * (M > 16 ? 2u : 1u) * 1024u;
}

struct NMat {
    int64_t N;
};

static void run_case(int cus, int64_t M, int64_t K, int sh, int group, const std::vector<int64_t>& Ns) {
    static uint8_t dummy[16];  // the plan never reads through the pointers
    const int count = (int)Ns.size();
    std::vector<HostMat> ref, nested, single;
    std::vector<NMat> nm;
    int64_t ntot = 0;
    for (int64_t N : Ns) {
        const int64_t nb = N * (K / 64), n2 = N * ((K / 64 + 3) / 4);
        HostMat r{dummy, N * (K / 2), dummy, nb, reinterpret_cast<const float*>(dummy), n2, dummy, N};
        HostMat n = r, s = r;
        n.mode = kScaleBnb;
        n.code2 = n.offset = reinterpret_cast<const float*>(dummy);
        n.sh = sh;
        n.sh2 = 8;
        n.nb = (N * K) >> (6 + sh);
        n.n2 = (n.nb + 255) / 256;
        s.mode = kScaleBnbSingle;
        s.a1 = nullptr;
        s.sh = sh;
        s.nb = s.n2 = n.nb;
        ref.push_back(r);
        nested.push_back(n);
        single.push_back(s);
        nm.push_back(NMat{N});
        ntot += N;
    }
    const Choice rc = library_choice(M, K, ref.data(), count, cus);
    const Choice bn = bnb_grouped_choice(M, K, nested.data(), count, cus);
    const Choice bs = bnb_grouped_choice(M, K, single.data(), count, cus);
    size_t need = 0;
    auto check = [&](const Choice& ch, const std::vector<HostMat>& h) {
        size_t w = workspace_need(M, ntot, K, ch.first);
        need = w > need ? w : need;
        if (!ch.per_weight) {
            bool ok = bnb_grouped_cfg_ok(ch.cfg, h.data(), count) && cfg_runs(ch.cfg, M, K, h.data(), count, cus) == NF4DQ_OK;
            for (int i = 0; i < count; ++i) ok = ok && valid_gemm_cfg(ch.cfg, M, h[i].N, K);
            return ok;
        }
        bool ok = true;
        for (int i = 0; i < count; ++i) {
            const Choice one = bnb_choice(M, K, h[i], cus);
            ok = ok && valid_gemm_cfg(one.cfg, M, h[i].N, K) && bnb_cfg_ok(one.cfg, h[i]) &&
                 cfg_runs(one.cfg, M, K, &h[i], 1, cus) == NF4DQ_OK;
            w = workspace_need(M, h[i].N, K, one.cfg);
            need = w > need ? w : need;
        }
        return ok;
    };
    const int v = check(bn, nested) && check(bs, single);
    const LaunchShape a = launch_shape(bn.cfg, M, K, nested.data(), count, cus);
    const LaunchShape s = launch_shape(bs.cfg, M, K, single.data(), count, cus);
    const LaunchShape b = launch_shape(bn.cfg, M, K, ref.data(), count, cus);
    printf("{\"c\":[%d,%lld,%lld,%d,%d]", cus, (long long)M, (long long)K, sh, group);
    put("ref", rc.cfg);
    put("first", rc.first);
    put("bnb", bn.cfg);
    put("bnbs", bs.cfg);
    printf(",\"refpw\":%d,\"pw\":%d,\"pws\":%d,\"v\":%d,\"need\":%zu,\"ws\":%zu", (int)rc.per_weight, (int)bn.per_weight,
           (int)bs.per_weight, v, need, bnb_grouped_workspace(M, K, nm.data(), count, nullptr));
    printf(",\"shape\":[%u,%u,%u,%u,%u,%u,%u,%u,%u],\"lds\":%u,\"tables\":%d}\n", a.grid, a.block, a.dyn, s.grid, s.block,
           s.dyn, b.grid, b.block, b.dyn, static_lds(bn.cfg, kScaleBnb, M) + a.dyn,
           bn.cfg.kernel == NF4DQ_GEMM_XR ? group_tables(nested.data(), count) : 0);
}

int main() {
    printf("{\"mat\":[%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu]}\n", sizeof(nf4_gemm_bnb_mat),
           offsetof(nf4_gemm_bnb_mat, packed), offsetof(nf4_gemm_bnb_mat, packed_len),
           offsetof(nf4_gemm_bnb_mat, absmax_q), offsetof(nf4_gemm_bnb_mat, nb), offsetof(nf4_gemm_bnb_mat, code2),
           offsetof(nf4_gemm_bnb_mat, absmax2), offsetof(nf4_gemm_bnb_mat, n2), offsetof(nf4_gemm_bnb_mat, offset),
           offsetof(nf4_gemm_bnb_mat, blocksize), offsetof(nf4_gemm_bnb_mat, blocksize2), offsetof(nf4_gemm_bnb_mat, y),
           offsetof(nf4_gemm_bnb_mat, N));
    const int64_t Ms[] = {1, 2, 4, 5, 8, 9, 12, 16, 17, 24, 25, 32};
    const int64_t Ks[] = {1024, 2048, 4096, 14336};
    const std::vector<int64_t> groups[] = {{4096, 1024, 1024}, {14336, 14336}, {64, 192, 64}};
    for (int cus : {256, 64})
        for (int sh = 0; sh < 2; ++sh)
            for (int64_t K : Ks)
                for (int64_t M : Ms)
                    for (int g = 0; g < 3; ++g) run_case(cus, M, K, sh, g, groups[g]);
    return 0;
}
