// gemm_bnb_plan_check.cpp -- what the fused GEMM's host plan (nf4_gemm_plan.h) decides for
// the bitsandbytes-semantics entries, over the single-weight (M, K, N) cases of
// gemm_plan_check.cpp, one compact JSON line each, integers only:
//   c     the case: [cus, M, K, N, sh]        (sh = log2(blocksize / 64): 0, and 1 where noted)
//   ref   the launch the reference plan runs:  [kernel, waves, depth, ksplit, strips]
//   bnb   the launch bnb_choice runs, nested mode; bnbs: single mode
//   v     bnb / bnbs valid for the weight and accepted by the entries (bnb_cfg_ok)
//   need  the most either call checks the workspace against;  ws  nf4_gemm_bnb_workspace_bytes(NULL)
//   shape grid, block, dynamic LDS of the bnb launch and of the reference launch of the same cfg
// tests/test_gemm_bnb_plan_cpu.py builds this for the host (no GPU, no HIP) and checks the lines.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_plan.h"

using namespace nf4gemm;

static void put(const char* key, const nf4_gemm_cfg& c) {
    printf(",\"%s\":[%d,%d,%d,%d,%d]", key, c.kernel, c.waves, c.depth, c.ksplit, c.strips);
}

static void run_case(int cus, int64_t M, int64_t K, int64_t N, int sh) {
    static uint8_t dummy[16];  // the plan never reads through the pointers
    const int64_t nb = N * (K / 64), n2 = N * ((K / 64 + 3) / 4);
    const HostMat ref{dummy, N * (K / 2), dummy, nb, reinterpret_cast<const float*>(dummy), n2, dummy, N};
    HostMat nested = ref, single = ref;
    nested.mode = kScaleBnb;
    nested.code2 = nested.offset = reinterpret_cast<const float*>(dummy);
    nested.sh = sh;
    nested.sh2 = 8;
    nested.nb = ((N * K) >> (6 + sh));
    nested.n2 = (nested.nb + 255) / 256;
    single.mode = kScaleBnbSingle;
    single.a1 = nullptr;
    single.sh = sh;
    single.nb = single.n2 = nested.nb;
    const Choice rc = library_choice(M, K, &ref, 1, cus);
    const nf4_gemm_cfg rcfg = launch_cfg(rc, M, K, ref);
    const Choice bn = bnb_choice(M, K, nested, cus), bs = bnb_choice(M, K, single, cus);
    const int v = valid_gemm_cfg(bn.cfg, M, N, K) && bnb_cfg_ok(bn.cfg, nested) && !bn.per_weight &&
                  cfg_runs(bn.cfg, M, K, &nested, 1, cus) == NF4DQ_OK && valid_gemm_cfg(bs.cfg, M, N, K) &&
                  bnb_cfg_ok(bs.cfg, single) && !bs.per_weight && cfg_runs(bs.cfg, M, K, &single, 1, cus) == NF4DQ_OK;
    const size_t n1 = workspace_need(M, N, K, bn.first), n2w = workspace_need(M, N, K, bs.first);
    const LaunchShape a = launch_shape(bn.cfg, M, K, &nested, 1, cus), b = launch_shape(bn.cfg, M, K, &ref, 1, cus);
    printf("{\"c\":[%d,%lld,%lld,%lld,%d]", cus, (long long)M, (long long)K, (long long)N, sh);
    put("ref", rcfg);
    put("bnb", bn.cfg);
    put("bnbs", bs.cfg);
    printf(",\"v\":%d,\"need\":%zu,\"ws\":%zu,\"shape\":[%u,%u,%u,%u,%u,%u]}\n", v, n1 > n2w ? n1 : n2w,
           bnb_library_workspace(M, N, K), a.grid, a.block, a.dyn, b.grid, b.block, b.dyn);
}

int main() {
    const int64_t Ms[] = {1, 2, 4, 5, 8, 9, 12, 16, 17, 24, 25, 32};
    const int64_t Ks[] = {128, 384, 1280, 2048, 2304, 4096, 8192, 14336, 16384, 16512};
    const int64_t Nthr[] = {1024, 4096, 6144, 8192, 12288, 16384, 24576};
    const int64_t Nrest[] = {64, 192, 2048, 4160, 14336, 28672};
    for (int sh = 0; sh < 2; ++sh) {
        for (int64_t M : Ms) {
            for (int64_t N : Nthr) run_case(256, M, 4096, N, sh);
            for (int64_t K : Ks)
                if (K != 4096) run_case(256, M, K, 4096, sh);
        }
        for (int64_t M : {1, 16, 32})
            for (int64_t N : Nrest)
                for (int64_t K : {1280, 4096}) run_case(256, M, K, N, sh);
        for (int64_t M : {17, 32})
            for (int64_t N : {6144, 12288}) run_case(256, M, 384, N, sh);
    }
    for (int64_t M : Ms)
        for (int64_t N : Nthr) run_case(64, M, 4096, N, 0);
    return 0;
}
