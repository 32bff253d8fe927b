// gemm_plan_check.cpp -- prints what the fused GEMM's host plan (nf4_gemm_plan.h) decides
// for a fixed list of cases, one compact JSON line each, integers only:
//   c   the case: [cus, M, K, wrap, N of each weight...]   (wrap: nb = 7, n2 = 3)
//   rc  what the entry answers before anything is launched (2: an empty weight the
//       chosen kernel cannot take)
//   l   the launches: [kernel, waves, depth, ksplit, strips, weights, grid, block, dynamic LDS]
//       each -- one, or one per weight when the library's persistent choice falls back
//   ws  workspace bytes: nf4_gemm_workspace_bytes, _cfg with the first launch's cfg (both
//       over the column total), nf4_gemm_grouped_workspace_bytes without and with that cfg
//   need  the most the call checks the workspace against;  v  every launch's cfg is valid
//       for each of its weights
// tests/test_gemm_plan_cpu.py builds this for the host (no GPU, no HIP), runs it and
// compares the output with tests/plan/gemm_plan_snapshot.jsonl.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_gemm_plan.h"

using namespace nf4gemm;

struct Launch {
    nf4_gemm_cfg cfg;
    int count;
    uint32_t grid, block, dyn;
};

struct Result {
    int rc, nlaunch, valid;
    Launch l[NF4DQ_GEMM_GROUP_MAX];
    size_t ws[4], need;
};

// ---- evaluation ------------------------------------------------------------
static Launch launch_of(const nf4_gemm_cfg& c, int64_t M, int64_t K, const HostMat* mats, int count, int cus) {
    const LaunchShape s = launch_shape(c, M, K, mats, count, cus);  // what the launcher launches with
    return Launch{c, count, s.grid, s.block, s.dyn};
}

static Result eval_case(int64_t M, int64_t K, const HostMat* mats, int count, int cus) {
    Result r{};
    const Choice ch = library_choice(M, K, mats, count, cus);
    int64_t ntot = 0;
    for (int i = 0; i < count; ++i) ntot += mats[i].N;
    r.valid = 1;
    r.need = workspace_need(M, ntot, K, ch.first);
    for (int i = 0; i < count; ++i) {
        if (mats[i].N == 0 && !takes_empty_weight(ch.first.kernel)) r.rc = NF4DQ_ERR_SHAPE;
        if (mats[i].N != 0 && !valid_gemm_cfg(ch.first, M, mats[i].N, K)) r.valid = 0;
    }
    if (!r.rc && !ch.per_weight) {
        r.l[r.nlaunch++] = launch_of(ch.cfg, M, K, mats, count, cus);
        for (int i = 0; i < count; ++i)
            if (mats[i].N != 0 && !valid_gemm_cfg(ch.cfg, M, mats[i].N, K)) r.valid = 0;
    }
    for (int i = 0; !r.rc && ch.per_weight && i < count; ++i) {
        const nf4_gemm_cfg c = launch_cfg(ch, M, K, mats[i]);  // as the dispatch's per-weight loop
        r.l[r.nlaunch++] = launch_of(c, M, K, &mats[i], 1, cus);
        if (!valid_gemm_cfg(c, M, mats[i].N, K)) r.valid = 0;
        const size_t w = workspace_need(M, mats[i].N, K, c);
        r.need = w > r.need ? w : r.need;
    }
    const nf4_gemm_cfg* chosen = r.nlaunch ? &r.l[0].cfg : nullptr;
    r.ws[0] = library_workspace(M, ntot, K);
    r.ws[1] = chosen ? workspace_need(M, ntot, K, *chosen) : r.ws[0];
    r.ws[2] = grouped_workspace(M, K, mats, count, nullptr);
    r.ws[3] = grouped_workspace(M, K, mats, count, chosen);
    return r;
}

// ---- cases -----------------------------------------------------------------
static void run_case(int cus, int64_t M, int64_t K, bool wrap, const int64_t* Ns, int count) {
    HostMat mats[NF4DQ_GEMM_GROUP_MAX];
    static uint8_t dummy[16];  // the plan never reads through the pointers
    printf("{\"c\":[%d,%lld,%lld,%d", cus, (long long)M, (long long)K, (int)wrap);
    for (int i = 0; i < count; ++i) {
        const int64_t nb = Ns[i] * (K / 64), n2 = Ns[i] * ((K / 64 + 3) / 4);
        mats[i] = HostMat{dummy, Ns[i] * (K / 2), dummy, wrap || !nb ? 7 : nb, reinterpret_cast<const float*>(dummy),
                          wrap || !n2 ? 3 : n2, dummy, Ns[i]};
        printf(",%lld", (long long)Ns[i]);
    }
    const Result r = eval_case(M, K, mats, count, cus);
    printf("],\"rc\":%d,\"l\":[", r.rc);
    for (int i = 0; i < r.nlaunch; ++i) {
        const Launch& l = r.l[i];
        printf("%s[%d,%d,%d,%d,%d,%d,%u,%u,%u]", i ? "," : "", l.cfg.kernel, l.cfg.waves, l.cfg.depth, l.cfg.ksplit,
               l.cfg.strips, l.count, l.grid, l.block, l.dyn);
    }
    printf("],\"ws\":[%zu,%zu,%zu,%zu],\"need\":%zu,\"v\":%d}\n", r.ws[0], r.ws[1], r.ws[2], r.ws[3], r.need, r.valid);
}

int main() {
    const int64_t Ms[] = {1, 2, 4, 5, 8, 9, 12, 16, 17, 24, 25, 32};
    const int64_t Ks[] = {128, 384, 1280, 2048, 2304, 4096, 8192, 14336, 16384, 16512};
    const int64_t Nthr[] = {1024, 4096, 6144, 8192, 12288, 16384, 24576};  // where the defaults change
    const int64_t Nrest[] = {64, 192, 2048, 4160, 14336, 28672};
    // a thinned cross product: every M at every N threshold (K = 4096, also with 64 CUs)
    // and at every K (N = 4096); the other widths at the M edges, K = 1280 and 4096
    for (int wrap = 0; wrap < 2; ++wrap) {
        for (int64_t M : Ms) {
            for (int64_t N : Nthr) run_case(256, M, 4096, wrap, &N, 1);
            for (int64_t K : Ks)
                if (K != 4096) run_case(256, M, K, wrap, &Ks[5], 1);
        }
        for (int64_t M : {1, 16, 32})
            for (int64_t N : Nrest)
                for (int64_t K : {1280, 4096}) run_case(256, M, K, wrap, &N, 1);
        for (int64_t M : {17, 32})  // wide and K % 256 != 0: the shared-activation kernel
            for (int64_t N : {6144, 12288}) run_case(256, M, 384, wrap, &N, 1);
    }
    for (int64_t M : Ms)
        for (int64_t N : Nthr) run_case(64, M, 4096, false, &N, 1);
    // grouped: the sets of tests/test_gpu_gemm.py, and one with an empty weight
    const int64_t sets[5][3] = {{4096, 1024, 1024}, {512, 1536, -1}, {14336, 14336, -1}, {64, 64, -1}, {1024, 0, 512}};
    for (int wrap = 0; wrap < 2; ++wrap)
        for (const auto& s : sets)
            for (int64_t M : {1, 4, 12, 17, 32})
                for (int64_t K : {2048, 4096}) run_case(256, M, K, wrap, s, s[2] < 0 ? 2 : 3);
    return 0;
}
