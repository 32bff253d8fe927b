// nf4_gemm.hip -- fused NF4 dequant + GEMM for small M: the C ABI of include/nf4_dequant.h
// and the host dispatch behind it.  Each entry validates its arguments, asks the plan
// (nf4_gemm_plan.h: library choice of kernel and decomposition, fallbacks, workspace
// size) what runs, and launches it.  The kernels are in nf4_gemm_dev.h (see its comment
// for the design), their launchers in nf4_gemm_launch_*.hip.
#include "nf4_gemm_launch.h"

namespace {

using namespace nf4gemm;

int launch(const nf4_gemm_cfg& cfg, const HostMat* h, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
           void* workspace, int cus, hipStream_t st) {
    if (count > 1 && h[0].mode != kScaleRef) {  // grouped bitsandbytes modes: all nested or all single
        for (int i = 1; i < count; ++i)
            if (h[i].mode != h[0].mode) return NF4DQ_ERR_ARG;
        if (!bnb_grouped_cfg_ok(cfg, h, count)) return NF4DQ_ERR_ARG;
        switch (cfg.kernel) {
            case NF4DQ_GEMM_K128: return launch_k128_bnbg(h, count, x, M, K, dtype, cfg, workspace, cus, st);
            case NF4DQ_GEMM_PERSIST: return launch_persist_bnbg(h, count, x, M, K, dtype, cfg, workspace, cus, st);
            case NF4DQ_GEMM_XR: return launch_xr_bnbg(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        }
        return NF4DQ_ERR_ARG;
    }
    if (count > 0 && h[0].mode != kScaleRef) {  // bitsandbytes scale modes: one weight, a family that has them
        if (!bnb_cfg_ok(cfg, h[0])) return NF4DQ_ERR_ARG;
        switch (cfg.kernel) {
            case NF4DQ_GEMM_K128: return launch_k128_bnb(h, count, x, M, K, dtype, cfg, workspace, cus, st);
            case NF4DQ_GEMM_PERSIST: return launch_persist_bnb(h, count, x, M, K, dtype, cfg, workspace, cus, st);
            case NF4DQ_GEMM_XR: return launch_xr_bnb(h, count, x, M, K, dtype, cfg, workspace, cus, st);
            case NF4DQ_GEMM_GEMV: return launch_gemv_bnb(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        }
        return NF4DQ_ERR_ARG;
    }
    switch (cfg.kernel) {
        case NF4DQ_GEMM_K128: return launch_k128(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        case NF4DQ_GEMM_STREAM: return launch_stream(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        case NF4DQ_GEMM_PERSIST: return launch_persist(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        case NF4DQ_GEMM_XS: return launch_xs(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        case NF4DQ_GEMM_XR: return launch_xr(h, count, x, M, K, dtype, cfg, workspace, cus, st);
        case NF4DQ_GEMM_GEMV: return launch_gemv(h, count, x, M, K, dtype, cfg, workspace, cus, st);
    }
    return NF4DQ_ERR_ARG;
}

// The split-K slab is addressed through one buffer descriptor (32-bit range).
int check_workspace(size_t need, const void* workspace, size_t workspace_bytes) {
    if (need >= (size_t(1) << 32)) return NF4DQ_ERR_TOO_LARGE;
    return need && (!workspace || workspace_bytes < need || !aligned16(workspace)) ? NF4DQ_ERR_ARG : NF4DQ_OK;
}

// The one dispatch path: `count` validated weights over ntot columns sharing x; `first`
// validated for every weight.  Checks the workspace and launches what the plan chose.
int run(const Choice& ch, bool named, int cus, const HostMat* h, int count, int64_t ntot, const void* x, int64_t M,
        int64_t K, int32_t dtype, void* workspace, size_t workspace_bytes, hipStream_t st) {
    int rc = check_workspace(workspace_need(M, ntot, K, ch.first), workspace, workspace_bytes);
    // a cfg the caller named never falls back: what keeps it from running is the caller's error
    if (!rc && named) rc = cfg_runs(ch.cfg, M, K, h, count, cus);
    if (rc) return rc;
    if (!ch.per_weight) return launch(ch.cfg, h, count, x, M, K, dtype, workspace, cus, st);
    // the library's persistent choice cannot run here: each weight's own next choice
    // (callers size the workspace with the size entries: the largest of these needs too)
    // (a bnb group: each weight's bnb_choice)
    for (int i = 0; i < count && !rc; ++i) {
        const nf4_gemm_cfg c = h[i].mode == kScaleRef ? launch_cfg(ch, M, K, h[i]) : bnb_choice(M, K, h[i], cus).cfg;
        if (!valid_gemm_cfg(c, M, h[i].N, K)) return NF4DQ_ERR_ARG;
        rc = check_workspace(workspace_need(M, h[i].N, K, c), workspace, workspace_bytes);
        if (!rc) rc = launch(c, &h[i], 1, x, M, K, dtype, workspace, cus, st);
    }
    return rc;
}

int gemm_impl(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
              int64_t nb, const float* absmax2, int64_t n2, void* y, int32_t dtype, int64_t N, int64_t K,
              void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfgp, hipStream_t st) {
    if (dtype != NF4DQ_F16 && dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (M < 0 || N < 0 || K < 0 || nb <= 0 || n2 <= 0) return NF4DQ_ERR_ARG;
    if (M == 0 || N == 0) return NF4DQ_OK;
    if (!x || !packed || !absmax_q || !absmax2 || !y) return NF4DQ_ERR_ARG;
    if (M > NF4DQ_GEMM_MAX_M || N % 64 || K % kChunkK || packed_len != N * (K / 2)) return NF4DQ_ERR_SHAPE;
    if ((size_t)(N / 16) * 4 > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    if (packed_len >= (int64_t(1) << 31) || M * K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    const HostMat h{packed, packed_len, absmax_q, nb, absmax2, n2, y, N};
    const int cus = device_cus();
    const Choice ch = cfgp ? explicit_choice(*cfgp, M, N, K) : library_choice(M, K, &h, 1, cus);
    if (!valid_gemm_cfg(ch.first, M, N, K)) return NF4DQ_ERR_ARG;
    return run(ch, cfgp != nullptr, cus, &h, 1, N, x, M, K, dtype, workspace, workspace_bytes, st);
}

// bitsandbytes semantics (nf4_gemm_bnb, nf4_gemm_bnb_single): the flat stream's statistics,
// no wrap.  Single mode: absmax_q and code2 null, absmax2 = the fp32 absmax, n2 = its length.
int gemm_bnb_impl(bool single, const void* x, int64_t M, const uint8_t* packed, int64_t packed_len,
                  const uint8_t* absmax_q, int64_t nb, const float* code2, const float* absmax2, int64_t n2,
                  const float* offset, int32_t blocksize, int32_t blocksize2, void* y, int32_t dtype, int64_t N,
                  int64_t K, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfgp, hipStream_t st) {
    if (dtype != NF4DQ_F16 && dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (M < 0 || N < 0 || K < 0 || nb < 0 || n2 < 0) return NF4DQ_ERR_ARG;
    if (blocksize < 64 || blocksize > 4096 || (blocksize & (blocksize - 1))) return NF4DQ_ERR_ARG;
    if (!single && (blocksize2 < 4 || (blocksize2 & (blocksize2 - 1)))) return NF4DQ_ERR_ARG;
    if (M == 0 || N == 0) return NF4DQ_OK;
    if (!x || !packed || !absmax2 || !y || (!single && (!absmax_q || !code2))) return NF4DQ_ERR_ARG;
    if (M > NF4DQ_GEMM_MAX_M || N % 64 || K % kChunkK || packed_len != N * (K / 2)) return NF4DQ_ERR_SHAPE;
    if ((size_t)(N / 16) * 4 > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    if (packed_len >= (int64_t(1) << 31) || M * K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    int sh = 0, sh2 = 0;
    while ((64 << sh) < blocksize) ++sh;
    while (!single && (1 << sh2) < blocksize2) ++sh2;
    const int64_t nblk = (N * K + blocksize - 1) / blocksize;
    if (single ? n2 < nblk : (nb < nblk || n2 < (nblk + blocksize2 - 1) / blocksize2)) return NF4DQ_ERR_SHAPE;
    HostMat h{packed, packed_len, absmax_q, single ? n2 : nb, absmax2, n2, y, N};
    h.mode = single ? kScaleBnbSingle : kScaleBnb;
    h.code2 = code2;
    h.offset = single ? nullptr : offset;
    h.sh = sh;
    h.sh2 = sh2;
    const int cus = device_cus();
    const Choice ch = cfgp ? explicit_choice(*cfgp, M, N, K) : bnb_choice(M, K, h, cus);
    // a family without the mode (or, above blocksize 64, any but the 128-deep one) is the caller's error
    if (!bnb_cfg_ok(ch.first, h) || !valid_gemm_cfg(ch.first, M, N, K)) return NF4DQ_ERR_ARG;
    return run(ch, cfgp != nullptr, cus, &h, 1, N, x, M, K, dtype, workspace, workspace_bytes, st);
}

// Weights that share x, one launch of whichever kernel cfg names (workgroups
// numbered over all the weights' strips / column groups); the library's
// persistent choice, when it cannot run, falls back to per-weight launches.
int gemm_grouped_impl(const void* x, int64_t M, int64_t K, const nf4_gemm_mat* mats, int32_t count, int32_t dtype,
                      void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfgp, hipStream_t st) {
    if (count < 0 || count > NF4DQ_GEMM_GROUP_MAX || (count > 0 && !mats)) return NF4DQ_ERR_ARG;
    if (dtype != NF4DQ_F16 && dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (M < 0 || K < 0) return NF4DQ_ERR_ARG;
    HostMat h[NF4DQ_GEMM_GROUP_MAX];
    int64_t ntot = 0;
    for (int i = 0; i < count; ++i) {
        const nf4_gemm_mat& m = mats[i];
        if (m.N < 0 || m.nb <= 0 || m.n2 <= 0) return NF4DQ_ERR_ARG;
        if (!m.packed || !m.absmax_q || !m.absmax2 || !m.y) return NF4DQ_ERR_ARG;
        if (m.N % 64 || m.packed_len != m.N * (K / 2)) return NF4DQ_ERR_SHAPE;
        h[i] = HostMat{m.packed, m.packed_len, m.absmax_q, m.nb, m.absmax2, m.n2, m.y, m.N};
        ntot += m.N;
    }
    if (M == 0 || ntot == 0 || count == 0) return NF4DQ_OK;
    if (!x) return NF4DQ_ERR_ARG;
    if (M > NF4DQ_GEMM_MAX_M || K % kChunkK) return NF4DQ_ERR_SHAPE;
    if ((size_t)(ntot / 16) * 4 > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const int cus = device_cus();
    const Choice ch = cfgp ? explicit_choice(*cfgp, M, ntot, K) : library_choice(M, K, h, count, cus);
    for (int i = 0; i < count; ++i) {
        if (h[i].N == 0 && !takes_empty_weight(ch.first.kernel)) return NF4DQ_ERR_SHAPE;
        if (h[i].N == 0) continue;
        if (!valid_gemm_cfg(ch.first, M, h[i].N, K)) return NF4DQ_ERR_ARG;
        if (h[i].packed_len >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    }
    if (M * K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    return run(ch, cfgp != nullptr, cus, h, count, ntot, x, M, K, dtype, workspace, workspace_bytes, st);
}

// Weights in bitsandbytes semantics that share x (nf4_gemm_bnb_grouped): the rules of
// gemm_bnb_impl per weight and of gemm_grouped_impl for the group; one launch of a family
// with the grouped mode (bnb_grouped_choice), a single weight through the one-weight launch.
int gemm_bnb_grouped_impl(const void* x, int64_t M, int64_t K, const nf4_gemm_bnb_mat* mats, int32_t count,
                          bool single, int32_t dtype, void* workspace, size_t workspace_bytes,
                          const nf4_gemm_cfg* cfgp, hipStream_t st) {
    if (count < 0 || count > NF4DQ_GEMM_GROUP_MAX || (count > 0 && !mats)) return NF4DQ_ERR_ARG;
    if (dtype != NF4DQ_F16 && dtype != NF4DQ_BF16) return NF4DQ_ERR_ARG;
    if (M < 0 || K < 0) return NF4DQ_ERR_ARG;
    HostMat h[NF4DQ_GEMM_GROUP_MAX];
    int64_t ntot = 0;
    for (int i = 0; i < count; ++i) {
        const nf4_gemm_bnb_mat& m = mats[i];
        if (m.N < 0 || m.nb < 0 || m.n2 < 0) return NF4DQ_ERR_ARG;
        if (m.blocksize < 64 || m.blocksize > 4096 || (m.blocksize & (m.blocksize - 1))) return NF4DQ_ERR_ARG;
        if (!single && (m.blocksize2 < 4 || (m.blocksize2 & (m.blocksize2 - 1)))) return NF4DQ_ERR_ARG;
        if (!m.packed || !m.absmax2 || !m.y || (!single && (!m.absmax_q || !m.code2))) return NF4DQ_ERR_ARG;
        if (m.N % 64 || m.packed_len != m.N * (K / 2)) return NF4DQ_ERR_SHAPE;
        int sh = 0, sh2 = 0;
        while ((64 << sh) < m.blocksize) ++sh;
        while (!single && (1 << sh2) < m.blocksize2) ++sh2;
        const int64_t nblk = (m.N * K + m.blocksize - 1) / m.blocksize;
        if (single ? m.n2 < nblk : (m.nb < nblk || m.n2 < (nblk + m.blocksize2 - 1) / m.blocksize2))
            return NF4DQ_ERR_SHAPE;
        h[i] = HostMat{m.packed, m.packed_len, single ? nullptr : m.absmax_q, single ? m.n2 : m.nb, m.absmax2, m.n2,
                       m.y, m.N};
        if (m.N == 0) h[i].nb = h[i].n2 = 1;  // an empty weight owns nothing: no statistics, but no zero divisor
        h[i].mode = single ? kScaleBnbSingle : kScaleBnb;
        h[i].code2 = single ? nullptr : m.code2;
        h[i].offset = single ? nullptr : m.offset;
        h[i].sh = sh;
        h[i].sh2 = sh2;
        ntot += m.N;
    }
    if (M == 0 || ntot == 0 || count == 0) return NF4DQ_OK;
    if (!x) return NF4DQ_ERR_ARG;
    if (M > NF4DQ_GEMM_MAX_M || K % kChunkK) return NF4DQ_ERR_SHAPE;
    if ((size_t)(ntot / 16) * 4 > kCounterBytes) return NF4DQ_ERR_TOO_LARGE;
    const int cus = device_cus();
    Choice ch;
    if (cfgp) ch = explicit_choice(*cfgp, M, ntot, K);
    else if (count == 1) ch = bnb_choice(M, K, h[0], cus);
    else ch = bnb_grouped_choice(M, K, h, count, cus);
    // a family without the grouped mode (or, above blocksize 64, any but the 128-deep one) is
    // the caller's error; one weight follows nf4_gemm_bnb's rule
    if (count == 1 ? !bnb_cfg_ok(ch.first, h[0]) : !bnb_grouped_cfg_ok(ch.first, h, count)) return NF4DQ_ERR_ARG;
    for (int i = 0; i < count; ++i) {
        if (h[i].N == 0 && !takes_empty_weight(ch.first.kernel)) return NF4DQ_ERR_SHAPE;
        if (h[i].N == 0) continue;
        if (!valid_gemm_cfg(ch.first, M, h[i].N, K)) return NF4DQ_ERR_ARG;
        if (h[i].packed_len >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    }
    if (M * K * 2 >= (int64_t(1) << 31)) return NF4DQ_ERR_TOO_LARGE;
    return run(ch, cfgp != nullptr, cus, h, count, ntot, x, M, K, dtype, workspace, workspace_bytes, st);
}

}  // namespace

extern "C" {

size_t nf4_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) { return library_workspace(M, N, K); }

size_t nf4_gemm_workspace_bytes_cfg(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg) {
    return cfg ? workspace_need(M, N, K, *cfg) : library_workspace(M, N, K);
}

int nf4_gemm_ref(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                 int64_t nb, const float* absmax2, int64_t n2, void* y, int32_t dtype, int64_t N, int64_t K,
                 void* workspace, size_t workspace_bytes, void* hip_stream) {
    return gemm_impl(x, M, packed, packed_len, absmax_q, nb, absmax2, n2, y, dtype, N, K, workspace, workspace_bytes,
                     nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

size_t nf4_gemm_grouped_workspace_bytes(int64_t M, int64_t K, const nf4_gemm_mat* mats, int32_t count,
                                        const nf4_gemm_cfg* cfg) {
    return grouped_workspace(M, K, mats, count, cfg);
}

size_t nf4_gemm_bnb_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg) {
    return cfg ? workspace_need(M, N, K, *cfg) : bnb_library_workspace(M, N, K);
}

int nf4_gemm_bnb(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                 int64_t nb, const float* code2, const float* absmax2, int64_t n2, const float* offset,
                 int32_t blocksize, int32_t blocksize2, void* y, int32_t out_dtype, int64_t N, int64_t K,
                 void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    return gemm_bnb_impl(false, x, M, packed, packed_len, absmax_q, nb, code2, absmax2, n2, offset, blocksize,
                         blocksize2, y, out_dtype, N, K, workspace, workspace_bytes, cfg,
                         reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_bnb_single(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const float* absmax,
                        int64_t nabs, int32_t blocksize, void* y, int32_t out_dtype, int64_t N, int64_t K,
                        void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    return gemm_bnb_impl(true, x, M, packed, packed_len, nullptr, 0, nullptr, absmax, nabs, nullptr, blocksize, 1, y,
                         out_dtype, N, K, workspace, workspace_bytes, cfg, reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_ref_grouped(const void* x, int64_t M, int64_t K, const nf4_gemm_mat* mats, int32_t count,
                         int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                         void* hip_stream) {
    return gemm_grouped_impl(x, M, K, mats, count, out_dtype, workspace, workspace_bytes, cfg,
                             reinterpret_cast<hipStream_t>(hip_stream));
}

size_t nf4_gemm_bnb_grouped_workspace_bytes(int64_t M, int64_t K, const void* mats, int32_t count, int32_t single,
                                            const nf4_gemm_cfg* cfg) {
    (void)single;  // the need does not depend on the statistics' form
    return bnb_grouped_workspace(M, K, reinterpret_cast<const nf4_gemm_bnb_mat*>(mats), count, cfg);
}

int nf4_gemm_bnb_grouped(const void* x, int64_t M, int64_t K, const void* mats, int32_t count, int32_t single,
                         int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                         void* hip_stream) {
    return gemm_bnb_grouped_impl(x, M, K, reinterpret_cast<const nf4_gemm_bnb_mat*>(mats), count, single != 0,
                                 out_dtype, workspace, workspace_bytes, cfg, reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_check_workspace(void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!workspace || workspace_bytes == 0) return NF4DQ_OK;  // no split-K ran on it
    if (workspace_bytes < kHeaderBytes) return NF4DQ_ERR_ARG;  // never a split-K workspace
    const hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    uint32_t err = 0;
    hipError_t e = hipMemcpyAsync(&err, reinterpret_cast<char*>(workspace) + kCounterBytes, sizeof(err),
                                  hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_rc2(e);
    if (!err) return NF4DQ_OK;
    // every kernel of the stream has finished: no late store can land after this
    e = hipMemsetAsync(workspace, 0, workspace_bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e != hipSuccess ? hip_rc2(e) : NF4DQ_ERR_SPLITK_TIMEOUT;
}

int nf4_gemm_ref_cfg(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                     int64_t nb, const float* absmax2, int64_t n2, void* y, int32_t dtype, int64_t N, int64_t K,
                     void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    return gemm_impl(x, M, packed, packed_len, absmax_q, nb, absmax2, n2, y, dtype, N, K, workspace, workspace_bytes,
                     cfg, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
