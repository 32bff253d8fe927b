// nf4_gemm_launch.h -- launcher side of the fused GEMM: the interface between the host
// dispatch (nf4_gemm.hip) and the per-family launchers (nf4_gemm_launch_*.hip), and what
// the launchers share: the CU count, the kernel-argument fills, the template dispatch
// and the launch itself.  The plan they carry out is in nf4_gemm_plan.h.
#pragma once

#include <type_traits>

#include "nf4_gemm_dev.h"

namespace nf4gemm {

// Launchers (shapes and cfg validated and known to run by the dispatch; workspace sized
// by it; cus = device_cus(), which the plan was made for).  They return NF4DQ_OK or a HIP
// code; NF4DQ_ERR_ARG only for a plan that cannot run, which the dispatch never sends.
int launch_stream(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                  const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_persist(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                   const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_xs(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
              const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_xr(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
              const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_k128(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_gemv(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
// The same launchers with the bitsandbytes scale modes (mats[0].mode: kScaleBnb or
// kScaleBnbSingle; one weight), for the families that have them (bnb_has_mode).  Each is its
// family's launcher source compiled once more with NF4_GEMM_BNB defined
// (nf4_gemm_launch_*_bnb.hip), so the modes' kernels build beside the reference ones.
int launch_persist_bnb(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                       const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_xr_bnb(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                  const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_k128_bnb(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                    const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_gemv_bnb(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                    const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);

// ... and with the grouped form of those modes (2 to NF4DQ_GEMM_GROUP_MAX weights, all nested
// or all single, each with its own code2, offset and block sizes), for the families that have
// it (bnb_grouped_has_mode): the launcher source compiled a third time with NF4_GEMM_BNBG
// defined (nf4_gemm_launch_*_bnbg.hip).
int launch_persist_bnbg(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                        const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_xr_bnbg(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                   const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);
int launch_k128_bnbg(const HostMat* mats, int count, const void* x, int64_t M, int64_t K, int32_t dtype,
                     const nf4_gemm_cfg& cfg, void* workspace, int cus, hipStream_t st);

}  // namespace nf4gemm

// What a launcher source defines and instantiates: launch_<family> with the reference
// scale mode, launch_<family>_bnb with the two bitsandbytes modes, or launch_<family>_bnbg
// with their grouped form (the kernels' GRP flag, the longer argument struct).
#if defined(NF4_GEMM_BNBG)
#define NF4_GEMM_FN(name_) name_##_bnbg
#define NF4_GEMM_MODES nf4gemm::kScaleBnb, nf4gemm::kScaleBnbSingle
#define NF4_GEMM_GRP true
#elif defined(NF4_GEMM_BNB)
#define NF4_GEMM_FN(name_) name_##_bnb
#define NF4_GEMM_MODES nf4gemm::kScaleBnb, nf4gemm::kScaleBnbSingle
#define NF4_GEMM_GRP false
#else
#define NF4_GEMM_FN(name_) name_
#define NF4_GEMM_MODES nf4gemm::kScaleRef
#define NF4_GEMM_GRP false
#endif

namespace {

using nf4gemm::HostMat;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int hip_rc2(hipError_t e) { return e == hipSuccess ? NF4DQ_OK : NF4DQ_ERR_HIP_BASE + (int)e; }

// CUs of the current device (256 where it cannot be asked).
inline int device_cus() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// The header fields every family's argument struct has.
template <class Args>
inline void fill_common(Args& a, int count, const void* x, int64_t M, int64_t K, const nf4_gemm_cfg& cfg,
                        void* workspace) {
    a.nmat = (uint32_t)count;
    a.x = x;
    a.counters = reinterpret_cast<uint32_t*>(workspace);
    a.slab = cfg.ksplit > 1 ? reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(workspace) + kHeaderBytes) : nullptr;
    a.M = (uint32_t)M;
    a.K = (uint32_t)K;
    a.ksplit = (uint32_t)cfg.ksplit;
    a.bpr = (uint32_t)(K / 64);
    a.groups = (a.bpr + 3) / 4;
}

// The scale mode's launch-wide fields (the bnb entries take one weight).
template <class Args>
inline void fill_mode(Args& a, const HostMat& h) {
    a.code2 = h.code2;
    a.offset = h.offset;
    a.sh = (uint32_t)h.sh;
    a.sh2 = (uint32_t)h.sh2;
}

inline void fill_mode(StreamArgs& a, const HostMat& h) {  // over the unused second weight's slot
    a.bnb.f = BnbFields{h.code2, h.offset, (uint32_t)h.sh, (uint32_t)h.sh2};
}

// The mode fields of a launch: launch-wide (one weight), or (GRP) every weight's own.
template <bool GRP, class Args>
inline void fill_modes(Args& a, const HostMat* mats, int count) {
    if constexpr (GRP) {
        for (int i = 0; i < count; ++i)
            a.side[i] = BnbSide{mats[i].code2, mats[i].offset, (uint32_t)mats[i].sh, (uint32_t)mats[i].sh2};
    } else {
        if (count > 0) fill_mode(a, mats[0]);
    }
}

// One weight's pointers, N and absmax divisors.  The divisors are clamped, nb at 2^31
// and n2 at 2^29 (its byte length fits 32 bits): an nb index is below N * K / 64 < 2^26 and
// an n2 index below N * ceil(K / 256) <= packed_len / 64 < 2^25, so at or above either
// clamp nothing ever wraps and the clamped divisor gives the same remainders.
template <class Mat>
inline void fill_mat(Mat& m, const HostMat& h) {
    m.packed = h.packed;
    m.a1 = h.a1;
    m.a2 = h.a2;
    m.y = h.y;
    m.N = (uint32_t)h.N;
    m.nb = make_fastdiv((uint32_t)(h.nb > (int64_t(1) << 31) ? (int64_t(1) << 31) : h.nb));
    m.n2 = make_fastdiv((uint32_t)(h.n2 > (int64_t(1) << 29) ? (int64_t(1) << 29) : h.n2));
}

// Run-time value -> template argument: f(integral_constant<V>) for the first V equal to
// v, the last V when none is (cfg validity has ruled the rest out).
template <auto V, auto... Rest, class F>
inline void pick(decltype(V) v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<decltype(V), V>{});
    else if (v == V) f(std::integral_constant<decltype(V), V>{});
    else pick<Rest...>(v, f);
}

// Opt in once per kernel to dynamic LDS up to `cap` (static + dynamic above 64 KiB needs
// it), then launch.
template <auto Kernel, class Args>
inline void launch_lds(uint32_t cap, dim3 grid, dim3 block, uint32_t dyn, hipStream_t st, const Args& a) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)cap);
        attr = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, dyn, st, a);
}

}  // namespace
