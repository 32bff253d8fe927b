// nf4_lora.hip -- the fused adapter launch of a Linear4bit (nf4_lora_add: y_i = base_i +
// scale_i * B_i (A_i x) for up to NF4DQ_LORA_GROUP_MAX adapters over one x): kernel, launcher and
// the C entry.  The plan -- validation, cfg, geometry, LDS -- is nf4_lora_plan.h.
//
// One workgroup per (adapter, tile of tile_n columns).  Shrink: the workgroup forms its adapter's
// whole t = rn(x A^T) with v_mfma_f32_16x16x32_{bf16,f16}, x rows as the A operand and rows of
// the adapter's A as the B operand (both are 16 contiguous bytes per lane in their natural
// layout), the K / 32 chunks split into one contiguous range per wave; the waves' fp32 partials
// meet in LDS and are summed in wave order, rounded once to 16 bits into the t image.  Expand:
// wave w takes the strips w, w + waves, .. of 16 columns; t from LDS is the A operand, rows of the
// adapter's B the B operand; the epilogue (rn, * scale, rn, + base, rn) runs in registers and each
// lane reads and writes its own four elements per row tile.
#include <type_traits>

#include "nf4_common.h"
#include "nf4_lora_plan.h"

namespace {

using namespace nf4dq;
using nf4lora::LoraPlan;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LoraMat {
    const char* A;
    const char* B;
    const uint16_t* base;
    uint16_t* y;
    uint32_t N, r;
    float scale;
    uint32_t tile0;  // the adapter's first workgroup
};

struct LoraArgs {
    const char* x;
    uint32_t M, K, nmat, tile_n;
    uint32_t row_blocks, ts, t_bytes;
    LoraMat m[NF4DQ_LORA_GROUP_MAX];
};

template <int DT>
__device__ __forceinline__ f32x4 lora_mfma(const u32x4& a, const u32x4& b, const f32x4& c) {
    if constexpr (DT == NF4DQ_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// fp32 -> 16 bits, round to nearest even (the value kept opaque: see nf4_common.h).
template <int DT>
__device__ __forceinline__ uint16_t rn16(float v) {
    v = opaque(v);
    if constexpr (DT == NF4DQ_BF16) return __builtin_bit_cast(uint16_t, (__bf16)v);
    else return __builtin_bit_cast(uint16_t, (_Float16)v);
}
template <int DT>
__device__ __forceinline__ float up16(uint16_t h) {
    if constexpr (DT == NF4DQ_BF16) return __uint_as_float((uint32_t)h << 16);
    else return (float)__builtin_bit_cast(_Float16, h);
}

__device__ __forceinline__ u32x4 ld16(const char* p) { return *reinterpret_cast<const u32x4*>(p); }

// MB: row tiles of 16 per row block; RT: r tiles of 16 the accumulators cover (the group's largest
// r, rounded up to a power of two; an adapter's own tiles and k steps are run-time bounds).
template <int DT, int MB, int RT>
__global__ __launch_bounds__(64 * nf4lora::kMaxWaves) void nf4_lora_kernel(const LoraArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr uint32_t kRows = 16 * MB, kCols = 16 * RT, kKS = RT == 1 ? 1 : RT / 2;
    constexpr uint32_t kPS = kCols + nf4lora::kPartPad;  // floats between rows of the partials
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, W = blockDim.x >> 6;
    const uint32_t lr = lane & 15u, lh = lane >> 4;
    uint32_t mi = 0;
    for (uint32_t i = 1; i < a.nmat; ++i) mi = blockIdx.x >= a.m[i].tile0 ? i : mi;
    const LoraMat& m = a.m[mi];
    const uint32_t M = a.M, K = a.K, r = m.r, ts = a.ts;
    const uint32_t rtiles = (r + 15u) >> 4, ksteps = (r + 31u) >> 5;
    uint16_t* t = reinterpret_cast<uint16_t*>(lds);
    float* part = reinterpret_cast<float*>(lds + a.t_bytes);

    // t starts as zeros: the columns from r to the MFMA depth are never written again
    for (uint32_t i = tid * 16u; i < a.t_bytes; i += blockDim.x * 16u) *reinterpret_cast<u32x4*>(lds + i) = u32x4{0, 0, 0, 0};

    // ---- shrink ----
    const uint32_t chunks = K >> 5, cpw = (chunks + W - 1) / W;
    const uint32_t c0 = min(wave * cpw, chunks), c1 = min(c0 + cpw, chunks);
    for (uint32_t rb = 0; rb < a.row_blocks; ++rb) {
        f32x4 acc[MB][RT];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[mb][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // Every load is unconditional -- a lane past M or r reads row 0 and its fragment is zeroed
        // in registers -- and kU chunks are loaded per step, so that a step's loads are all in
        // flight before its first MFMA waits for one: the loop is bound by load latency, not by
        // bytes.  A chunk past the wave's range re-reads the last one and takes no part in the sum
        // (not even as a zero operand: the x it re-read may hold an infinity, and inf * 0 is NaN):
        // the order of the sum stays c0, c0 + 1, ..
        constexpr uint32_t kU = RT >= 8 ? 2 : 4;
        const u32x4 zero = {0, 0, 0, 0};
        const char* xp[MB];
        bool xin[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const uint32_t row = rb * kRows + 16u * mb + lr;
            xin[mb] = row < M;
            xp[mb] = a.x + ((size_t)(xin[mb] ? row : 0u) * K + 8u * lh) * 2u;
        }
        const char* ap[RT];
        bool ain[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t j = 16u * rt + lr;
            ain[rt] = j < r;
            ap[rt] = m.A + ((size_t)(ain[rt] ? j : 0u) * K + 8u * lh) * 2u;
        }
        for (uint32_t c = c0; c < c1; c += kU) {
            u32x4 xf[kU][MB], af[kU][RT];
#pragma unroll
            for (uint32_t h = 0; h < kU; ++h) {
                const size_t kb = (size_t)min(c + h, c1 - 1u) * 64u;  // bytes; a chunk past the range re-reads the last
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) xf[h][mb] = ld16(xp[mb] + kb);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) af[h][rt] = ld16(ap[rt] + kb);
            }
#pragma unroll
            for (uint32_t h = 0; h < kU; ++h) {
                if (c + h >= c1) break;  // uniform over the wave
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    if ((uint32_t)rt < rtiles) {
                        const u32x4 bq = ain[rt] ? af[h][rt] : zero;
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) acc[mb][rt] = lora_mfma<DT>(xin[mb] ? xf[h][mb] : zero, bq, acc[mb][rt]);
                    }
                }
            }
        }
        // D: column (r index) on lane & 15, row 4 * (lane >> 4) + register
        float* mine = part + (size_t)wave * kRows * kPS;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int g = 0; g < 4; ++g) mine[(16u * mb + 4u * lh + g) * kPS + 16u * rt + lr] = acc[mb][rt][g];
        __syncthreads();
        for (uint32_t e = tid; e < kRows * kCols; e += blockDim.x) {
            const uint32_t row = e / kCols, col = e % kCols, at = row * kPS + col;
            float s = part[at];
            for (uint32_t w = 1; w < W; ++w) s += part[(size_t)w * kRows * kPS + at];
            if (col < r) t[(size_t)(rb * kRows + row) * ts + col] = rn16<DT>(s);
        }
        __syncthreads();
    }

    // ---- expand ----
    const uint32_t n_begin = (blockIdx.x - m.tile0) * a.tile_n, strips = a.tile_n >> 4, mtiles = (M + 15u) >> 4;
    for (uint32_t s = wave; s < strips; s += W) {
        const uint32_t n0 = n_begin + 16u * s;
        if (n0 >= m.N) break;  // N % 16 == 0: a strip is whole or absent
        u32x4 bf[kKS];
#pragma unroll
        for (uint32_t ks = 0; ks < kKS; ++ks) {
            const uint32_t j = 32u * ks + 8u * lh;
            bf[ks] = j < r ? ld16(m.B + ((size_t)(n0 + lr) * r + j) * 2u) : u32x4{0, 0, 0, 0};
        }
        for (uint32_t mt = 0; mt < mtiles; ++mt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (uint32_t ks = 0; ks < kKS; ++ks) {
                if (ks < ksteps) {
                    const u32x4 tf = *reinterpret_cast<const u32x4*>(t + (size_t)(16u * mt + lr) * ts + 32u * ks + 8u * lh);
                    acc = lora_mfma<DT>(tf, bf[ks], acc);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t row = 16u * mt + 4u * lh + g;
                if (row < M) {
                    const size_t at = (size_t)row * m.N + n0 + lr;
                    const float u = up16<DT>(rn16<DT>(acc[g]));
                    uint16_t out = rn16<DT>(u * m.scale);
                    if (m.base) out = rn16<DT>(up16<DT>(m.base[at]) + up16<DT>(out));
                    m.y[at] = out;
                }
            }
        }
    }
}

inline int hip_rc(hipError_t e) { return e == hipSuccess ? NF4DQ_OK : NF4DQ_ERR_HIP_BASE + (int)e; }

// CUs of the current device (256 where it cannot be asked).  A plain static: a race between
// threads only repeats the query.
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

// Opt in once per kernel and device to dynamic LDS above 64 KiB (a race between threads only
// repeats the call), then launch.
template <int DT, int MB, int RT>
int launch(const LoraPlan& p, const LoraArgs& A, hipStream_t st) {
    static bool attr[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (p.dyn > 64u * 1024u && (dev < 0 || !attr[dev])) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&nf4_lora_kernel<DT, MB, RT>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)nf4lora::kLdsPerCu);
        if (e != hipSuccess) return hip_rc(e);
        if (dev >= 0) attr[dev] = true;
    }
    hipLaunchKernelGGL((nf4_lora_kernel<DT, MB, RT>), dim3(p.grid), dim3(p.block), p.dyn, st, A);
    return hip_rc(hipGetLastError());
}

template <int DT, int MB>
int launch_rt(const LoraPlan& p, const LoraArgs& A, hipStream_t st) {
    switch (p.rt) {
        case 1: return launch<DT, MB, 1>(p, A, st);
        case 2: return launch<DT, MB, 2>(p, A, st);
        case 4: return launch<DT, MB, 4>(p, A, st);
        default: return launch<DT, MB, 8>(p, A, st);
    }
}

}  // namespace

extern "C" int nf4_lora_add(const void* x, int64_t M, int64_t K, const void* mats, int32_t count, int32_t dtype,
                            const void* cfg, void* hip_stream) {
    const nf4_lora_mat* hm = reinterpret_cast<const nf4_lora_mat*>(mats);
    const nf4lora::LoraCall call{x, M, K, hm, count, dtype, reinterpret_cast<const nf4_lora_cfg*>(cfg)};
    int rc = nf4lora::validate(call);  // every rule answers before any device work
    if (rc) return rc;
    nf4_lora_cfg c{};
    rc = nf4lora::check(call, call.cfg ? 0 : device_cus(), &c);
    if (rc) return rc;
    const LoraPlan p = nf4lora::plan(c, M, hm, count);
    LoraArgs A{};
    A.x = reinterpret_cast<const char*>(x);
    A.M = (uint32_t)M;
    A.K = (uint32_t)K;
    A.nmat = (uint32_t)count;
    A.tile_n = p.tile_n;
    A.row_blocks = p.row_blocks;
    A.ts = p.ts;
    A.t_bytes = p.t_bytes;
    for (int32_t i = 0; i < count; ++i)
        A.m[i] = LoraMat{reinterpret_cast<const char*>(hm[i].A), reinterpret_cast<const char*>(hm[i].B),
                         reinterpret_cast<const uint16_t*>(hm[i].base), reinterpret_cast<uint16_t*>(hm[i].y),
                         (uint32_t)hm[i].N, (uint32_t)hm[i].r, hm[i].scale, p.tile0[i]};
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype == NF4DQ_BF16) return p.mb == 1 ? launch_rt<NF4DQ_BF16, 1>(p, A, st) : launch_rt<NF4DQ_BF16, 2>(p, A, st);
    return p.mb == 1 ? launch_rt<NF4DQ_F16, 1>(p, A, st) : launch_rt<NF4DQ_F16, 2>(p, A, st);
}
