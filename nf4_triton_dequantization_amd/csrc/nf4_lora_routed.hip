// nf4_lora_routed.hip -- the routed adapter launch of a Linear4bit (nf4_lora_add_routed: row m of
// the batch takes adapter adapter_ids[m] of each stack): kernel, launcher and the C entry.  The
// plan -- validation, cfg, geometry, LDS -- is nf4_lora_routed_plan.h.
//
// One workgroup per (stack, slot, tile of tile_n columns).  Every wave reads the M ids (two per
// lane, in-bounds repeats past M), ORs the ids present into one 64-bit set and takes the slot-th
// smallest as its adapter; two ballots give that adapter's rows, which wave 0 lists in LDS in
// ascending order by popcount prefix.  A slot beyond the adapters present returns before any load
// of x, A or B; slot 0's workgroups first store the rows without an adapter (base, or zeros) when
// base != y.  From there the workgroup is nf4_lora.hip's, over its listed rows instead of all M:
// the same shrink (the K / 32 chunks split into one contiguous range per wave, the MFMAs of a
// wave in chunk order, the partials summed in wave order, one rounding into the t image) with the
// x rows gathered through the list, the same expand with the rows scattered through it.  MFMA
// rows are independent, so a row's bits are those nf4_lora_add stores for it with this adapter
// and the same waves.  (The 16-bit helpers are nf4_lora.hip's, repeated here: that source stays
// as it is.)
#include <type_traits>

#include "nf4_common.h"
#include "nf4_lora_routed_plan.h"

namespace {

using namespace nf4dq;
using nf4lora::RoutedPlan;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct RoutedStack {
    const char* A;
    const char* B;
    const float* scale;
    const uint16_t* base;
    uint16_t* y;
    uint64_t a_bytes, b_bytes;  // bytes between adapters
    uint32_t N, r;
    uint32_t tile0;  // the stack's first workgroup
    uint32_t tiles;  // column tiles of the stack
};

struct RoutedArgs {
    const char* x;
    const int32_t* ids;
    uint32_t M, K, S, nstack, tile_n;
    uint32_t ts, t_bytes, part_bytes;
    RoutedStack m[NF4DQ_LORA_GROUP_MAX];
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

// The OR of a 32-bit value over the wave, the same in every lane.
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// MB: row tiles of 16 per row block; RT: r tiles of 16 the accumulators cover (the call's largest
// r, rounded up to a power of two; a stack's own tiles and k steps are run-time bounds).
template <int DT, int MB, int RT>
__global__ __launch_bounds__(64 * nf4lora::kMaxWaves) void nf4_lora_routed_kernel(const RoutedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr uint32_t kRows = 16 * MB, kCols = 16 * RT, kKS = RT == 1 ? 1 : RT / 2;
    constexpr uint32_t kPS = kCols + nf4lora::kPartPad;  // floats between rows of the partials
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, W = blockDim.x >> 6;
    const uint32_t lr = lane & 15u, lh = lane >> 4;
    uint32_t mi = 0;
    for (uint32_t i = 1; i < a.nstack; ++i) mi = blockIdx.x >= a.m[i].tile0 ? i : mi;
    const RoutedStack& m = a.m[mi];
    const uint32_t M = a.M, K = a.K, S = a.S, r = m.r, ts = a.ts;
    const uint32_t local = blockIdx.x - m.tile0, slot = local / m.tiles, tile = local - slot * m.tiles;
    const uint32_t n_begin = tile * a.tile_n;

    // the routing: every wave reads all M ids (in-bounds repeats past M)
    const uint32_t p0 = lane, p1 = lane + 64u;
    const int32_t id0 = a.ids[p0 < M ? p0 : M - 1u], id1 = a.ids[p1 < M ? p1 : M - 1u];
    const bool in0 = p0 < M, in1 = p1 < M;
    const bool ok0 = in0 && (uint32_t)id0 < S, ok1 = in1 && (uint32_t)id1 < S;  // S <= 64
    const uint64_t b0 = ok0 ? uint64_t(1) << id0 : 0u, b1 = ok1 ? uint64_t(1) << id1 : 0u;
    uint64_t present = (uint64_t)wave_or((uint32_t)(b0 | b1)) | (uint64_t)wave_or((uint32_t)((b0 | b1) >> 32)) << 32;

    if (slot == 0u && m.base != m.y) {  // rows without an adapter: the base, or zeros, in this tile's columns
        const uint64_t z0 = __ballot(in0 && !ok0), z1 = __ballot(in1 && !ok1);
        const uint32_t n_end = min(n_begin + a.tile_n, m.N);
        for (int h = 0; h < 2; ++h)
            for (uint64_t b = h ? z1 : z0; b; b &= b - 1u) {
                const size_t row = (size_t)((uint32_t)__builtin_ctzll(b) + 64u * (uint32_t)h) * m.N;
                for (uint32_t n = n_begin + 4u * tid; n < n_end; n += 4u * blockDim.x)  // N % 16 == 0: 8 bytes whole and aligned
                    *reinterpret_cast<u32x2*>(m.y + row + n) = m.base ? *reinterpret_cast<const u32x2*>(m.base + row + n) : u32x2{0u, 0u};
            }
    }
    if (slot >= (uint32_t)__popcll(present)) return;  // fewer adapters present than slots: nothing of x, A or B is loaded

    for (uint32_t i = 0; i < slot; ++i) present &= present - 1u;
    const uint32_t ad = (uint32_t)__builtin_ctzll(present);  // the slot-th smallest adapter present
    const uint64_t m0 = __ballot(ok0 && (uint32_t)id0 == ad), m1 = __ballot(ok1 && (uint32_t)id1 == ad);
    const uint32_t cnt0 = (uint32_t)__popcll(m0), cnt = cnt0 + (uint32_t)__popcll(m1);  // >= 1

    const char* Aad = m.A + (size_t)ad * m.a_bytes;
    const char* Bad = m.B + (size_t)ad * m.b_bytes;
    const float scale = m.scale[ad];
    const uint32_t rtiles = (r + 15u) >> 4, ksteps = (r + 31u) >> 5;
    uint16_t* t = reinterpret_cast<uint16_t*>(lds);
    float* part = reinterpret_cast<float*>(lds + a.t_bytes);
    uint32_t* rows = reinterpret_cast<uint32_t*>(lds + a.t_bytes + a.part_bytes);  // list position -> row of x and y

    // t starts as zeros: the columns from r to the MFMA depth are never written again
    for (uint32_t i = tid * 16u; i < a.t_bytes; i += blockDim.x * 16u) *reinterpret_cast<u32x4*>(lds + i) = u32x4{0, 0, 0, 0};
    if (wave == 0u) {  // the adapter's ascending row list, by popcount prefix
        const uint64_t below = (uint64_t(1) << lane) - 1u;
        if ((m0 >> lane) & 1u) rows[__popcll(m0 & below)] = p0;
        if ((m1 >> lane) & 1u) rows[cnt0 + (uint32_t)__popcll(m1 & below)] = p1;
    }
    __syncthreads();  // the row list, ahead of the first gather

    // ---- shrink ----
    const uint32_t chunks = K >> 5, cpw = (chunks + W - 1) / W;
    const uint32_t c0 = min(wave * cpw, chunks), c1 = min(c0 + cpw, chunks);
    const uint32_t row_blocks = (cnt + kRows - 1u) / kRows;
    for (uint32_t rb = 0; rb < row_blocks; ++rb) {
        f32x4 acc[MB][RT];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[mb][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // Every load is unconditional -- a lane past the list or r reads the first listed row or
        // row 0 of A and its fragment is zeroed in registers -- and kU chunks are loaded per step, so
        // that a step's loads are all in flight before its first MFMA waits for one.  A chunk past
        // the wave's range re-reads the last one and takes no part in the sum (not even as a zero
        // operand: the x it re-read may hold an infinity, and inf * 0 is NaN): the order of the
        // sum stays c0, c0 + 1, ..
        constexpr uint32_t kU = RT >= 8 ? 2 : 4;
        const u32x4 zero = {0, 0, 0, 0};
        const char* xp[MB];
        bool xin[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const uint32_t li = rb * kRows + 16u * mb + lr;
            xin[mb] = li < cnt;
            xp[mb] = a.x + ((size_t)rows[xin[mb] ? li : 0u] * K + 8u * lh) * 2u;
        }
        const char* ap[RT];
        bool ain[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t j = 16u * rt + lr;
            ain[rt] = j < r;
            ap[rt] = Aad + ((size_t)(ain[rt] ? j : 0u) * K + 8u * lh) * 2u;
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
    const uint32_t strips = a.tile_n >> 4, mtiles = (cnt + 15u) >> 4;
    for (uint32_t s = wave; s < strips; s += W) {
        const uint32_t n0 = n_begin + 16u * s;
        if (n0 >= m.N) break;  // N % 16 == 0: a strip is whole or absent
        u32x4 bf[kKS];
#pragma unroll
        for (uint32_t ks = 0; ks < kKS; ++ks) {
            const uint32_t j = 32u * ks + 8u * lh;
            bf[ks] = j < r ? ld16(Bad + ((size_t)(n0 + lr) * r + j) * 2u) : u32x4{0, 0, 0, 0};
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
                const uint32_t li = 16u * mt + 4u * lh + g;
                if (li < cnt) {
                    const size_t at = (size_t)rows[li] * m.N + n0 + lr;
                    const float u = up16<DT>(rn16<DT>(acc[g]));
                    uint16_t out = rn16<DT>(u * scale);
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
int launch(const RoutedPlan& p, const RoutedArgs& A, hipStream_t st) {
    static bool attr[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (p.dyn > 64u * 1024u && (dev < 0 || !attr[dev])) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&nf4_lora_routed_kernel<DT, MB, RT>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)nf4lora::kLdsPerCu);
        if (e != hipSuccess) return hip_rc(e);
        if (dev >= 0) attr[dev] = true;
    }
    hipLaunchKernelGGL((nf4_lora_routed_kernel<DT, MB, RT>), dim3(p.grid), dim3(p.block), p.dyn, st, A);
    return hip_rc(hipGetLastError());
}

template <int DT, int MB>
int launch_rt(const RoutedPlan& p, const RoutedArgs& A, hipStream_t st) {
    switch (p.rt) {
        case 1: return launch<DT, MB, 1>(p, A, st);
        case 2: return launch<DT, MB, 2>(p, A, st);
        case 4: return launch<DT, MB, 4>(p, A, st);
        default: return launch<DT, MB, 8>(p, A, st);
    }
}

}  // namespace

extern "C" int nf4_lora_add_routed(const void* x, const void* adapter_ids, int64_t M, int64_t K, int32_t adapters,
                                   const void* stacks, int32_t count, int32_t dtype, const void* cfg, void* hip_stream) {
    const nf4_lora_stack* hs = reinterpret_cast<const nf4_lora_stack*>(stacks);
    const nf4lora::RoutedCall call{x, adapter_ids, M, K, adapters, hs, count, dtype, reinterpret_cast<const nf4_lora_cfg*>(cfg)};
    int rc = nf4lora::routed_validate(call);  // every rule answers before any device work
    if (rc) return rc;
    nf4_lora_cfg c{};
    rc = nf4lora::routed_check(call, call.cfg ? 0 : device_cus(), &c);
    if (rc) return rc;
    const RoutedPlan p = nf4lora::routed_plan(c, M, adapters, hs, count);
    RoutedArgs A{};
    A.x = reinterpret_cast<const char*>(x);
    A.ids = reinterpret_cast<const int32_t*>(adapter_ids);
    A.M = (uint32_t)M;
    A.K = (uint32_t)K;
    A.S = (uint32_t)adapters;
    A.nstack = (uint32_t)count;
    A.tile_n = p.tile_n;
    A.ts = p.ts;
    A.t_bytes = p.t_bytes;
    A.part_bytes = p.part_bytes;
    for (int32_t i = 0; i < count; ++i)
        A.m[i] = RoutedStack{reinterpret_cast<const char*>(hs[i].A), reinterpret_cast<const char*>(hs[i].B), hs[i].scale,
                             reinterpret_cast<const uint16_t*>(hs[i].base), reinterpret_cast<uint16_t*>(hs[i].y),
                             (uint64_t)hs[i].a_stride * 2u, (uint64_t)hs[i].b_stride * 2u, (uint32_t)hs[i].N, (uint32_t)hs[i].r,
                             p.tile0[i], (p.tile0[i + 1] - p.tile0[i]) / p.slots};
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (dtype == NF4DQ_BF16) return p.mb == 1 ? launch_rt<NF4DQ_BF16, 1>(p, A, st) : launch_rt<NF4DQ_BF16, 2>(p, A, st);
    return p.mb == 1 ? launch_rt<NF4DQ_F16, 1>(p, A, st) : launch_rt<NF4DQ_F16, 2>(p, A, st);
}
