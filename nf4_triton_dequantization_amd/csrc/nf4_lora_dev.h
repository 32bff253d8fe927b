// nf4_lora_dev.h -- what the two adapter launches share beside the plan: the 16-bit helpers, the
// one kernel template lora_kernel<DT, MB, RT, ROUTED, Args> -- nf4_lora.hip instantiates it over all
// M rows in order, nf4_lora_routed.hip with the routing prologue, over the rows that lists in LDS --
// and the host helpers that launch it.  None of the GEMM families' headers.
//
// Shrink: the workgroup forms its adapter's whole t = rn(x A^T) with
// v_mfma_f32_16x16x32_{bf16,f16}, x rows as the A operand and rows of the adapter's A as the B
// operand (both are 16 contiguous bytes per lane in their natural layout), the K / 32 chunks split
// into one contiguous range per wave; the waves' fp32 partials meet in LDS and are summed in wave
// order, rounded once to 16 bits into the t image.  Expand: wave w takes the strips w, w + waves,
// .. of 16 columns; t from LDS is the A operand, rows of the adapter's B the B operand; the
// epilogue (rn, * scale, rn, + base, rn) runs in registers and each lane reads and writes its own
// four elements per row tile.  MFMA rows are independent and both launches run these statements,
// so a row's bits from the routed launch are those nf4_lora_add stores for it with the same
// adapter and waves.  The kernel itself holds the statements (no shared callee): a body inlined
// from a function compiles to other code than the same statements in the kernel, and measurably
// slower code in some instantiations (profiles/lora_family/README.md).
#pragma once

#include <type_traits>

#include "nf4_common.h"
#include "nf4_lora_plan.h"

namespace nf4lora {

using namespace nf4dq;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// t starts as zeros: the columns from r to the MFMA depth are never written again
__device__ __forceinline__ void lora_zero_t(char* lds, uint32_t t_bytes) {
    for (uint32_t i = threadIdx.x * 16u; i < t_bytes; i += blockDim.x * 16u) *reinterpret_cast<u32x4*>(lds + i) = u32x4{0, 0, 0, 0};
}

// List position -> row of x and y: the position itself, or the list's entry; a position past the
// end (`in` false) reads the first row.
template <bool ROUTED>
__device__ __forceinline__ uint32_t lora_row(const uint32_t* rows, uint32_t li, bool in) {
    if constexpr (ROUTED) return rows[in ? li : 0u];
    else return in ? li : 0u;
}

// The OR of a 32-bit value over the wave, the same in every lane.
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The one kernel of both adapter launches, over the launch's argument struct (nf4_lora.hip,
// nf4_lora_routed.hip: x, M, K, nmat, tile_n, ts, t_bytes and the per-matrix entries m[] with A, B,
// base, y, N, r, tile0).  ROUTED = false: one workgroup per (adapter, tile of tile_n columns) over
// all M rows, row li is row li; no row list, no barrier of its own.  ROUTED = true: one workgroup
// per (stack, slot, tile); the routing prologue finds the slot's adapter and lists its rows in LDS,
// and the shrink gathers and the expand scatters through the list.  MB: row tiles of 16 per row
// block; RT: r tiles of 16 the accumulators cover (the call's largest r, rounded up to a power of
// two; a matrix's own tiles and k steps are run-time bounds).
template <int DT, int MB, int RT, bool ROUTED, class Args>
__global__ __launch_bounds__(64 * kMaxWaves) void lora_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr uint32_t kRows = 16 * MB, kCols = 16 * RT, kKS = RT == 1 ? 1 : RT / 2;
    constexpr uint32_t kPS = kCols + kPartPad;  // floats between rows of the partials
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, W = blockDim.x >> 6;
    const uint32_t lr = lane & 15u, lh = lane >> 4;
    uint32_t mi = 0;
    for (uint32_t i = 1; i < a.nmat; ++i) mi = blockIdx.x >= a.m[i].tile0 ? i : mi;
    const auto& m = a.m[mi];
    const uint32_t M = a.M, K = a.K, r = m.r, ts = a.ts;
    const uint32_t rtiles = (r + 15u) >> 4, ksteps = (r + 31u) >> 5;
    uint16_t* t = reinterpret_cast<uint16_t*>(lds);
    float* part;  // behind t; set in each arm below, at the place that keeps the launch's code (see there)

    // What the routing finds: the rows of the slot's adapter (list position -> row of x and y, in
    // LDS behind t and the partials), their count, the adapter's matrices and scale, the first
    // column.  Its order is fixed: the ids, the adapters present, slot 0's store of the rows without
    // an adapter, the idle slot's return, the row list, one barrier.
    const uint32_t* rows = nullptr;
    uint32_t cnt = 0, n_routed = 0;
    const char *Aad = nullptr, *Bad = nullptr;
    float scale_ad = 0.f;
    // The routing's values that are alive at the idle slot's return are declared here, not in the
    // block: a return out of a block with live locals leaves through that block's end, the idle
    // path then rejoins behind the barrier and is tested again, and the compiler lays the whole
    // kernel out in another order -- 0.4 % to 2.5 % slower at a quarter of the measured points.
    // Likewise `part` is set and `row_blocks` computed where each launch had them before the two
    // kernels were one.  With these three, all 32 instantiations compile to the instruction
    // streams of the two kernels this template replaced (profiles/lora_family/README.md).
    uint32_t S, local, slot, tile, p0, p1;
    int32_t id0, id1;
    bool in0, in1, ok0, ok1;
    uint64_t b0, b1, present;
    if constexpr (ROUTED) {
        S = a.S;
        local = blockIdx.x - m.tile0, slot = local / m.tiles, tile = local - slot * m.tiles;
        n_routed = tile * a.tile_n;

        // every wave reads all M ids (in-bounds repeats past M)
        p0 = lane, p1 = lane + 64u;
        id0 = a.ids[p0 < M ? p0 : M - 1u], id1 = a.ids[p1 < M ? p1 : M - 1u];
        in0 = p0 < M, in1 = p1 < M;
        ok0 = in0 && (uint32_t)id0 < S, ok1 = in1 && (uint32_t)id1 < S;  // S <= 64
        b0 = ok0 ? uint64_t(1) << id0 : 0u, b1 = ok1 ? uint64_t(1) << id1 : 0u;
        present = (uint64_t)wave_or((uint32_t)(b0 | b1)) | (uint64_t)wave_or((uint32_t)((b0 | b1) >> 32)) << 32;

        if (slot == 0u && m.base != m.y) {  // rows without an adapter: the base, or zeros, in this tile's columns
            const uint64_t z0 = __ballot(in0 && !ok0), z1 = __ballot(in1 && !ok1);
            const uint32_t n_end = min(n_routed + a.tile_n, m.N);
            for (int h = 0; h < 2; ++h)
                for (uint64_t b = h ? z1 : z0; b; b &= b - 1u) {
                    const size_t row = (size_t)((uint32_t)__builtin_ctzll(b) + 64u * (uint32_t)h) * m.N;
                    for (uint32_t n = n_routed + 4u * tid; n < n_end; n += 4u * blockDim.x)  // N % 16 == 0: 8 bytes whole and aligned
                        *reinterpret_cast<u32x2*>(m.y + row + n) = m.base ? *reinterpret_cast<const u32x2*>(m.base + row + n) : u32x2{0u, 0u};
                }
        }
        if (slot >= (uint32_t)__popcll(present)) return;  // fewer adapters present than slots: nothing of x, A, B or scale is loaded

        for (uint32_t i = 0; i < slot; ++i) present &= present - 1u;
        const uint32_t ad = (uint32_t)__builtin_ctzll(present);  // the slot-th smallest adapter present
        const uint64_t m0 = __ballot(ok0 && (uint32_t)id0 == ad), m1 = __ballot(ok1 && (uint32_t)id1 == ad);
        const uint32_t cnt0 = (uint32_t)__popcll(m0);
        cnt = cnt0 + (uint32_t)__popcll(m1);  // >= 1
        Aad = m.A + (size_t)ad * m.a_bytes;
        Bad = m.B + (size_t)ad * m.b_bytes;
        scale_ad = m.scale[ad];
        part = reinterpret_cast<float*>(lds + a.t_bytes);
        uint32_t* list = reinterpret_cast<uint32_t*>(lds + a.t_bytes + a.part_bytes);
        rows = list;

        lora_zero_t(lds, a.t_bytes);
        if (wave == 0u) {  // the adapter's ascending row list, by popcount prefix
            const uint64_t below = (uint64_t(1) << lane) - 1u;
            if ((m0 >> lane) & 1u) list[__popcll(m0 & below)] = p0;
            if ((m1 >> lane) & 1u) list[cnt0 + (uint32_t)__popcll(m1 & below)] = p1;
        }
        __syncthreads();  // the row list, ahead of the first gather
    } else {
        part = reinterpret_cast<float*>(lds + a.t_bytes);
        lora_zero_t(lds, a.t_bytes);
    }
    const uint32_t nrows = ROUTED ? cnt : M;

    // ---- shrink ----
    const uint32_t chunks = K >> 5, cpw = (chunks + W - 1) / W;
    const uint32_t c0 = min(wave * cpw, chunks), c1 = min(c0 + cpw, chunks);
    uint32_t row_blocks;
    if constexpr (ROUTED) row_blocks = (cnt + kRows - 1u) / kRows;
    else row_blocks = a.row_blocks;
    for (uint32_t rb = 0; rb < row_blocks; ++rb) {
        f32x4 acc[MB][RT];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[mb][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // Every load is unconditional -- a lane past the rows or r reads the first row and its
        // fragment is zeroed in registers -- and kU chunks are loaded per step, so that a step's
        // loads are all in flight before its first MFMA waits for one: the loop is bound by load
        // latency, not by bytes.  A chunk past the wave's range re-reads the last one and takes no
        // part in the sum (not even as a zero operand: the x it re-read may hold an infinity, and
        // inf * 0 is NaN): the order of the sum stays c0, c0 + 1, ..
        constexpr uint32_t kU = RT >= 8 ? 2 : 4;
        const u32x4 zero = {0, 0, 0, 0};
        const char* xp[MB];
        bool xin[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const uint32_t li = rb * kRows + 16u * mb + lr;
            xin[mb] = li < nrows;
            xp[mb] = a.x + ((size_t)lora_row<ROUTED>(rows, li, xin[mb]) * K + 8u * lh) * 2u;
        }
        const char* ap[RT];
        bool ain[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t j = 16u * rt + lr;
            ain[rt] = j < r;
            ap[rt] = (ROUTED ? Aad : m.A) + ((size_t)(ain[rt] ? j : 0u) * K + 8u * lh) * 2u;
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
    const uint32_t n_begin = ROUTED ? n_routed : (blockIdx.x - m.tile0) * a.tile_n, strips = a.tile_n >> 4, mtiles = (nrows + 15u) >> 4;
    for (uint32_t s = wave; s < strips; s += W) {
        const uint32_t n0 = n_begin + 16u * s;
        if (n0 >= m.N) break;  // N % 16 == 0: a strip is whole or absent
        u32x4 bf[kKS];
#pragma unroll
        for (uint32_t ks = 0; ks < kKS; ++ks) {
            const uint32_t j = 32u * ks + 8u * lh;
            bf[ks] = j < r ? ld16((ROUTED ? Bad : m.B) + ((size_t)(n0 + lr) * r + j) * 2u) : u32x4{0, 0, 0, 0};
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
                if (li < nrows) {
                    const size_t at = (size_t)lora_row<ROUTED>(rows, li, true) * m.N + n0 + lr;
                    const float u = up16<DT>(rn16<DT>(acc[g]));
                    float sc;
                    if constexpr (ROUTED) sc = scale_ad;
                    else sc = m.scale;
                    uint16_t out = rn16<DT>(u * sc);
                    if (m.base) out = rn16<DT>(up16<DT>(m.base[at]) + up16<DT>(out));
                    m.y[at] = out;
                }
            }
        }
    }
}

// ---- host ----

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
// repeats the call), then launch.  The kernel is a template argument: the flags are its own.
template <auto KERNEL, class Args>
int lora_launch(const LoraPlan& p, const Args& A, hipStream_t st) {
    static bool attr[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (p.dyn > 64u * 1024u && (dev < 0 || !attr[dev])) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)kLdsPerCu);
        if (e != hipSuccess) return hip_rc(e);
        if (dev >= 0) attr[dev] = true;
    }
    hipLaunchKernelGGL(KERNEL, dim3(p.grid), dim3(p.block), p.dyn, st, A);
    return hip_rc(hipGetLastError());
}

// The instantiation of a plan: f(DT, MB, RT as std::integral_constant) for dtype, p.mb and p.rt.
template <class F>
int lora_dispatch(int32_t dtype, const LoraPlan& p, F f) {
    auto with_rt = [&](auto dt, auto mb) {
        switch (p.rt) {
            case 1: return f(dt, mb, std::integral_constant<int, 1>{});
            case 2: return f(dt, mb, std::integral_constant<int, 2>{});
            case 4: return f(dt, mb, std::integral_constant<int, 4>{});
            default: return f(dt, mb, std::integral_constant<int, 8>{});
        }
    };
    auto with_mb = [&](auto dt) { return p.mb == 1 ? with_rt(dt, std::integral_constant<int, 1>{}) : with_rt(dt, std::integral_constant<int, 2>{}); };
    return dtype == NF4DQ_BF16 ? with_mb(std::integral_constant<int, NF4DQ_BF16>{}) : with_mb(std::integral_constant<int, NF4DQ_F16>{});
}

}  // namespace nf4lora
