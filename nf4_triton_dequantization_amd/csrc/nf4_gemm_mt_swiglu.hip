// nf4_gemm_mt_swiglu.hip -- the fused gate/up SwiGLU launch in bitsandbytes semantics for
// 1..128 rows (nf4_gemm_bnb_mt_swiglu): kernel, launcher and C entries.  The plan --
// validation, cfg, geometry, LDS, workspace -- is nf4_gemm_mt_swiglu_plan.h.
//
// h[M][I] = silu(g) * u with g = x . Wg^T and u = x . Wu^T what nf4_gemm_bnb_mt stores for each
// weight (fp32 accumulation, one RNE to 16 bits), and the rounding chain of
// `F.silu(gate(x)) * up(x)` on 16-bit tensors behind them:
//   s = RNE16(g / (1 + expf(-g)))   fp32, IEEE division        h = RNE16(s * u)   fp32 product
// The anatomy is the row-tiled kernel's (nf4_gemm_mt.hip: x staged per 128-deep chunk in two
// rotated LDS buffers, loads clamped in bounds and never branched around, the weights three
// chunks ahead in registers, the exact 16-bit decode, MFMA 16x16x32), with the wave's two
// strips given to the two weights:
//  * a workgroup (WV waves) owns 16 WV columns of h, ALL MT row tiles and one K slice;
//  * a wave owns 16 columns of h: strip 0 is rows col .. col + 15 of the gate weight, strip 1
//    the same rows of the up weight, each with its own statistics, code2 table (two tables in
//    LDS), offset and blocksize2.  acc[mt][0][i] and acc[mt][1][i] are g and u of ONE output
//    element in one lane, so the epilogue is lane-local and the register budget the parent's.
// Split-K: every slice stores both fp32 planes to its slab ([ksplit][2][M][I]), then the
// release, the ticket and the acquire of the row-tiled kernel: one ticket per column tile,
// nobody waits.  The last slice sums each plane in slice order, applies the chain, stores h and
// puts the slabs and the ticket back to 0.
#include "nf4_gemm_launch.h"
#include "nf4_gemm_mt_swiglu_plan.h"

namespace {

struct SgArgs {
    const uint8_t* packed[2];  // gate, up: [I][K/2]
    const uint8_t* a1[2];      // nested: absmax bytes [I K / 64]
    const float* a2[2];        // nested: absmax2; single: the fp32 absmax
    const float* code2[2];     // nested: [256]
    const float* offset[2];    // nested: [1] or null (= 0)
    const void* x;             // [M][K]
    void* h;                   // [M][I]
    float* slab;               // [ksplit][2][M][I] (ksplit > 1)
    uint32_t* counters;        // one ticket per column tile
    uint32_t M, I, K;
    uint32_t ksplit, cps, chunks;  // K slices, chunks per slice, K / 128
    uint32_t sh2[2];           // log2(blocksize2)
};

// One chunk of a lane's two strips: the packed bytes and the raw statistics.
struct SgW {
    u32x4 w[2];
    uint32_t qa[2];
    float qb[2];
};

// Slot rotation of a staged row (nf4_gemm_mt.hip).
__device__ __forceinline__ uint32_t sg_rot(uint32_t row) { return (row & 3u) | ((row & 4u) << 1); }

// RNE to the 16-bit type and back.  (opaque: the backend must not fold the rounding into the
// operation before it -- v_fma_mix rounds once where the chain rounds twice)
template <int DT>
__device__ __forceinline__ float rne16(float v) {
    if constexpr (DT == NF4DQ_BF16) return (float)(__bf16)opaque(v);
    else return (float)(_Float16)opaque(v);
}

// The chain behind the two 16-bit GEMM results: fp32 silu with IEEE division, one rounding,
// the (exact) fp32 product, one rounding.  Returns h widened to fp32.
template <int DT>
__device__ __forceinline__ float swiglu16(float acc_g, float acc_u) {
    const float g = rne16<DT>(acc_g), u = rne16<DT>(acc_u);
    const float s = rne16<DT>(g / (1.0f + expf(-g)));
    return rne16<DT>(s * u);
}

template <int DT, int MT, int SM, int WV>
__global__ __launch_bounds__(64 * WV) void nf4_gemm_mt_swiglu_kernel(const SgArgs A) {
    constexpr uint32_t T = 64u * WV;
    constexpr uint32_t kBuf = 16u * MT * kMtRowBytes;
    constexpr int NP = 16 * MT * 16 / (int)T;  // 16-byte pieces of a stage per thread
    constexpr uint32_t COLS = 16u * WV;        // columns of h per workgroup
    static_assert(16 * MT * 16 % T == 0, "a stage divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2 gate][code2 up][codes][flag]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * kBuf);
    float* lut = c2tab + 512;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t ks = blockIdx.x % A.ksplit, tile = blockIdx.x / A.ksplit;
    const uint32_t col0 = tile * COLS + wave * 16u;
    const uint32_t c_begin = ks * A.cps < A.chunks ? ks * A.cps : A.chunks;
    const uint32_t c_end = c_begin + A.cps < A.chunks ? c_begin + A.cps : A.chunks;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;

    if constexpr (SM == kScaleBnb)
        for (uint32_t i = tid; i < 256u; i += T) {
            c2tab[i] = A.code2[0][i];
            c2tab[256u + i] = A.code2[1][i];
        }
    write_lut(lut);
    const float off[2] = {load_offset<SM>(A.offset[0]), load_offset<SM>(A.offset[1])};

    // Loads run ahead of the MFMAs in registers: the weights (HBM) kWD chunks, x (L2) two.
    // Slots are compile-time (the chunk loop is unrolled by kWD), chunk numbers past the
    // slice's end are clamped to its last chunk -- a repeated load, never a branch, so the
    // compiler's wait counts stay exact.
    // (two-wave workgroups with 6 or 8 row tiles stage 12 or 16 pieces per thread, and eight
    // row tiles need their registers for the MFMA operands: one register set, x one chunk
    // ahead in two halves, or the sets would spill)
    constexpr int kWD = 4;
    constexpr int kXS = NP > 8 || MT >= 8 ? 1 : 2;
    constexpr int NPR = kXS == 2 ? NP : NP / 2;  // one set: the stage in two halves, half the registers
    u32x4 xr[kXS][NPR];
    SgW w[kWD];
    const uint32_t n = c_end - c_begin;  // chunks of this slice
    auto chunk_at = [&](uint32_t i) { return c_begin + (i < n ? i : n - 1u); };
    // (rows >= M load row M - 1 again and are zeroed on their way into LDS: an in-bounds repeat,
    // no branch around a load, so the compiler counts the loads in flight exactly)
    auto xload = [&](auto S, uint32_t c, int half = 0) {
        const char* xg = reinterpret_cast<const char*>(A.x);
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const uint32_t p = tid + (uint32_t)(i + half * NPR) * T, row = p >> 4, seg = p & 15u;
            const uint32_t r = row < A.M ? row : A.M - 1u;
            xr[S][i] = *reinterpret_cast<const u32x4*>(xg + (r * A.K + c * kChunkK + seg * 8u) * 2u);  // < 2^31: validated
        }
    };
    auto xstore = [&](auto S, char* buf, int half = 0) {
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const uint32_t p = tid + (uint32_t)(i + half * NPR) * T, row = p >> 4, seg = p & 15u;
            const u32x4 v = row < A.M ? xr[S][i] : u32x4{0u, 0u, 0u, 0u};  // rows >= M: zeros in LDS
            *reinterpret_cast<u32x4*>(buf + row * kMtRowBytes + ((seg + sg_rot(row)) & 15u) * 16u) = v;
        }
    };
    // strip nt is weight nt (0 gate, 1 up): the same row of both, col0 + nl < I
    const uint32_t r = col0 + nl;
    auto wload = [&](auto S, uint32_t c) {
        const uint32_t f = r * bpr + 2u * c + (kh >> 1);  // 64-block on the weight's flat stream
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            w[S].w[nt] = *reinterpret_cast<const u32x4*>(A.packed[nt] + (r * kb + c * 64u + 16u * kh));  // < 2^31: validated
            if constexpr (SM == kScaleBnb) {
                w[S].qa[nt] = A.a1[nt][f];
                w[S].qb[nt] = A.a2[nt][f >> A.sh2[nt]];
            } else {
                w[S].qa[nt] = 0u;
                w[S].qb[nt] = A.a2[nt][f];
            }
        }
    };

    f32x4 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    if (n > 0u) {
        xload(I0{}, chunk_at(0));
        wload(I0{}, chunk_at(0));
        if constexpr (kXS == 2) xload(I1{}, chunk_at(1));
        wload(I1{}, chunk_at(1));
        wload(I2{}, chunk_at(2));
        xstore(I0{}, smem);
        if constexpr (kXS == 2) xload(I0{}, chunk_at(2));
        else {
            xload(I0{}, chunk_at(0), 1);
            xstore(I0{}, smem, 1);
        }
    }
    __syncthreads();  // the tables and the first stage

    const char* t = reinterpret_cast<const char*>(lut);
    const uint32_t rot = sg_rot(nl);  // row 16 mt + nl: the rotation depends on nl alone
    // chunk i of the slice (slot J = i % kWD): x[i] is in LDS buffer i & 1, x[i + 1] and
    // x[i + 2] in registers or in flight (set = chunk & 1; one set: x[i + 1] is loaded here),
    // the weights of i .. i + 2 in flight or landed
    auto step = [&](auto J, uint32_t i) {
        constexpr int j = decltype(J)::value;
        const char* buf = smem + (uint32_t)(j & 1) * kBuf;
        wload(std::integral_constant<int, (j + 3) % kWD>{}, chunk_at(i + 3u));
        if constexpr (kXS == 1) xload(I0{}, chunk_at(i + 1u));
        const SgW& cur = w[j];
        float sc[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) sc[nt] = block_scale<SM>(c2tab + 256 * nt, cur.qa[nt], cur.qb[nt], off[nt]);
        // One wave per SIMD: the x fragments and the decoded weights of MFMA step s + 1 are
        // fetched and made while the MFMAs of step s run (two sets of each).
        auto aread = [&](u32x4(&a)[MT], int s) {
            const uint32_t slot = ((4u * kh + (uint32_t)s + rot) & 15u) * 16u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                a[mt] = *reinterpret_cast<const u32x4*>(buf + (16u * mt + nl) * kMtRowBytes + slot);
        };
        auto decode = [&](u32x4(&bw)[2], int s) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const uint32_t wd = cur.w[nt][s];
                const uint32_t hi4 = (wd >> 2) & 0x3C3C3C3Cu;
                const uint32_t lo4 = (wd << 2) & 0x3C3C3C3Cu;
                float v[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[2 * k] = *reinterpret_cast<const float*>(t + ((hi4 >> (8 * k)) & 0xFFu)) * sc[nt];
                    v[2 * k + 1] = *reinterpret_cast<const float*>(t + ((lo4 >> (8 * k)) & 0xFFu)) * sc[nt];
                }
                // the exact weights nf4_dequant_bnb writes: fp32 product, RNE to 16 bits
                bw[nt] = u32x4{pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]), pack2<DT>(v[4], v[5]), pack2<DT>(v[6], v[7])};
            }
        };
        // (eight row tiles: one set of x fragments, read at the head of their own step -- two
        // sets would spill -- with the next step's decode between the reads and their MFMAs)
        constexpr int kAF = MT >= 8 ? 1 : 2;
        u32x4 af[kAF][MT], bw[2][2];
        if constexpr (kAF == 2) aread(af[0], 0);
        decode(bw[0], 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (kAF == 1) {
                aread(af[0], s);
                __builtin_amdgcn_sched_barrier(0);  // the batch is issued here, not where it is used
            }
            if (s < 3) {
                if constexpr (kAF == 2) {
                    aread(af[(s + 1) & 1], s + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                decode(bw[(s + 1) & 1], s + 1);
            }
            if constexpr (kXS == 1)
                if (s == 2) {  // first half of x[i + 1] lands in the other buffer, the second half sets out
                    xstore(I0{}, smem + (uint32_t)((j + 1) & 1) * kBuf, 0);
                    xload(I0{}, chunk_at(i + 1u), 1);
                }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    if constexpr (DT == NF4DQ_BF16)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8, af[s & (kAF - 1)][mt]), __builtin_bit_cast(bf16x8, bw[s & 1][nt]),
                            acc[mt][nt], 0, 0, 0);
                    else
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            __builtin_bit_cast(f16x8, af[s & (kAF - 1)][mt]), __builtin_bit_cast(f16x8, bw[s & 1][nt]),
                            acc[mt][nt], 0, 0, 0);
                }
            }
        }
        // x[i + 1] (loaded one chunk ago) into the other buffer, last read one barrier ago; its
        // registers then take x[i + 2]
        constexpr int xs = kXS == 2 ? (j + 1) & 1 : 0;
        xstore(std::integral_constant<int, xs>{}, smem + (uint32_t)((j + 1) & 1) * kBuf, kXS == 2 ? 0 : 1);
        if constexpr (kXS == 2) xload(std::integral_constant<int, xs>{}, chunk_at(i + 3u));
        __syncthreads();
    };
    for (uint32_t i = 0; i < n; i += kWD) {
        step(std::integral_constant<int, 0>{}, i);
        if (i + 1u >= n) break;
        step(std::integral_constant<int, 1>{}, i + 1u);
        if (i + 2u >= n) break;
        step(std::integral_constant<int, 2>{}, i + 2u);
        if (i + 3u >= n) break;
        step(std::integral_constant<int, 3>{}, i + 3u);
    }

    // acc[mt][0][i] = g, acc[mt][1][i] = u of h[16 mt + 4 kh + i][col0 + nl]
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
                if (m < A.M) store_y<DT>(A.h, m * A.I + r, swiglu16<DT>(acc[mt][0][i], acc[mt][1][i]));  // exact: a 16-bit value
            }
        return;
    }
    const uint32_t plane = A.M * A.I;  // floats per plane; 2 ksplit planes < 2^30 floats: validated
    float* mine = A.slab + (size_t)ks * 2u * plane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
            if (m < A.M) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) mine[(uint32_t)nt * plane + m * A.I + r] = acc[mt][nt][i];
            }
        }
    // publish: every wave's stores done, then ONE agent-scope release ahead of the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(A.counters + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = ticket == A.ksplit - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(A.counters + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next call
        }
        *flag = last ? 1u : 0u;
    }
    __syncthreads();
    if (*flag == 0u) return;
    // the reducer: every slice's tile of both planes in slice order, 4 columns per thread and
    // element, cleared behind it.  A thread's loads of one slice (its kE elements of each plane)
    // are in flight together, so the tile costs one round trip per slice; each element's sum
    // still runs in slice order.  Elements past the tile repeat its last one (an in-bounds
    // load, no branch) and are not stored.
    constexpr int kE = 16 * MT * (int)(COLS / 4u) / (int)T;  // elements per thread and plane at 16 MT rows
    const uint32_t total = A.M * (COLS / 4u);
    uint32_t at[kE];
    f32x4 sum[kE][2];
#pragma unroll
    for (int j = 0; j < kE; ++j) {
        const uint32_t e0 = tid + (uint32_t)j * T, e = e0 < total ? e0 : total - 1u;
        at[j] = (e / (COLS / 4u)) * A.I + tile * COLS + 4u * (e % (COLS / 4u));
    }
    for (uint32_t sl = 0; sl < A.ksplit; ++sl) {
        f32x4 v[kE][2];
#pragma unroll
        for (int j = 0; j < kE; ++j)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                v[j][nt] = *reinterpret_cast<const f32x4*>(A.slab + (2u * sl + (uint32_t)nt) * plane + at[j]);
#pragma unroll
        for (int j = 0; j < kE; ++j)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                if (sl == 0u) sum[j][nt] = v[j][nt];  // the first slice starts the sum: -0 stays -0
                else {
                    sum[j][nt].x += v[j][nt].x;
                    sum[j][nt].y += v[j][nt].y;
                    sum[j][nt].z += v[j][nt].z;
                    sum[j][nt].w += v[j][nt].w;
                }
            }
    }
#pragma unroll
    for (int j = 0; j < kE; ++j)
        if (tid + (uint32_t)j * T < total) {
            for (uint32_t sl = 0; sl < 2u * A.ksplit; ++sl)
                *reinterpret_cast<f32x4*>(A.slab + sl * plane + at[j]) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 g = sum[j][0], u = sum[j][1];
            u32x2* dst = reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.h) + at[j]);
            *dst = u32x2{pack2<DT>(swiglu16<DT>(g.x, u.x), swiglu16<DT>(g.y, u.y)),
                         pack2<DT>(swiglu16<DT>(g.z, u.z), swiglu16<DT>(g.w, u.w))};
        }
}

template <int SM>
int launch_sg(const nf4gemm::SgCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const int64_t I = a.mats[0].N;
    const MtPlan p = sg_plan(cfg, a.M, I, a.K);
    SgArgs A{};
    for (int i = 0; i < 2; ++i) {
        const nf4_gemm_bnb_mat& m = a.mats[i];
        A.packed[i] = m.packed;
        A.a1[i] = a.single ? nullptr : m.absmax_q;
        A.a2[i] = m.absmax2;
        A.code2[i] = a.single ? nullptr : m.code2;
        A.offset[i] = a.single ? nullptr : m.offset;
        while (!a.single && (1 << A.sh2[i]) < m.blocksize2) ++A.sh2[i];
    }
    A.x = a.x;
    A.h = a.h;
    A.counters = reinterpret_cast<uint32_t*>(a.workspace);
    A.slab = cfg.ksplit > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(a.workspace) + kHeaderBytes) : nullptr;
    A.M = (uint32_t)a.M;
    A.I = (uint32_t)I;
    A.K = (uint32_t)a.K;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.cps = p.cps;
    A.chunks = p.chunks;
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_mt_swiglu_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_mt_swiglu_workspace_bytes(int64_t M, int64_t I, int64_t K, const nf4_gemm_cfg* cfg) {
    return sg_workspace_need(M, I, K, cfg ? *cfg : sg_default_cfg(M, I, K, device_cus()));
}

int nf4_gemm_bnb_mt_swiglu(const void* x, int64_t M, int64_t K, const void* gate_up, int32_t single, int32_t act,
                           void* h, int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                           void* hip_stream) {
    const nf4gemm::SgCall a{single != 0, x,         M,         K,               reinterpret_cast<const nf4_gemm_bnb_mat*>(gate_up),
                            act,         h,         out_dtype, workspace,       workspace_bytes,
                            cfg};
    nf4_gemm_cfg c{};
    const int rc = sg_check(a, device_cus(), &c);
    if (rc) return rc;
    const hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.single ? launch_sg<kScaleBnbSingle>(a, c, st) : launch_sg<kScaleBnb>(a, c, st);
}

}  // extern "C"
