// nf4_gemm_mt.hip -- the row-tiled fused NF4 dequant + GEMM in bitsandbytes semantics for
// 33..128 rows (nf4_gemm_bnb_mt, nf4_gemm_bnb_mt_single): kernel, launcher and C entries.
// The plan -- validation, cfg, geometry, LDS, workspace -- is nf4_gemm_mt_plan.h.
//
// y[M][N] = x[M][K] . W[N][K]^T with W the 16-bit weights nf4_dequant_bnb writes, bit for
// bit.  The families of nf4_gemm_dev.h hold x whole (LDS or registers) and at most two row
// tiles; here M reaches 128, so
//  * a workgroup (WV waves) owns 32 WV columns, ALL MT row tiles and one K slice;
//  * a wave owns two 16-column strips.  Per 128-deep chunk a lane loads 16 packed bytes of
//    its row in each strip (one 64-block, one scale) straight into registers, decodes each
//    dword once into one MFMA B fragment (fp32 product, RNE to 16 bits: the oracle's weight)
//    and multiplies it with every row tile: the decode cost per weight does not grow with M;
//  * x goes through LDS one chunk at a time, two buffers, one barrier per chunk.  Global loads
//    run ahead in registers: the weights (HBM) three chunks, x (L2) two, landing in the other
//    buffer after the current chunk's MFMAs.  An x fragment read (ds_read_b128) feeds the two
//    strips' MFMAs, so the LDS read rate stays at half the MFMA issue rate's demand;
//  * a CU holds one wave per SIMD of this kernel (64 KiB of x buffers at 128 rows, up to 256
//    registers), so the wave hides its own LDS round trips: the x fragments of an MFMA step
//    are read as one batch and the weights of the next step decoded while this step's MFMAs
//    run;
//  * a staged row is one 256-byte bank row; its sixteen 16-byte slots are rotated by
//    (row & 3) | (row & 4) << 1 slots, which puts the 16 lanes of every ds_read_b128 lane
//    group (rows 0-3 / 12-15 of one 32-deep K quarter with rows 4-11 of the next) on 16
//    different slots.  Rows >= M are zeros in LDS (their loads repeat row M - 1, in bounds);
//  * the k permutation of nf4_gemm_dev.h: a lane's packed dword is its B fragment of one
//    MFMA step, and the A fragment is x at the same 8 k, so nothing is shuffled.
// Split-K: every slice stores its fp32 partials to its slab, waits for the stores, and after
// the workgroup barrier one lane releases at agent scope and draws the tile's ticket.  The
// workgroup that draws the last ticket acquires, sums the slabs in slice order, stores y and
// puts the slab and the ticket back to 0.  Nobody waits for anybody: there is no poll.
#include "nf4_gemm_launch.h"
#include "nf4_gemm_mt_plan.h"

namespace {

struct MtArgs {
    const uint8_t* packed;  // [N][K/2]
    const uint8_t* a1;      // nested: absmax bytes [N K / 64]
    const float* a2;        // nested: absmax2; single: the fp32 absmax
    const float* code2;     // nested: [256]
    const float* offset;    // nested: [1] or null (= 0)
    const void* x;          // [M][K]
    void* y;                // [M][N]
    float* slab;            // [ksplit][M][N] (ksplit > 1)
    uint32_t* counters;     // one ticket per column tile
    uint32_t M, N, K;
    uint32_t ksplit, cps, chunks;  // K slices, chunks per slice, K / 128
    uint32_t sh2;           // log2(blocksize2)
};

// One chunk of a lane's two strips: the packed bytes and the raw statistics.
struct MtW {
    u32x4 w[kMtStrips];
    uint32_t qa[kMtStrips];
    float qb[kMtStrips];
};

// Slot rotation of a staged row (see the header comment).
__device__ __forceinline__ uint32_t mt_rot(uint32_t row) { return (row & 3u) | ((row & 4u) << 1); }

template <int DT, int MT, int SM, int WV>
__global__ __launch_bounds__(64 * WV) void nf4_gemm_mt_kernel(const MtArgs A) {
    constexpr uint32_t T = 64u * WV;
    constexpr uint32_t kBuf = 16u * MT * kMtRowBytes;
    constexpr int NP = 16 * MT * 16 / (int)T;  // 16-byte pieces of a stage per thread
    constexpr uint32_t COLS = 32u * WV;
    static_assert(16 * MT * 16 % T == 0, "a stage divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2][codes][flag]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * kBuf);
    float* lut = c2tab + 256;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t ks = blockIdx.x % A.ksplit, tile = blockIdx.x / A.ksplit;
    const uint32_t col0 = tile * COLS + wave * 32u;
    const uint32_t c_begin = ks * A.cps < A.chunks ? ks * A.cps : A.chunks;
    const uint32_t c_end = c_begin + A.cps < A.chunks ? c_begin + A.cps : A.chunks;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;

    if constexpr (SM == kScaleBnb)
        for (uint32_t i = tid; i < 256u; i += T) c2tab[i] = A.code2[i];
    write_lut(lut);
    const float off = load_offset<SM>(A.offset);

    // Loads run ahead of the MFMAs in registers: the weights (HBM) kWD chunks, x (L2) two.
    // Slots are compile-time (the chunk loop is unrolled by kWD), chunk numbers past the
    // slice's end are clamped to its last chunk -- a repeated load, never a branch, so the
    // compiler's wait counts stay exact.
    // (64-column workgroups with 6 or 8 row tiles stage 12 or 16 pieces per thread, and eight
    // row tiles need their registers for the MFMA operands: one register set, x one chunk
    // ahead in two halves, or the sets would spill)
    constexpr int kWD = 4;
    constexpr int kXS = NP > 8 || MT >= 8 ? 1 : 2;
    constexpr int NPR = kXS == 2 ? NP : NP / 2;  // one set: the stage in two halves, half the registers
    u32x4 xr[kXS][NPR];
    MtW w[kWD];
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
            *reinterpret_cast<u32x4*>(buf + row * kMtRowBytes + ((seg + mt_rot(row)) & 15u) * 16u) = v;
        }
    };
    auto wload = [&](auto S, uint32_t c) {
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) {
            const uint32_t r = col0 + 16u * nt + nl;
            w[S].w[nt] = *reinterpret_cast<const u32x4*>(A.packed + (r * kb + c * 64u + 16u * kh));  // < 2^31: validated
            const uint32_t f = r * bpr + 2u * c + (kh >> 1);  // 64-block on the flat stream
            if constexpr (SM == kScaleBnb) {
                w[S].qa[nt] = A.a1[f];
                w[S].qb[nt] = A.a2[f >> A.sh2];
            } else {
                w[S].qa[nt] = 0u;
                w[S].qb[nt] = A.a2[f];
            }
        }
    };

    f32x4 acc[MT][kMtStrips];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

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
    const uint32_t rot = mt_rot(nl);  // row 16 mt + nl: the rotation depends on nl alone
    // chunk i of the slice (slot J = i % kWD): x[i] is in LDS buffer i & 1, x[i + 1] and
    // x[i + 2] in registers or in flight (set = chunk & 1; one set: x[i + 1] is loaded here),
    // the weights of i .. i + 2 in flight or landed
    auto step = [&](auto J, uint32_t i) {
        constexpr int j = decltype(J)::value;
        const char* buf = smem + (uint32_t)(j & 1) * kBuf;
        wload(std::integral_constant<int, (j + 3) % kWD>{}, chunk_at(i + 3u));
        if constexpr (kXS == 1) xload(I0{}, chunk_at(i + 1u));
        const MtW& cur = w[j];
        float sc[kMtStrips];
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) sc[nt] = block_scale<SM>(c2tab, cur.qa[nt], cur.qb[nt], off);
        // One wave per SIMD: nothing hides an LDS round trip but the wave's own MFMAs.  So the
        // x fragments and the decoded weights of MFMA step s + 1 are fetched and made while the
        // MFMAs of step s run (two sets of each), the x fragment reads as one batch.
        auto aread = [&](u32x4(&a)[MT], int s) {
            const uint32_t slot = ((4u * kh + (uint32_t)s + rot) & 15u) * 16u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                a[mt] = *reinterpret_cast<const u32x4*>(buf + (16u * mt + nl) * kMtRowBytes + slot);
        };
        auto decode = [&](u32x4(&bw)[kMtStrips], int s) {
#pragma unroll
            for (int nt = 0; nt < kMtStrips; ++nt) {
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
        u32x4 af[kAF][MT], bw[2][kMtStrips];
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
                for (int nt = 0; nt < kMtStrips; ++nt) {
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

    // acc[mt][nt][i] = y[16 mt + 4 kh + i][col0 + 16 nt + nl]
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
                if (m < A.M) {
#pragma unroll
                    for (int nt = 0; nt < kMtStrips; ++nt) store_y<DT>(A.y, m * A.N + col0 + 16u * nt + nl, acc[mt][nt][i]);
                }
            }
        return;
    }
    float* mine = A.slab + (size_t)ks * A.M * A.N;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
            if (m < A.M) {
#pragma unroll
                for (int nt = 0; nt < kMtStrips; ++nt) mine[m * A.N + col0 + 16u * nt + nl] = acc[mt][nt][i];
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
    // the reducer: every slice's tile in slice order, 4 columns per thread and element, cleared
    // behind it.  The slabs come from other XCDs' stores: a thread's loads of one slice (all its
    // kE elements) are in flight together, so the tile costs one round trip per slice; each
    // element's sum still runs in slice order.  Elements past the tile repeat its last one
    // (an in-bounds load, no branch) and are not stored.
    constexpr int kE = 16 * MT * (int)(COLS / 4u) / (int)T;  // elements per thread at 16 MT rows
    const uint32_t total = A.M * (COLS / 4u);
    const uint32_t sstride = A.M * A.N;  // floats per slab; ksplit slabs < 2^30 floats: validated
    uint32_t at[kE];
    f32x4 sum[kE];
#pragma unroll
    for (int j = 0; j < kE; ++j) {
        const uint32_t e0 = tid + (uint32_t)j * T, e = e0 < total ? e0 : total - 1u;
        at[j] = (e / (COLS / 4u)) * A.N + tile * COLS + 4u * (e % (COLS / 4u));
    }
    for (uint32_t sl = 0; sl < A.ksplit; ++sl) {
        f32x4 v[kE];
#pragma unroll
        for (int j = 0; j < kE; ++j) v[j] = *reinterpret_cast<const f32x4*>(A.slab + sl * sstride + at[j]);
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            if (sl == 0u) sum[j] = v[j];  // the first slice starts the sum: -0 stays -0
            else {
                sum[j].x += v[j].x;
                sum[j].y += v[j].y;
                sum[j].z += v[j].z;
                sum[j].w += v[j].w;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kE; ++j)
        if (tid + (uint32_t)j * T < total) {
            for (uint32_t sl = 0; sl < A.ksplit; ++sl)
                *reinterpret_cast<f32x4*>(A.slab + sl * sstride + at[j]) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            u32x2* dst = reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + at[j]);
            *dst = u32x2{pack2<DT>(sum[j].x, sum[j].y), pack2<DT>(sum[j].z, sum[j].w)};
        }
}

template <int SM>
int launch_mt(const nf4gemm::MtCall& a, const nf4_gemm_cfg& cfg, const float* offset, hipStream_t st) {
    const MtPlan p = mt_plan(cfg, a.M, a.N, a.K);
    MtArgs A{};
    A.packed = a.packed;
    A.a1 = a.a1;
    A.a2 = a.a2;
    A.code2 = a.code2;
    A.offset = offset;
    A.x = a.x;
    A.y = a.y;
    A.counters = reinterpret_cast<uint32_t*>(a.workspace);
    A.slab = cfg.ksplit > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(a.workspace) + kHeaderBytes) : nullptr;
    A.M = (uint32_t)a.M;
    A.N = (uint32_t)a.N;
    A.K = (uint32_t)a.K;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.cps = p.cps;
    A.chunks = p.chunks;
    while (!a.single && (1 << A.sh2) < a.blocksize2) ++A.sh2;
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_mt_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

int gemm_mt_impl(const nf4gemm::MtCall& a, const float* offset, hipStream_t st) {
    nf4_gemm_cfg cfg{};
    const int rc = mt_check(a, device_cus(), &cfg);
    if (rc) return rc;
    return a.single ? launch_mt<kScaleBnbSingle>(a, cfg, nullptr, st) : launch_mt<kScaleBnb>(a, cfg, offset, st);
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_mt_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg) {
    return mt_workspace_need(M, N, K, cfg ? *cfg : mt_default_cfg(M, N, K, device_cus()));
}

int nf4_gemm_bnb_mt(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                    int64_t nb, const float* code2, const float* absmax2, int64_t n2, const float* offset,
                    int32_t blocksize, int32_t blocksize2, void* y, int32_t out_dtype, int64_t N, int64_t K,
                    void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{false, x,          M, packed,    packed_len, absmax_q,  nb, code2,           absmax2, n2,
                            blocksize, blocksize2, y, out_dtype, N,          K,         workspace, workspace_bytes, cfg};
    return gemm_mt_impl(a, offset, reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_bnb_mt_single(const void* x, int64_t M, const uint8_t* packed, int64_t packed_len, const float* absmax,
                           int64_t nabs, int32_t blocksize, void* y, int32_t out_dtype, int64_t N, int64_t K,
                           void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{true,      x, M, packed,    packed_len, nullptr, nabs, nullptr,   absmax,          nabs,
                            blocksize, 1, y, out_dtype, N,          K,       workspace, workspace_bytes, cfg};
    return gemm_mt_impl(a, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
