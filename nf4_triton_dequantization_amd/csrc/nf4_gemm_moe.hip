// nf4_gemm_moe.hip -- the fused NF4 expert GEMM of a mixture-of-experts block in bitsandbytes
// semantics (nf4_gemm_bnb_moe): kernel, launcher and C entries.  The plan -- validation, cfg,
// geometry, LDS, workspace -- is nf4_gemm_moe_plan.h.
//
// y[p][N] = x[p / x_div][K] . W_e[N][K]^T with e = expert_ids[p] read ON THE DEVICE and W_e the
// 16-bit weights nf4_dequant_bnb writes for expert e, bit for bit.  One launch covers every
// expert; the anatomy is the row-tiled family's (nf4_gemm_mt_dev.h, whose header comment gives the
// reasons for the clamped loads, the slot rotation and the register budget -- they hold here).
// The ring entry, the rotation, the decode, the MFMA call, the split-K hand-off and the reducer
// are that header's; the chunk loop is this file's own, because of its run-time row-tile guards:
//  * the grid is experts x column tiles x K slices, fixed by the host from (P, E, N, K, CUs);
//    a workgroup (WV waves) owns ONE expert, 32 WV of its columns and one K slice;
//  * every wave reads the P ids (two per lane, clamped in bounds) and ballots `id == expert`:
//    the two masks are wave-uniform, so the count and, by popcount prefix, the expert's
//    ascending pair list follow without an atomic -- the list, and with it the summation, is a
//    function of the inputs and the cfg alone.  Wave 0 writes the list to LDS twice: the x row
//    (pair / x_div) and the y row (the pair) of every staged row;
//  * a workgroup whose expert has no pair returns before any weight or statistics load and
//    draws no ticket (all K slices of that expert see the same ids, so the ticket stays 0): an
//    idle expert's weights cost no HBM traffic;
//  * rows are gathered from x through the list into the staged tiles (rows past the expert's
//    count repeat its last row's load, in bounds, and are zeros in LDS) and scattered back to
//    y[pair].  The kernel is instantiated for the row tiles P can need (2 / 4 / 6 / 8: one
//    expert may get every pair); row tiles beyond the expert's own count skip their LDS stores,
//    fragment reads and MFMAs under wave-uniform branches -- never their global loads, so the
//    compiler's wait counts stay exact;
//  * rows of y whose id is outside [0, E) are zeroed by the workgroups of expert 0, K slice 0
//    (one per column tile): they exist whatever the routing and do it before they look at their
//    own count, so those rows are stored even when expert 0 is idle.  Every other row belongs
//    to exactly one expert: stored once per column tile, directly or by the reducer.
// Split-K: the row-tiled kernel's hand-off with the slab indexed by pair and one ticket per
// (expert, column tile).  Nobody waits for anybody: there is no poll.
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_moe_plan.h"

namespace {

struct MoeArgs {
    const uint8_t* packed;  // [E] x [N][K/2], packed_stride bytes apart
    const uint8_t* a1;      // nested: absmax bytes [N K / 64] per expert, nb_stride apart
    const float* a2;        // nested: absmax2; single: the fp32 absmax; n2_stride floats apart
    const float* code2;     // nested: [256], code2_stride floats apart (0: shared)
    const float* offset;    // nested: [E] or null (= 0)
    const int32_t* ids;     // [P]
    const void* x;          // [ceil(P / x_div)][K]
    void* y;                // [P][N]
    float* slab;            // [ksplit][P][N] (ksplit > 1)
    uint32_t* counters;     // one ticket per (expert, column tile)
    int64_t packed_stride, nb_stride, n2_stride, code2_stride;
    uint32_t P, E, N, K, x_div;
    uint32_t tiles, ksplit, cps, chunks;  // column tiles, K slices, chunks per slice, K / 128
    uint32_t sh2;           // log2(blocksize2)
};

// (the second launch bound, waves per SIMD: with two row tiles the kernel needs no more than 256
// registers, so a CU holds two workgroups of 4 waves -- what the plan's K-slice rule counts on,
// moe_resident(); more than two would spill)
template <int DT, int MT, int SM, int WV>
__global__ __launch_bounds__(64 * WV, MT <= 2 ? 2 : 1) void nf4_gemm_moe_kernel(const MoeArgs A) {
    constexpr uint32_t T = 64u * WV;
    constexpr uint32_t kBuf = 16u * MT * kMtRowBytes;
    constexpr int NP = 16 * MT * 16 / (int)T;  // 16-byte pieces of a stage per thread
    constexpr uint32_t COLS = 32u * WV;
    static_assert(16 * MT * 16 % T == 0, "a stage divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2][codes][flag][x rows][y rows]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * kBuf);
    float* lut = c2tab + 256;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);
    uint32_t* srow = flag + 4;                       // staged row -> row of x
    uint32_t* prow = srow + NF4DQ_MOE_MAX_PAIRS;     // staged row -> pair (row of y)

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t ks = blockIdx.x % A.ksplit, et = blockIdx.x / A.ksplit;
    const uint32_t tile = et % A.tiles, ex = et / A.tiles;

    // the routing: every wave reads all P ids (in-bounds repeats past P) and ballots
    const uint32_t p0 = lane, p1 = lane + 64u;
    const int32_t id0 = A.ids[p0 < A.P ? p0 : A.P - 1u], id1 = A.ids[p1 < A.P ? p1 : A.P - 1u];
    const bool in0 = p0 < A.P, in1 = p1 < A.P;
    const uint64_t m0 = __ballot(in0 && id0 == (int32_t)ex), m1 = __ballot(in1 && id1 == (int32_t)ex);
    const uint32_t cnt0 = (uint32_t)__popcll(m0), cnt = cnt0 + (uint32_t)__popcll(m1);

    if (ex == 0u && ks == 0u) {  // rows of ids outside [0, E): zeros in this tile's columns
        const uint64_t z0 = __ballot(in0 && (uint32_t)id0 >= A.E), z1 = __ballot(in1 && (uint32_t)id1 >= A.E);
        for (int h = 0; h < 2; ++h)
            for (uint64_t b = h ? z1 : z0; b; b &= b - 1u) {
                const uint32_t p = (uint32_t)__builtin_ctzll(b) + 64u * (uint32_t)h;
                if (tid < COLS / 4u)
                    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + (p * A.N + tile * COLS + 4u * tid)) = u32x2{0u, 0u};
            }
    }
    if (cnt == 0u) return;  // an idle expert: no weight, no statistics, no ticket

    if (wave == 0u) {  // the expert's ascending pair list, by popcount prefix
        const uint64_t below = (uint64_t(1) << lane) - 1u;
        if ((m0 >> lane) & 1u) {
            const uint32_t r = (uint32_t)__popcll(m0 & below);
            prow[r] = p0;
            srow[r] = p0 / A.x_div;
        }
        if ((m1 >> lane) & 1u) {
            const uint32_t r = cnt0 + (uint32_t)__popcll(m1 & below);
            prow[r] = p1;
            srow[r] = p1 / A.x_div;
        }
    }
    const uint32_t my_tiles = (cnt + 15u) >> 4;  // row tiles this expert fills

    const uint32_t col0 = tile * COLS + wave * 32u;
    const uint32_t c_begin = ks * A.cps < A.chunks ? ks * A.cps : A.chunks;
    const uint32_t c_end = c_begin + A.cps < A.chunks ? c_begin + A.cps : A.chunks;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;
    const uint8_t* packed = A.packed + (int64_t)ex * A.packed_stride;
    const uint8_t* a1 = SM == kScaleBnb ? A.a1 + (int64_t)ex * A.nb_stride : nullptr;
    const float* a2 = A.a2 + (int64_t)ex * A.n2_stride;

    if constexpr (SM == kScaleBnb) {
        const float* code2 = A.code2 + (int64_t)ex * A.code2_stride;
        for (uint32_t i = tid; i < 256u; i += T) c2tab[i] = code2[i];
    }
    write_lut(lut);
    const float off = load_offset<SM>(A.offset ? A.offset + ex : nullptr);
    __syncthreads();  // the pair list, ahead of the first gather

    // Loads run ahead of the MFMAs in registers, slots compile-time, chunk numbers past the
    // slice's end clamped to its last chunk: as in nf4_gemm_mt_dev.h.
    constexpr int kWD = 4;
    constexpr int kXS = kMtXSets<MT, WV>;
    constexpr int NPR = kXS == 2 ? NP : NP / 2;  // one set: the stage in two halves, half the registers
    u32x4 xr[kXS][NPR];
    MtW w[kWD];
    const uint32_t n = c_end - c_begin;  // chunks of this slice
    auto chunk_at = [&](uint32_t i) { return c_begin + (i < n ? i : n - 1u); };
    // (staged rows >= cnt load the expert's last row again and are zeroed on their way into LDS:
    // an in-bounds repeat, no branch around a load)
    auto xload = [&](auto S, uint32_t c, int half = 0) {
        const char* xg = reinterpret_cast<const char*>(A.x);
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const uint32_t p = tid + (uint32_t)(i + half * NPR) * T, row = p >> 4, seg = p & 15u;
            const uint32_t r = srow[row < cnt ? row : cnt - 1u];
            xr[S][i] = *reinterpret_cast<const u32x4*>(xg + (r * A.K + c * kChunkK + seg * 8u) * 2u);  // < 2^31: validated
        }
    };
    auto xstore = [&](auto S, char* buf, int half = 0) {
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const uint32_t piece = (uint32_t)(i + half * NPR);
            const uint32_t p = tid + piece * T, row = p >> 4, seg = p & 15u;
            if (piece * T / 256u < my_tiles) {  // the piece's row tile (wave-uniform): tiles the expert does not fill are never read
                const u32x4 v = row < cnt ? xr[S][i] : u32x4{0u, 0u, 0u, 0u};  // rows >= cnt: zeros in LDS
                *reinterpret_cast<u32x4*>(buf + row * kMtRowBytes + ((seg + mt_rot(row)) & 15u) * 16u) = v;
            }
        }
    };
    auto wload = [&](auto S, uint32_t c) {
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) {
            const uint32_t r = col0 + 16u * nt + nl;
            w[S].w[nt] = *reinterpret_cast<const u32x4*>(packed + (r * kb + c * 64u + 16u * kh));  // < 2^31: validated
            const uint32_t f = r * bpr + 2u * c + (kh >> 1);  // 64-block on the expert's flat stream
            if constexpr (SM == kScaleBnb) {
                w[S].qa[nt] = a1[f];
                w[S].qb[nt] = a2[f >> A.sh2];
            } else {
                w[S].qa[nt] = 0u;
                w[S].qb[nt] = a2[f];
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
    auto step = [&](auto J, uint32_t i) {
        constexpr int j = decltype(J)::value;
        const char* buf = smem + (uint32_t)(j & 1) * kBuf;
        wload(std::integral_constant<int, (j + 3) % kWD>{}, chunk_at(i + 3u));
        if constexpr (kXS == 1) xload(I0{}, chunk_at(i + 1u));
        const MtW& cur = w[j];
        float sc[kMtStrips];
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) sc[nt] = block_scale<SM>(c2tab, cur.qa[nt], cur.qb[nt], off);
        auto aread = [&](u32x4(&a)[MT], int s) {
            const uint32_t slot = ((4u * kh + (uint32_t)s + rot) & 15u) * 16u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                if ((uint32_t)mt < my_tiles)
                    a[mt] = *reinterpret_cast<const u32x4*>(buf + (16u * mt + nl) * kMtRowBytes + slot);
        };
        auto decode = [&](u32x4(&bw)[kMtStrips], int s) {
#pragma unroll
            for (int nt = 0; nt < kMtStrips; ++nt) bw[nt] = mt_decode<DT>(t, cur.w[nt][s], sc[nt]);
        };
        constexpr int kAF = MT >= 8 ? 1 : 2;
        u32x4 af[kAF][MT], bw[2][kMtStrips];  // (af[.][mt] is read and used under the same mt < my_tiles)
        if constexpr (kAF == 2) aread(af[0], 0);
        decode(bw[0], 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (kAF == 1) aread(af[0], s);
            if (s < 3) {
                if constexpr (kAF == 2) aread(af[(s + 1) & 1], s + 1);
                decode(bw[(s + 1) & 1], s + 1);
            }
            if constexpr (kXS == 1)
                if (s == 2) {  // first half of x[i + 1] lands in the other buffer, the second half sets out
                    xstore(I0{}, smem + (uint32_t)((j + 1) & 1) * kBuf, 0);
                    xload(I0{}, chunk_at(i + 1u), 1);
                }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if ((uint32_t)mt < my_tiles) {  // wave-uniform: a row tile the expert does not fill
#pragma unroll
                    for (int nt = 0; nt < kMtStrips; ++nt)
                        acc[mt][nt] = mt_mfma<DT>(af[s & (kAF - 1)][mt], bw[s & 1][nt], acc[mt][nt]);
                }
            }
        }
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

    // acc[mt][nt][i] = y[pair of staged row 16 mt + 4 kh + i][col0 + 16 nt + nl]
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
                if (m < cnt) {
                    const uint32_t at = prow[m] * A.N + col0 + nl;
#pragma unroll
                    for (int nt = 0; nt < kMtStrips; ++nt) store_y<DT>(A.y, at + 16u * nt, acc[mt][nt][i]);
                }
            }
        return;
    }
    float* mine = A.slab + (size_t)ks * A.P * A.N;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
            if (m < cnt) {
                const uint32_t at = prow[m] * A.N + col0 + nl;
#pragma unroll
                for (int nt = 0; nt < kMtStrips; ++nt) mine[at + 16u * nt] = acc[mt][nt][i];
            }
        }
    // publish, ticket, acquire and the slice-order reducer: the family's (nf4_gemm_mt_dev.h), with
    // the rows taken from the pair list and the ticket of this (expert, column tile)
    const MtJob job{A.x, A.y, A.slab, A.counters + et, smem, lut, flag, A.P, A.N, A.K, tile, ks, A.ksplit, A.cps, A.chunks};
    if (mt_publish_last(job.ticket, A.ksplit, flag))
        mt_reduce<DT, MT, WV, MtStrips<1>, MtSumOut<DT>>(job, MtListedRows{cnt, prow});
}

template <int SM>
int launch_moe(const nf4gemm::MoeCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& e = *a.ex;
    const MoePlan p = moe_plan(cfg, a.P, e.experts, e.N, e.K);
    MoeArgs A{};
    A.packed = e.packed;
    A.a1 = e.absmax_q;
    A.a2 = e.absmax2;
    A.code2 = e.code2;
    A.offset = e.offset;
    A.ids = reinterpret_cast<const int32_t*>(a.ids);
    A.x = a.x;
    A.y = a.y;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.packed_stride = e.packed_stride;
    A.nb_stride = e.nb_stride;
    A.n2_stride = e.n2_stride;
    A.code2_stride = e.code2_stride;
    A.P = (uint32_t)a.P;
    A.E = (uint32_t)e.experts;
    A.N = (uint32_t)e.N;
    A.K = (uint32_t)e.K;
    A.x_div = (uint32_t)a.x_div;
    A.tiles = p.tiles;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.cps = p.cps;
    A.chunks = p.chunks;
    A.sh2 = mt_log2_blocksize2(e.single, e.blocksize2);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_moe_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg) {
    if (!experts) return 0;
    const nf4_moe_experts& e = *reinterpret_cast<const nf4_moe_experts*>(experts);
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return moe_workspace_need(P, e.N, e.K, cfg ? *cfg : moe_default_cfg(P, e.experts, e.N, e.K, device_cus()));
}

int nf4_gemm_bnb_moe(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts, void* y,
                     int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                     void* hip_stream) {
    const nf4gemm::MoeCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(experts), y, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex->single ? launch_moe<kScaleBnbSingle>(a, c, st) : launch_moe<kScaleBnb>(a, c, st);
}

}  // extern "C"
