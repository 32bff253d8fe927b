// nf4_gemm_moe_pf.hip -- the fused NF4 expert GEMM for prompts in bitsandbytes semantics
// (nf4_gemm_bnb_moe_pf: 1..16384 (token, choice) pairs, routed on the device): kernels, launcher
// and C entries.  The plan -- validation, cfg, geometry, LDS, workspace layout -- is
// nf4_gemm_moe_pf_plan.h.
//
// y[p][N] = x[p / x_div][K] . W_e[N][K]^T with e = expert_ids[p] read ON THE DEVICE and W_e the
// 16-bit weights nf4_dequant_bnb writes for expert e, bit for bit.  One C call is three kernels on
// the stream, all of a geometry the host fixes from (P, E, cfg) alone:
//
//  1. moe_pf_route_kernel, ONE workgroup of 16 waves, turns ids[P] into the workspace's tables:
//     perm[P], the pair indices grouped by bucket (bucket = the id, or E for an id outside
//     0..E-1) and ascending within a bucket; count[E + 1]; and the slot table, which cuts every
//     bucket into runs of at most BM = 32 WV entries of perm: {bucket, first position, live rows}.
//     Wave w owns the ids [w c, w c + c) (c = the 64-multiple at or above P / 16) and walks them
//     in rounds of 64, one id per lane.  In a round the lanes with the same bucket find each other
//     by nine ballots (one per bit of the bucket: match-any), so a lane knows its rank among them
//     (popcount below) and their number without an atomic.  Pass 1 counts per (wave, bucket) in
//     LDS (16 x 257 words; the group's first lane adds, no two lanes of a round touch one word);
//     a prefix over (bucket, wave) -- per bucket over the waves by one thread each, over the
//     buckets by a shuffle scan of wave 0 -- turns the counts into each (wave, bucket)'s first
//     position; pass 2 walks the rounds again and stores pair p at position + rank.  Positions are
//     a function of the ids alone: no atomic takes part.
//  2. nf4_gemm_moe_pf_kernel, grid slots x column tiles x K slices.  A workgroup reads its slot
//     entry; no live row: it returns before any other load.  A slot of bucket E stores zero rows of
//     its 128 columns for its pairs (slice 0 alone) and returns.  Every other slot copies its
//     entries of perm into an LDS list (entries past `live` repeat the last live pair: in-bounds
//     loads that are never stored) and runs the prefill GEMM's pipeline (nf4_gemm_pf.hip, whose
//     header comment gives the layout of the staged rows, the slot rotation and the two-steps-ahead
//     loads) on expert `bucket`'s weights and statistics: the row of x a thread loads is
//     list[row] / x_div (a magic-number division, once per row ahead of the K loop), the row of y
//     a lane stores is list[row].  The split-K slab is indexed by POSITION IN perm, so a slot's
//     rows are contiguous in it and the reducer is the prefill one with its last store scattered;
//     one ticket per (slot, column tile) through mt_publish_last.
//     A row's fp32 sum runs over the same steps in the same order with the same MFMA as in
//     nf4_gemm_bnb_pf under the cfg of the same waves and ksplit, so its bits are that entry's.
//  3. moe_pf_clear_kernel zeroes the tables, so the whole workspace reads 0 again when the call
//     ends (a kernel, not a memset node: the three operations are then of one kind under capture).
// (pf_rot, the reducer and the MFMA step repeat nf4_gemm_pf.hip's: that file's code is not touched.)
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_moe_pf_plan.h"

namespace {

constexpr uint32_t kRouteWaves = kMoePfRouteThreads / 64u;
constexpr uint32_t kRouteBuckets = NF4DQ_MOE_MAX_EXPERTS + 1;  // the experts and the bucket of invalid ids
constexpr uint32_t kRoutePerLane = (kRouteBuckets + 63u) / 64u;  // buckets a lane of wave 0 scans

struct MoePfRouteArgs {
    const int32_t* ids;  // [P]
    uint32_t* slots;     // [S] x {bucket, first, live, 0}
    uint32_t* perm;      // [P]
    uint32_t* count;     // [E + 1]
    uint32_t P, E, bm, S;
};

// The lanes of this round with lane's bucket (bits 0..8), among the lanes `ok`.
__device__ __forceinline__ uint64_t moe_pf_match(uint32_t b, bool ok) {
    uint64_t m = __ballot(ok);
#pragma unroll
    for (uint32_t i = 0; i < 9u; ++i) {
        const bool bit = (b >> i) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__global__ __launch_bounds__(kMoePfRouteThreads) void moe_pf_route_kernel(const MoePfRouteArgs A) {
    __shared__ uint32_t cnt[kRouteWaves * kRouteBuckets];  // pass 1: counts; then first positions within the bucket
    __shared__ uint32_t tot[kRouteBuckets], base[kRouteBuckets], sbase[kRouteBuckets];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nb = A.E + 1u;
    const uint64_t below = (uint64_t(1) << lane) - 1u;
    const uint32_t chunk = ((A.P + kRouteWaves - 1u) / kRouteWaves + 63u) & ~63u;
    const uint32_t p_begin = wave * chunk < A.P ? wave * chunk : A.P;
    const uint32_t p_end = p_begin + chunk < A.P ? p_begin + chunk : A.P;
    uint32_t* mine = cnt + wave * kRouteBuckets;

    for (uint32_t i = tid; i < kRouteWaves * kRouteBuckets; i += kMoePfRouteThreads) cnt[i] = 0u;
    __syncthreads();
    auto bucket_of = [&](uint32_t p, bool ok) {
        const int32_t id = A.ids[ok ? p : A.P - 1u];  // (past P: the last id again, in bounds)
        return (uint32_t)id < A.E ? (uint32_t)id : A.E;
    };
    for (uint32_t p0 = p_begin; p0 < p_end; p0 += 64u) {  // (wave-uniform bounds)
        const uint32_t p = p0 + lane;
        const bool ok = p < A.P;
        const uint32_t b = bucket_of(p, ok);
        const uint64_t m = moe_pf_match(b, ok);
        if (ok && (m & below) == 0u) mine[b] += (uint32_t)__popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next round's first lanes may be others
    }
    __syncthreads();
    if (tid < nb) {  // over the waves, per bucket
        uint32_t run = 0;
        for (uint32_t w = 0; w < kRouteWaves; ++w) {
            const uint32_t c = cnt[w * kRouteBuckets + tid];
            cnt[w * kRouteBuckets + tid] = run;
            run += c;
        }
        tot[tid] = run;
    }
    __syncthreads();
    if (wave == 0u) {  // over the buckets: pairs and slots ahead of each
        uint32_t pairs = 0, blocks = 0;
        for (uint32_t j = 0; j < kRoutePerLane; ++j) {
            const uint32_t b = lane * kRoutePerLane + j, c = b < nb ? tot[b] : 0u;
            pairs += c;
            blocks += (c + A.bm - 1u) / A.bm;
        }
        uint32_t ip = pairs, ib = blocks;  // inclusive scan over the lanes
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(ip, d), ub = __shfl_up(ib, d);
            if (lane >= d) ip += up, ib += ub;
        }
        uint32_t ep = ip - pairs, eb = ib - blocks;
        for (uint32_t j = 0; j < kRoutePerLane; ++j) {
            const uint32_t b = lane * kRoutePerLane + j;
            if (b < nb) {
                base[b] = ep, sbase[b] = eb;
                ep += tot[b];
                eb += (tot[b] + A.bm - 1u) / A.bm;
            }
        }
    }
    __syncthreads();
    if (tid < nb) {
        const uint32_t c = tot[tid];
        A.count[tid] = c;
        for (uint32_t j = 0, s = sbase[tid]; j * A.bm < c && s < A.S; ++j, ++s) {  // (s < S: the bound holds for every routing)
            const uint32_t left = c - j * A.bm;
            *reinterpret_cast<u32x4*>(A.slots + 4u * s) = u32x4{tid, base[tid] + j * A.bm, left < A.bm ? left : A.bm, 0u};
        }
    }
    for (uint32_t p0 = p_begin; p0 < p_end; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const bool ok = p < A.P;
        const uint32_t b = bucket_of(p, ok);
        const uint64_t m = moe_pf_match(b, ok);
        const uint32_t rank = (uint32_t)__popcll(m & below);
        const uint32_t at = ok ? base[b] + mine[b] + rank : 0u;
        if (ok && at < A.P) A.perm[at] = p;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // every lane has read its bucket's position
        if (ok && rank == 0u) mine[b] += (uint32_t)__popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

__global__ __launch_bounds__(256) void moe_pf_clear_kernel(u32x4* at, uint32_t n16) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n16) at[i] = u32x4{0u, 0u, 0u, 0u};
}

struct MoePfArgs {
    const uint8_t* packed;  // [E] x [N][K/2], packed_stride bytes apart
    const uint8_t* a1;      // nested: absmax bytes [N K / 64] per expert, nb_stride apart
    const float* a2;        // nested: absmax2; single: the fp32 absmax; n2_stride floats apart
    const float* code2;     // nested: [256], code2_stride floats apart (0: shared)
    const float* offset;    // nested: [E] or null (= 0)
    int64_t packed_stride, nb_stride, n2_stride, code2_stride;
    const void* x;          // [ceil(P / x_div)][K]
    void* y;                // [P][N]
    float* slab;            // [ksplit][P positions][N] (ksplit > 1)
    uint32_t* counters;     // one ticket per (slot, column tile)
    const uint32_t* slots;  // the routing kernel's tables
    const uint32_t* perm;
    FastDiv xdiv;
    uint32_t P, E, N, K;
    uint32_t ksplit, sps, steps, tiles;  // K slices, steps per slice, K / 64, N / 128
    uint32_t sh2;           // log2(blocksize2)
};

// Slot rotation of a staged row (the prefill kernel's).
__device__ __forceinline__ uint32_t mpf_rot(uint32_t row) { return (row >> 1) & 3u; }

// The reducer of one (slot, column tile): the prefill kernel's over the slot's `live` consecutive
// positions from `first`, each element summed in slice order and cleared behind the sum; the
// finished row goes to y[list[row]].
template <int DT, int WV>
__device__ inline void mpf_reduce(const MoePfArgs& A, const uint32_t* list, uint32_t first, uint32_t live, uint32_t col0) {
    constexpr uint32_t T = 64u * WV, kE = 4;
    const uint32_t total = live * (kPfCols / 4u), plane = A.P * A.N;  // < 2^30 floats: validated
    for (uint32_t b0 = 0; b0 < total; b0 += kE * T) {  // (a workgroup-uniform trip count)
        const uint32_t base = b0 + threadIdx.x;
        uint32_t at[kE], to[kE];
        f32x4 sum[kE];
#pragma unroll
        for (uint32_t j = 0; j < kE; ++j) {
            const uint32_t e0 = base + j * T, e = e0 < total ? e0 : total - 1u;
            const uint32_t row = e / (kPfCols / 4u), col = col0 + 4u * (e % (kPfCols / 4u));
            at[j] = (first + row) * A.N + col;
            to[j] = list[row] * A.N + col;
        }
        for (uint32_t sl = 0; sl < A.ksplit; ++sl) {
            f32x4 v[kE];
#pragma unroll
            for (uint32_t j = 0; j < kE; ++j) v[j] = *reinterpret_cast<const f32x4*>(A.slab + sl * plane + at[j]);
#pragma unroll
            for (uint32_t j = 0; j < kE; ++j) {
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
        for (uint32_t j = 0; j < kE; ++j)
            if (base + j * T < total) {
                for (uint32_t sl = 0; sl < A.ksplit; ++sl)
                    *reinterpret_cast<f32x4*>(A.slab + sl * plane + at[j]) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + to[j]) =
                    u32x2{pack2<DT>(sum[j].x, sum[j].y), pack2<DT>(sum[j].z, sum[j].w)};
            }
    }
}

// (two waves per SIMD, as the prefill kernel: two 128-row workgroups or one 256-row workgroup on a CU)
template <int DT, int SM, int WV>
__global__ __launch_bounds__(64 * WV, 2) void nf4_gemm_moe_pf_kernel(const MoePfArgs A) {
    constexpr uint32_t T = 64u * WV, BM = 32u * WV;
    constexpr uint32_t kXBuf = BM * kPfRowBytes, kWBuf = kPfCols * kPfRowBytes;
    constexpr int NP = 4;                    // 16-byte pieces of x per thread and step: BM * 8 / T
    constexpr uint32_t WP = T / kPfCols;     // threads per weight row: 2 / 4
    constexpr int WD = 8 / (int)WP;          // packed dwords per thread and step: 4 / 2
    static_assert(BM * 8u == NP * T && WP * WD == 8, "a step divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x 0][x 1][w 0][w 1][code2][codes][flag][list]
    char* xs = smem;
    char* ws = smem + 2u * kXBuf;
    float* c2tab = reinterpret_cast<float*>(ws + 2u * kWBuf);
    float* lut = c2tab + 256;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);
    uint32_t* list = reinterpret_cast<uint32_t*>(ws + 2u * kWBuf + kPfTableBytes);  // staged row -> pair

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t wr = wave >> 1, wc = wave & 1u;  // the wave's 64 x 64 of the tile
    const uint32_t ks = blockIdx.x % A.ksplit, rest = blockIdx.x / A.ksplit;
    const uint32_t tile = rest % A.tiles, slot = rest / A.tiles;
    const uint32_t col0 = tile * kPfCols;

    const u32x4 se = *reinterpret_cast<const u32x4*>(A.slots + 4u * slot);
    const uint32_t ex = se.x, first = se.y, live = se.z;
    if (live == 0u) return;  // a slot the routing does not use
    if (ex >= A.E) {         // ids outside 0..E-1: rows of zero bits, once per column tile
        if (ks == 0u)
            for (uint32_t e = tid; e < live * (kPfCols / 4u); e += T) {
                const uint32_t pair = A.perm[first + e / (kPfCols / 4u)];
                *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + (pair * A.N + col0 + 4u * (e % (kPfCols / 4u)))) =
                    u32x2{0u, 0u};
            }
        return;
    }
    if (tid < BM) list[tid] = A.perm[first + (tid < live ? tid : live - 1u)];  // past live: the last live pair again

    // expert ex's bases
    const uint8_t* packed = A.packed + (int64_t)ex * A.packed_stride;
    const uint8_t* a1 = SM == kScaleBnb ? A.a1 + (int64_t)ex * A.nb_stride : nullptr;
    const float* a2 = A.a2 + (int64_t)ex * A.n2_stride;
    if constexpr (SM == kScaleBnb) {
        const float* code2 = A.code2 + (int64_t)ex * A.code2_stride;
        for (uint32_t i = tid; i < 256u; i += T) c2tab[i] = code2[i];
    }
    write_lut(lut);
    const float off = load_offset<SM>(A.offset ? A.offset + ex : nullptr);
    __syncthreads();  // the list and the tables

    const uint32_t s_begin = ks * A.sps < A.steps ? ks * A.sps : A.steps;
    const uint32_t s_end = s_begin + A.sps < A.steps ? s_begin + A.sps : A.steps;
    const uint32_t n = s_end - s_begin;  // steps of this slice
    auto step_at = [&](uint32_t i) { return s_begin + (i < n ? i : n - 1u); };

    // what a thread moves per step: NP pieces of x (of NP gathered rows, fixed over the K loop), WD
    // packed dwords of weight row wn with their block's statistics
    const uint32_t wn = tid / WP, wh = tid % WP;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;
    uint32_t xat[NP];  // element offset of the piece within its row of x, step 0
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const uint32_t p = tid + (uint32_t)i * T, row = p >> 3, seg = p & 7u;
        xat[i] = fdiv(list[row], A.xdiv) * A.K + seg * 8u;  // < 2^30: validated
    }
    u32x4 xr[2][NP];
    uint32_t wq[2][WD], qa[2];
    float qb[2];
    auto load = [&](auto S, uint32_t st) {
        const char* xg = reinterpret_cast<const char*>(A.x);
#pragma unroll
        for (int i = 0; i < NP; ++i) xr[S][i] = *reinterpret_cast<const u32x4*>(xg + (xat[i] + st * kPfStepK) * 2u);
        const uint8_t* wp = packed + ((col0 + wn) * kb + st * 32u + wh * (4u * WD));  // < 2^31: validated
        if constexpr (WD == 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(wp);
            wq[S][0] = v.x, wq[S][1] = v.y, wq[S][2] = v.z, wq[S][3] = v.w;
        } else {
            const u32x2 v = *reinterpret_cast<const u32x2*>(wp);
            wq[S][0] = v.x, wq[S][1] = v.y;
        }
        const uint32_t f = (col0 + wn) * bpr + st;  // 64-block on the expert's flat stream
        if constexpr (SM == kScaleBnb) {
            qa[S] = a1[f];
            qb[S] = a2[f >> A.sh2];
        } else {
            qa[S] = 0u;
            qb[S] = a2[f];
        }
    };
    const char* t = reinterpret_cast<const char*>(lut);
    auto store = [&](auto S, uint32_t b) {
        char* xb = xs + b * kXBuf;
        char* wb = ws + b * kWBuf;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t p = tid + (uint32_t)i * T, row = p >> 3, seg = p & 7u;
            *reinterpret_cast<u32x4*>(xb + row * kPfRowBytes + ((seg + mpf_rot(row)) & 7u) * 16u) = xr[S][i];
        }
        const float sc = block_scale<SM>(c2tab, qa[S], qb[S], off);
#pragma unroll
        for (int d = 0; d < WD; ++d)
            *reinterpret_cast<u32x4*>(wb + wn * kPfRowBytes + ((wh * WD + (uint32_t)d + mpf_rot(wn)) & 7u) * 16u) =
                mt_decode<DT>(t, wq[S][d], sc);
    };

    f32x4 acc[4][4];  // [x row tile][column tile]
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    if (n > 0u) {
        load(I0{}, step_at(0));
        load(I1{}, step_at(1));
        store(I0{}, 0u);
        load(I0{}, step_at(2));
    }
    __syncthreads();  // the first stage

    const uint32_t q0 = 4u * (kh & 1u) + 2u * (kh >> 1) + mpf_rot(nl);  // row 16 t + nl: the rotation depends on nl alone
    const uint32_t wfrag = (wc * 64u + nl) * kPfRowBytes, xfrag = (wr * 64u + nl) * kPfRowBytes;
    // step i of the slice (J = i & 1): its x and weights are in buffer J, step i + 1 in register
    // set J ^ 1 (landed or in flight), step i + 2 in set J (in flight)
    auto step = [&](auto J, uint32_t i) {
        constexpr int j = decltype(J)::value;
        const char* xb = xs + (uint32_t)j * kXBuf + xfrag;
        const char* wb = ws + (uint32_t)j * kWBuf + wfrag;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t sl = ((q0 + (uint32_t)s) & 7u) * 16u;
            u32x4 a[4], b[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) a[ct] = *reinterpret_cast<const u32x4*>(wb + 16u * ct * kPfRowBytes + sl);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) b[mt] = *reinterpret_cast<const u32x4*>(xb + 16u * mt * kPfRowBytes + sl);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = mt_mfma<DT>(a[ct], b[mt], acc[mt][ct]);
            __builtin_amdgcn_sched_barrier(0);  // one set of fragments live at a time (the prefill kernel's reason)
        }
        store(std::integral_constant<int, j ^ 1>{}, (uint32_t)(j ^ 1));
        load(std::integral_constant<int, j ^ 1>{}, step_at(i + 3u));
        __syncthreads();
    };
    for (uint32_t i = 0; i < n; i += 2u) {
        step(I0{}, i);
        if (i + 1u >= n) break;
        step(I1{}, i + 1u);
    }

    // acc[mt][ct][i] is the slot's row 64 wr + 16 mt + nl, column col0 + 64 wc + 16 ct + 4 kh + i
    const uint32_t ycol = col0 + wc * 64u + 4u * kh;
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const uint32_t m = wr * 64u + 16u * mt + nl;
            if (m < live) {
                const uint32_t at = list[m] * A.N + ycol;  // < 2^30: validated
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + at + 16u * ct) =
                        u32x2{pack2<DT>(acc[mt][ct].x, acc[mt][ct].y), pack2<DT>(acc[mt][ct].z, acc[mt][ct].w)};
            }
        }
        return;
    }
    float* mine = A.slab + ks * (A.P * A.N);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const uint32_t m = wr * 64u + 16u * mt + nl;
        if (m < live)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<f32x4*>(mine + (first + m) * A.N + ycol + 16u * ct) = acc[mt][ct];
    }
    if (mt_publish_last(A.counters + slot * A.tiles + tile, A.ksplit, flag)) mpf_reduce<DT, WV>(A, list, first, live, col0);
}

template <int SM>
int launch_moe_pf(const nf4gemm::MoeCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& e = *a.ex;
    const MoePfPlan p = moe_pf_plan(cfg, a.P, e.experts, e.N, e.K);
    const MoePfLayout l = moe_pf_layout(a.P, e.experts, e.N, cfg);
    char* ws = reinterpret_cast<char*>(a.workspace);
    MoePfRouteArgs R{};
    R.ids = reinterpret_cast<const int32_t*>(a.ids);
    R.slots = reinterpret_cast<uint32_t*>(ws + l.slots);
    R.perm = reinterpret_cast<uint32_t*>(ws + l.perm);
    R.count = reinterpret_cast<uint32_t*>(ws + l.count);
    R.P = (uint32_t)a.P;
    R.E = (uint32_t)e.experts;
    R.bm = p.bm;
    R.S = p.slots;
    MoePfArgs A{};
    A.packed = e.packed;
    A.a1 = e.absmax_q;
    A.a2 = e.absmax2;
    A.code2 = e.code2;
    A.offset = e.offset;
    A.packed_stride = e.packed_stride;
    A.nb_stride = e.nb_stride;
    A.n2_stride = e.n2_stride;
    A.code2_stride = e.code2_stride;
    A.x = a.x;
    A.y = a.y;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.slots = R.slots;
    A.perm = R.perm;
    A.xdiv = make_fastdiv((uint32_t)a.x_div);
    A.P = R.P;
    A.E = R.E;
    A.N = (uint32_t)e.N;
    A.K = (uint32_t)e.K;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.sps = p.sps;
    A.steps = p.steps;
    A.tiles = p.tiles;
    A.sh2 = mt_log2_blocksize2(e.single != 0, e.blocksize2);

    hipLaunchKernelGGL(moe_pf_route_kernel, dim3(1), dim3(kMoePfRouteThreads), 0, st, R);
    int rc = hip_rc2(hipGetLastError());
    if (rc) return rc;
    rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<8, 4>(cfg.waves, [&](auto WV) {
            launch_lds<&nf4_gemm_moe_pf_kernel<DT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
            rc = hip_rc2(hipGetLastError());
        });
    });
    // the tables are cleared whatever the GEMM's launch answered: the route kernel has been enqueued
    const uint32_t n16 = (uint32_t)((l.need - l.slots) / 16u);
    hipLaunchKernelGGL(moe_pf_clear_kernel, dim3((n16 + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<u32x4*>(ws + l.slots), n16);
    const int rc2 = hip_rc2(hipGetLastError());
    return rc ? rc : rc2;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_pf_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg) {
    if (!experts) return 0;
    const nf4_moe_experts& e = *reinterpret_cast<const nf4_moe_experts*>(experts);
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS || !moe_pf_shape(P, e.N, e.K)) return 0;
    nf4_gemm_cfg c = cfg ? *cfg : moe_pf_default_cfg(P, e.experts, e.N, e.K, device_cus());
    if (cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_MOE_PF;
    return valid_moe_pf_cfg(c, P, e.N, e.K) ? moe_pf_workspace_need(P, e.experts, e.N, e.K, c) : 0;
}

int nf4_gemm_bnb_moe_pf(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts, void* y,
                        int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                        void* hip_stream) {
    const nf4gemm::MoeCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(experts), y, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_pf_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex->single ? launch_moe_pf<kScaleBnbSingle>(a, c, st) : launch_moe_pf<kScaleBnb>(a, c, st);
}

}  // extern "C"
