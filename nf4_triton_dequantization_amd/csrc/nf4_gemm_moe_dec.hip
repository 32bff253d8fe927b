// nf4_gemm_moe_dec.hip -- the fused NF4 expert GEMM for decode in 16-row slots, in bitsandbytes
// semantics (nf4_gemm_bnb_moe_dec: 1..128 (token, choice) pairs, routed on the device, one launch):
// kernel, launcher and C entries.  The plan -- validation, cfg, geometry, LDS, workspace -- is
// nf4_gemm_moe_dec_plan.h.
//
// y[p][N] = x[p / x_div][K] . W_e[N][K]^T with e = expert_ids[p] read ON THE DEVICE and W_e the
// 16-bit weights nf4_dequant_bnb writes for expert e, bit for bit.  nf4_gemm_bnb_moe gives an
// expert one workgroup per column tile whose row tiles are sized from P and whose two or four
// waves decode every weight through the 16-entry code table; with 1..16 rows per expert that
// decode is the whole cost.  This kernel joins device-side routing to the body of the
// register-resident small-M family (nf4_gemm_dev.h) instead:
//  * the grid is slots x column tiles (64 columns) x K slices, fixed by the host; a slot is one
//    (expert, block of 16 consecutive entries of its ascending pair list), numbered in (expert,
//    block) order, so a workgroup's row tile is ONE MFMA M-tile whatever P is;
//  * the routing.  Wave 0 reads the P ids, two per lane (in-bounds repeats past P), and finds for
//    every pair the lanes that hold the same id by sixteen ballots (one per id bit and half:
//    match-any), hence the pair's rank in its expert's ascending list and the expert's count by
//    popcounts.  The first pair of every expert stores the count to LDS (one writer a word), a
//    shuffle scan over the 256 counts turns ceil(count / 16) into each expert's first slot, and a
//    pair's slot is first[id] + rank / 16: the pairs whose slot is the workgroup's store
//    themselves at rank % 16 of the slot's list.  Everything is a function of the ids alone: no
//    atomic takes part.  Meanwhile all waves build the pair table.  A slot nobody claims returns
//    before any weight or statistics load and draws no ticket;
//  * rows of ids outside [0, E) are stored as zero bits by the workgroups of slot 0, K slice 0
//    (one per column tile): slot 0 is in every grid, and they do it before they look at their own
//    rows, so those rows are stored whatever the routing;
//  * K is split over the WAVES: wave w of K slice ks owns the KPW 128-deep chunks from
//    (ks WV + w) KPW.  It gathers the slot's rows of x for them straight from global memory into
//    MFMA A fragments (row nl of the list, k = 128 c + 32 kh + 8 s: 16 bytes a fragment; rows past
//    the slot's count and chunks past K take an offset beyond the buffer and read as zeros) and
//    keeps them in registers for the whole launch;
//  * each wave walks the tile's four 16-column strips with a D-deep register ring: per strip and
//    chunk one 16-byte packed load of the lane's row (k as above) and its 64-block's statistics;
//  * the decode is the small-M families' pair table: byte b of a packed dword addresses one
//    8-byte entry {code[b >> 4], code[b & 15]} (32 copies, one per lane mod 32: no bank conflict),
//    one packed fp32 multiply by the block scale (nested: fl32(fl32(code2[q] * absmax2) + offset),
//    never fused) and one RNE pack give two exact 16-bit weights; four dwords are four
//    v_mfma_f32_16x16x32 into the strip's one accumulator;
//  * the waves' partial tiles meet in LDS (in the pair table's place, once every wave is done with
//    it) and waves 0..3 sum one strip each in wave order over the waves that own a chunk;
//  * one K slice: rounded once, stored to y[pair].  More: the slice's tile goes to the family's
//    fp32 slab indexed by pair; one ticket per (slot, column tile) through mt_publish_last; the
//    last arrival sums in slice order, rounds once, scatters to y[pair] and clears what it read.
// A row's bits depend on its x row, its expert and the cfg alone: an MFMA row takes nothing from
// the rows beside it, and which wave and slice own which chunk is fixed by the cfg.
// Nobody waits for anybody: there is no poll.
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_moe_dec_plan.h"

namespace {

struct MoeDecArgs {
    const uint8_t* packed;  // [E] x [N][K/2], packed_stride bytes apart
    const uint8_t* a1;      // nested: absmax bytes [N K / 64] per expert, nb_stride apart
    const float* a2;        // nested: absmax2; single: the fp32 absmax; n2_stride floats apart
    const float* code2;     // nested: [256], code2_stride floats apart (0: shared)
    const float* offset;    // nested: [E] or null (= 0)
    int64_t packed_stride, nb_stride, n2_stride, code2_stride;
    const int32_t* ids;     // [P]
    const void* x;          // [ceil(P / x_div)][K]
    void* y;                // [P][N]
    float* slab;            // [ksplit][P][N] (ksplit > 1)
    uint32_t* counters;     // one ticket per (slot, column tile)
    uint32_t P, E, N, K, x_div;
    uint32_t tiles, ksplit, chunks;  // column tiles, K slices, K / 128
    uint32_t sh2;           // log2(blocksize2)
};

// One strip of the ring: per chunk of the wave the lane's 16 packed bytes and its block's statistics.
template <int KPW>
struct DecSlot {
    u32x4 w[KPW];
    uint8_t qa[KPW];  // kept 8-bit: a widening right behind the load would wait for it
    float qb[KPW];
};

// One 128-deep chunk of one strip: 32 weights of the lane's row through the pair table, four MFMAs.
template <int DT>
__device__ __forceinline__ void dec_chunk_mma(const u32x4& w, float sc, const char* pt, uint32_t slot8, const u32x4 (&xf)[4],
                                              f32x4& acc) {
    const f32x2 sc2 = {sc, opaque(sc)};
    constexpr int LA = 2;  // steps the lookups run ahead of their products
    f32x2 v[4][4];
    auto issue = [&](int st) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            // (byte b of the dword) * 256 + the lane's copy * 8
            const uint32_t addr = __builtin_amdgcn_perm(w[st], slot8, 0x0C0C0000u | ((4u + b) << 8));
            v[st][b] = *reinterpret_cast<const f32x2*>(pt + addr);
        }
    };
#pragma unroll
    for (int st = 0; st < LA; ++st) issue(st);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        if (st + LA < 4) issue(st + LA);
        uint32_t bw[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const f32x2 p = v[st][b] * sc2;  // fp32 products, never fused
            bw[b] = pack2<DT>(p.x, p.y);     // RNE
        }
        acc = mt_mfma<DT>(xf[st], u32x4{bw[0], bw[1], bw[2], bw[3]}, acc);
    }
}

// (at least 4 waves per SIMD: at most 128 registers a lane, the plan's moe_dec_resident())
template <int DT, int SM, int WV, int KPW, int D>
__global__ __launch_bounds__(64 * WV, 4) void nf4_gemm_moe_dec_kernel(const MoeDecArgs A) {
    constexpr uint32_t T = 64u * WV;
    constexpr int NS = kMoeDecTileStrips;
    static_assert(KPW <= 2 && NS % D == 0, "x fragments and ring within 128 registers; whole ring rounds per tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // the plan's layout
    char* pt = smem;                                 // the pair table; then the waves' partial tiles
    f32x4* red = reinterpret_cast<f32x4*>(smem);     // [WV][NS][64]
    float* c2tab = reinterpret_cast<float*>(smem + kMoeDecPairTableBytes);
    uint32_t* ecnt = reinterpret_cast<uint32_t*>(c2tab + 256);  // pairs per expert
    uint32_t* efirst = ecnt + 256;                              // first slot per expert
    uint32_t* info = efirst + 256;                              // {reducer flag, expert, rows, -}
    uint32_t* prow = info + 4;                                  // the slot's pairs, ascending

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t ks = blockIdx.x % A.ksplit, st = blockIdx.x / A.ksplit;
    const uint32_t tile = st % A.tiles, slot = st / A.tiles;  // (st is also the ticket's index)

    // wave 0: the ids, two per lane, ahead of everything else
    const uint32_t p0 = lane, p1 = lane + 64u;
    int32_t id0 = 0, id1 = 0;
    if (wave == 0u) id0 = A.ids[p0 < A.P ? p0 : A.P - 1u], id1 = A.ids[p1 < A.P ? p1 : A.P - 1u];
    if (tid < 256u) ecnt[tid] = 0u;
    if (tid < 4u) info[tid] = 0u;
    __syncthreads();

    if (wave == 0u) {
        const bool in0 = p0 < A.P, in1 = p1 < A.P;
        const bool v0 = in0 && (uint32_t)id0 < A.E, v1 = in1 && (uint32_t)id1 < A.E;
        if (slot == 0u && ks == 0u) {  // rows of ids outside [0, E): zero bits in this tile's columns
            const uint64_t z0 = __ballot(in0 && !v0), z1 = __ballot(in1 && !v1);
            for (int h = 0; h < 2; ++h)
                for (uint64_t b = h ? z1 : z0; b; b &= b - 1u) {
                    const uint32_t p = (uint32_t)__builtin_ctzll(b) + 64u * (uint32_t)h;
                    if (lane < kMoeDecCols / 4u)
                        *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + (p * A.N + tile * kMoeDecCols + 4u * lane)) =
                            u32x2{0u, 0u};
                }
        }
        // match-any over both halves: a0 / a1 = the lanes whose id0 / id1 equals this lane's id0,
        // b0 / b1 the same for this lane's id1 (valid ids are below 256: eight bits)
        const uint64_t vb0 = __ballot(v0), vb1 = __ballot(v1);
        uint64_t a0 = vb0, a1 = vb1, b0 = vb0, b1 = vb1;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const bool t0 = ((uint32_t)id0 >> i) & 1u, t1 = ((uint32_t)id1 >> i) & 1u;
            const uint64_t bal0 = __ballot(t0), bal1 = __ballot(t1);
            a0 &= t0 ? bal0 : ~bal0;
            a1 &= t0 ? bal1 : ~bal1;
            b0 &= t1 ? bal0 : ~bal0;
            b1 &= t1 ? bal1 : ~bal1;
        }
        const uint64_t below = (uint64_t(1) << lane) - 1u;
        const uint32_t rank0 = (uint32_t)__popcll(a0 & below), n0 = (uint32_t)(__popcll(a0) + __popcll(a1));
        const uint32_t rank1 = (uint32_t)(__popcll(b0) + __popcll(b1 & below)), n1 = (uint32_t)(__popcll(b0) + __popcll(b1));
        if (v0 && rank0 == 0u) ecnt[id0] = n0;  // an expert's first pair alone
        if (v1 && rank1 == 0u) ecnt[id1] = n1;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // first slot per expert: four experts a lane, an inclusive scan over the lanes
        uint32_t nb[4], mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            nb[j] = (ecnt[4u * lane + j] + 15u) >> 4;
            mine += nb[j];
        }
        uint32_t inc = mine;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        uint32_t run = inc - mine;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            efirst[4u * lane + j] = run;
            run += nb[j];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // the pairs of this workgroup's slot list themselves; the slot's first pair names the expert
        if (v0 && efirst[id0] + (rank0 >> 4) == slot) {
            prow[rank0 & 15u] = p0;
            if ((rank0 & 15u) == 0u) info[1] = (uint32_t)id0, info[2] = n0 - rank0 < 16u ? n0 - rank0 : 16u;
        }
        if (v1 && efirst[id1] + (rank1 >> 4) == slot) {
            prow[rank1 & 15u] = p1;
            if ((rank1 & 15u) == 0u) info[1] = (uint32_t)id1, info[2] = n1 - rank1 < 16u ? n1 - rank1 : 16u;
        }
    }
    // the pair table, by all waves: entry (16 hi + lo) * 32 + copy = {code[hi], code[lo]}
    for (uint32_t u = tid; u < 1024u; u += T) {
        const uint32_t lo = (u & 511u) >> 5, copy = u & 31u, half = u >> 9;  // (half is wave-uniform)
        const float clo = nf4_code(lo);
        f32x2* ptab = reinterpret_cast<f32x2*>(pt);
#pragma unroll
        for (uint32_t hi = 0; hi < 16u; ++hi)
            if ((hi >> 3) == half) ptab[(16u * hi + lo) * 32u + copy] = f32x2{nf4_code(hi), clo};
    }
    __syncthreads();  // the slot, the list, the pair table

    const uint32_t ex = info[1], cnt = info[2];
    if (cnt == 0u) return;  // a slot past the used ones: no weight, no statistics, no ticket

    // the wave's chunks, its rows of x as A fragments, the first D strips of the ring
    const uint32_t cw = (ks * (uint32_t)WV + wave) * (uint32_t)KPW;  // the wave's first chunk
    const uint32_t live = A.chunks - ks * (uint32_t)(WV * KPW);      // chunks from this slice's first on (>= 1)
    const uint32_t nlive = live >= (uint32_t)(WV * KPW) ? (uint32_t)WV : (live + (uint32_t)KPW - 1u) / (uint32_t)KPW;  // waves that own one
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1, nblk = A.N * bpr;
    const uint32_t xrows = (A.P + A.x_div - 1u) / A.x_div;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)A.x, 0, xrows * A.K * 2u, kRsrcFlags);  // < 2^31: validated
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc((void*)(A.packed + (int64_t)ex * A.packed_stride), 0, A.N * kb, kRsrcFlags);
    const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(SM == kScaleBnb ? A.a1 + (int64_t)ex * A.nb_stride : A.packed), 0, SM == kScaleBnb ? nblk : 0u, kRsrcFlags);
    const uint32_t n2 = SM == kScaleBnb ? (nblk + (1u << A.sh2) - 1u) >> A.sh2 : nblk;
    const __amdgpu_buffer_rsrc_t ra2 = __builtin_amdgcn_make_buffer_rsrc((void*)(A.a2 + (int64_t)ex * A.n2_stride), 0, n2 * 4u, kRsrcFlags);

    u32x4 xf[KPW][4];
    {
        const uint32_t xr = prow[nl < cnt ? nl : 0u] / A.x_div;
#pragma unroll
        for (int q = 0; q < KPW; ++q) {
            const uint32_t c = cw + (uint32_t)q;
            const uint32_t xoff = nl < cnt && c < A.chunks ? (xr * A.K + c * kChunkK + 32u * kh) * 2u : kOob;
#pragma unroll
            for (int s = 0; s < 4; ++s) xf[q][s] = __builtin_amdgcn_raw_buffer_load_b128(rx, xoff + 16u * (uint32_t)s, 0, 0);
        }
    }
    const uint32_t row0 = tile * kMoeDecCols + nl;  // the lane's weight row in strip 0
    DecSlot<KPW> ring[D];
    auto issue = [&](DecSlot<KPW>& s, uint32_t strip) {
        const uint32_t r = row0 + 16u * strip;
#pragma unroll
        for (int q = 0; q < KPW; ++q) {
            const uint32_t c = cw + (uint32_t)q;
            const uint32_t oob = c < A.chunks ? 0u : kOob;  // past K: zeros, no traffic, still one counted load each
            s.w[q] = __builtin_amdgcn_raw_buffer_load_b128(rw, (r * kb + c * 64u + 16u * kh) | oob, 0, 0);  // < 2^31: validated
            const uint32_t f = r * bpr + 2u * c + (kh >> 1);  // the lane's 64-block on the expert's flat stream
            if constexpr (SM == kScaleBnb) {
                s.qa[q] = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(ra1, f | oob, 0, 0);
                s.qb[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ra2, ((f >> A.sh2) * 4u) | oob, 0, 0));
            } else {
                s.qa[q] = 0;
                s.qb[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ra2, (f * 4u) | oob, 0, 0));
            }
        }
    };
    __builtin_amdgcn_sched_barrier(0);  // issue order = wait order: x, then the ring strip by strip
#pragma unroll
    for (int d = 0; d < D; ++d) {
        issue(ring[d], (uint32_t)d);
        __builtin_amdgcn_sched_barrier(0);
    }
    float off = 0.0f;
    if constexpr (SM == kScaleBnb) {
        const float* code2 = A.code2 + (int64_t)ex * A.code2_stride;
        if (tid < 256u) c2tab[tid] = code2[tid];
        off = load_offset<SM>(A.offset ? A.offset + ex : nullptr);
        __syncthreads();  // the expert's code2 table
    }

    const uint32_t slot8 = (lane & 31u) * 8u;
    f32x4 acc[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        DecSlot<KPW>& s = ring[t % D];
#pragma unroll
        for (int q = 0; q < KPW; ++q)
            dec_chunk_mma<DT>(s.w[q], block_scale<SM>(c2tab, s.qa[q], s.qb[q], off), pt, slot8, xf[q], acc[t]);
        if (t + D < NS) {
            __builtin_amdgcn_sched_barrier(0);
            issue(s, (uint32_t)(t + D));
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // the waves' partial tiles, in the pair table's place; waves 0..3 sum one strip each in wave order
    __syncthreads();  // every wave is done with the pair table
    if (wave < nlive) {
#pragma unroll
        for (int t = 0; t < NS; ++t) red[(wave * NS + (uint32_t)t) * 64u + lane] = acc[t];
    }
    __syncthreads();
    // sum[i]: the slot's row 4 kh + i, column tile * 64 + 16 wave + nl
    const uint32_t col = tile * kMoeDecCols + 16u * wave + nl;
    f32x4 sum = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (wave < (uint32_t)NS) {
        sum = red[wave * 64u + lane];
        for (uint32_t w = 1; w < nlive; ++w) sum += red[(w * NS + wave) * 64u + lane];
    }
    if (A.ksplit == 1u) {
        if (wave < (uint32_t)NS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 4u * kh + (uint32_t)i;
                const float right = __shfl_xor(sum[i], 1, 64);  // column col + 1
                if (m < cnt && !(nl & 1u))
                    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(A.y) + (prow[m] * A.N + col)) = pack2<DT>(sum[i], right);
            }
        }
        return;
    }
    const uint32_t plane = A.P * A.N;  // floats per slice; ksplit planes < 2^30 floats: validated
    if (wave < (uint32_t)NS) {
        float* mine = A.slab + (size_t)ks * plane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 4u * kh + (uint32_t)i;
            if (m < cnt) mine[prow[m] * A.N + col] = sum[i];
        }
    }
    if (!mt_publish_last(A.counters + st, A.ksplit, info)) return;
    // the last arrival: (row, four columns) per thread, summed in slice order, cleared behind the sum
    if (tid < cnt * (kMoeDecCols / 4u)) {
        const uint32_t at = prow[tid >> 4] * A.N + tile * kMoeDecCols + 4u * (tid & 15u);
        f32x4 s4 = *reinterpret_cast<const f32x4*>(A.slab + at);  // the first slice starts the sum: -0 stays -0
        for (uint32_t sl = 1; sl < A.ksplit; ++sl) s4 += *reinterpret_cast<const f32x4*>(A.slab + (size_t)sl * plane + at);
        for (uint32_t sl = 0; sl < A.ksplit; ++sl) *reinterpret_cast<f32x4*>(A.slab + (size_t)sl * plane + at) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + at) = u32x2{pack2<DT>(s4.x, s4.y), pack2<DT>(s4.z, s4.w)};
    }
}

template <int SM>
int launch_moe_dec(const nf4gemm::MoeCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& e = *a.ex;
    const MoeDecPlan p = moe_dec_plan(cfg, a.P, e.experts, e.N, e.K);
    MoeDecArgs A{};
    A.packed = e.packed;
    A.a1 = e.absmax_q;
    A.a2 = e.absmax2;
    A.code2 = e.code2;
    A.offset = e.offset;
    A.packed_stride = e.packed_stride;
    A.nb_stride = e.nb_stride;
    A.n2_stride = e.n2_stride;
    A.code2_stride = e.code2_stride;
    A.ids = reinterpret_cast<const int32_t*>(a.ids);
    A.x = a.x;
    A.y = a.y;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.P = (uint32_t)a.P;
    A.E = (uint32_t)e.experts;
    A.N = (uint32_t)e.N;
    A.K = (uint32_t)e.K;
    A.x_div = (uint32_t)a.x_div;
    A.tiles = p.tiles;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.chunks = p.chunks;
    A.sh2 = mt_log2_blocksize2(e.single != 0, e.blocksize2);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<16, 8>(cfg.waves, [&](auto WV) {
            pick<1, 2>(cfg.strips, [&](auto KPW) {
                pick<2, 4>(cfg.depth, [&](auto D) {
                    launch_lds<&nf4_gemm_moe_dec_kernel<DT, SM, WV, KPW, D>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                    rc = hip_rc2(hipGetLastError());
                });
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_dec_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg) {
    if (!experts) return 0;
    const nf4_moe_experts& e = *reinterpret_cast<const nf4_moe_experts*>(experts);
    if (e.experts < 1 || e.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return moe_dec_workspace_need(P, e.N, e.K, cfg ? *cfg : moe_dec_default_cfg(P, e.experts, e.N, e.K, device_cus()));
}

int nf4_gemm_bnb_moe_dec(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts, void* y,
                         int32_t out_dtype, void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg,
                         void* hip_stream) {
    const nf4gemm::MoeCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(experts), y, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = moe_dec_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex->single ? launch_moe_dec<kScaleBnbSingle>(a, c, st) : launch_moe_dec<kScaleBnb>(a, c, st);
}

}  // extern "C"
