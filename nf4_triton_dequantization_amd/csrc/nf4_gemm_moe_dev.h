// nf4_gemm_moe_dev.h -- the device code of the fused NF4 expert kernels of a mixture-of-experts
// block in bitsandbytes semantics, once.  Four launchers instantiate this one kernel template:
//  * nf4_gemm_moe.hip (nf4_gemm_bnb_moe: the products of the (token, choice) pairs): DOWN false,
//    W = 1;
//  * nf4_gemm_moe_down.hip (nf4_gemm_bnb_moe_down: the same products, combined per token with the
//    routing weights inside the launch): DOWN true, W = 1;
//  * nf4_gemm_moe_swiglu.hip (nf4_gemm_bnb_moe_swiglu: h = silu(g) * u over a gate and an up stack):
//    DOWN false, W = 2;
//  * nf4_gemm_moe_rb.hip (nf4_gemm_bnb_moe_rb: nf4_gemm_bnb_moe's products for up to 1024 pairs,
//    in row blocks of 128 listed rows): DOWN false, W = 1, RB true.
// DOWN, W and RB are compile-time: every branch of the other instantiations is discarded.  What the
// merge of the three kernels into this template moved in the generated code, and what it cost, is
// in profiles/gemm_moe_family/README.md; that RB left every earlier instantiation's instruction
// stream as it was, and what that took, is in profiles/gemm_moe_rb/README.md.
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
//
// RB: the grid gains ceil(P / 128) row blocks (the outermost index).  A workgroup ballots all P ids
// in rounds of 64, one per lane, with a running count, and owns entries [128 rb, 128 rb + 128) of
// its expert's ascending pair list: wave 0 writes only those to the LDS list, which stays 128
// entries.  A workgroup whose expert has no more than 128 rb pairs returns before any weight or
// statistics load and draws no ticket; tickets are one per (expert, column tile, row block); rows
// of invalid ids are zeroed by the workgroups of expert 0, K slice 0, row block 0 over all P.
// Everything behind the list -- gather, stage, decode, MFMA, scatter, hand-off, reducer -- is the
// code above on the block's rows, so a row's bits do not depend on the entry that computed it.
//
// W: what a wave's two strips are (MtStrips<W>) and what becomes of their sums.  All of the above
// holds for both.
//  * W = 1: two 16-column strips of ONE stack, 32 WV columns of y a workgroup, MtSumOut, one fp32
//    plane per slice;
//  * W = 2: h[p][I] = silu(g) * u with g = x[p / x_div] . Wg_e^T and u = x[p / x_div] . Wu_e^T.
//    Strip 0 is rows col .. col + 15 of the expert's gate weight and strip 1 the same rows of its
//    up weight, each from its own stack: base pointers (base + e * stride), statistics,
//    blocksize2, offset (offset[e]) and code2 table (two tables in LDS, c2tab + 256 wt, each from
//    code2 + e * code2_stride of its own stack).  A workgroup owns 16 WV columns of h;
//    acc[mt][0][i] and acc[mt][1][i] are g and u of ONE element of h in one lane.  g and u are
//    what W = 1 stores for the gate and the up stack (exact 16-bit weights, fp32 MFMA sums, one
//    RNE), the chain SgOut's (swiglu16 of nf4_gemm_mt_dev.h); a slice stores two planes,
//    [ksplit][2][P][I], and the slice that draws the last ticket sums each in slice order over the
//    expert's listed rows and applies the chain.
//
// DOWN: out[t][N] = rn(sum_j rn(y[t k + j] * rn(rw[t k + j]))) with y[p] the 16-bit row above.
//  * A.y is a 16-bit scratch [P][N] in the workspace: the workgroup (one K slice) or the
//    slice-order reducer (several) stores the expert's finished rows there through the paths
//    above.  Rows of invalid ids are never stored and never used: the combiner reads the ids;
//  * a second ticket per COLUMN TILE counts E arrivals, one per expert: the workgroup that stored
//    the expert's rows, or -- an idle expert -- its K-slice-0 workgroup, which still returns
//    before any weight or statistics load.  An arrival is mt_publish_last: stores drained,
//    barrier, one agent-scope release, a relaxed fetch-add; the last one acquires and puts the
//    ticket back to 0;
//  * the workgroup that draws a tile's last ticket combines the tile (moe_combine): per token
//    and four columns the products in fp32, rounded once each, summed in fp32 from +0 in the
//    order j = 0 .. k-1, rounded once.  The order depends on j alone, so out is a function of
//    the inputs and the cfg alone.  Nobody waits for anybody here either.
#pragma once

#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_moe_plan.h"

namespace {

// A launch over W stacks of experts (1: one weight; 2: gate, up).  Per-stack fields are arrays of W.
template <int W>
struct MoeArgsT {
    const uint8_t* packed[W];  // [E] x [N][K/2], packed_stride bytes apart
    const uint8_t* a1[W];      // nested: absmax bytes [N K / 64] per expert, nb_stride apart
    const float* a2[W];        // nested: absmax2; single: the fp32 absmax; n2_stride floats apart
    const float* code2[W];     // nested: [256], code2_stride floats apart (0: shared)
    const float* offset[W];    // nested: [E] or null (= 0)
    const int32_t* ids;        // [P]
    const void* x;             // [ceil(P / x_div)][K]
    void* y;                   // [P][N]
    float* slab;               // [ksplit][W][P][N] (ksplit > 1)
    uint32_t* counters;        // one ticket per (expert, column tile)
    int64_t packed_stride[W], nb_stride[W], n2_stride[W], code2_stride[W];
    uint32_t P, E, N, K, x_div;
    uint32_t tiles, ksplit, cps, chunks;  // column tiles, K slices, chunks per slice, K / 128
    uint32_t sh2[W];           // log2(blocksize2)
};

// The fill every launcher shares: the stacks, the call (Call: MoeCall or MsgCall) and the plan.
// y: where the kernel stores its rows (the caller's output, or DOWN's scratch).
template <int W, class Call>
inline MoeArgsT<W> moe_fill(const Call& a, void* y, const nf4gemm::MoePlan& p, const nf4_gemm_cfg& cfg) {
    MoeArgsT<W> A{};
    for (int i = 0; i < W; ++i) {
        const nf4_moe_experts& e = a.ex[i];
        A.packed[i] = e.packed;
        A.a1[i] = e.absmax_q;
        A.a2[i] = e.absmax2;
        A.code2[i] = e.code2;
        A.offset[i] = e.offset;
        A.packed_stride[i] = e.packed_stride;
        A.nb_stride[i] = e.nb_stride;
        A.n2_stride[i] = e.n2_stride;
        A.code2_stride[i] = e.code2_stride;
        A.sh2[i] = mt_log2_blocksize2(e.single, e.blocksize2);
    }
    A.ids = reinterpret_cast<const int32_t*>(a.ids);
    A.x = a.x;
    A.y = y;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.P = (uint32_t)a.P;
    A.E = (uint32_t)a.ex[0].experts;
    A.N = (uint32_t)a.ex[0].N;
    A.K = (uint32_t)a.ex[0].K;
    A.x_div = (uint32_t)a.x_div;
    A.tiles = p.tiles;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.cps = p.cps;
    A.chunks = p.chunks;
    return A;
}

// A 16-bit value of the output dtype, widened to fp32 (exact).
template <int DT>
__device__ __forceinline__ float widen16(uint16_t b) {
    if constexpr (DT == NF4DQ_BF16) return __builtin_bit_cast(float, (uint32_t)b << 16);
    else return (float)__builtin_bit_cast(_Float16, b);
}

// What DOWN adds to a launch (A.y is then the scratch).
struct MoeCombine {
    const int32_t* ids;     // [P]
    const void* rw;         // [P] routing weights, fp32 (rw_f32) or the output dtype
    const uint16_t* d;      // the scratch [P][N]: the 16-bit products
    void* out;              // [P / topk][N]
    uint32_t* tile_ticket;  // one per column tile
    uint32_t P, E, N, topk, rw_f32;
};

// The combine of one column tile (COLS columns from col0), by the whole workgroup of T threads:
// element = (token, four columns).  Elements past the tile repeat its last one (in-bounds loads)
// and are not stored; the scratch row of an invalid id is loaded (in bounds, whatever it holds)
// and replaced by +0, so a NaN weight still gives NaN.
template <int DT, uint32_t T, uint32_t COLS>
__device__ inline void moe_combine(const MoeCombine& C, uint32_t col0) {
    const uint32_t total = C.P / C.topk * (COLS / 4u);
    for (uint32_t e0 = threadIdx.x; e0 < total + T - 1u - (total + T - 1u) % T; e0 += T) {
        const uint32_t e = e0 < total ? e0 : total - 1u;
        const uint32_t t = e / (COLS / 4u), col = col0 + 4u * (e % (COLS / 4u));
        float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // from +0, as torch's sum: -0 + -0 gives +0
        for (uint32_t j = 0; j < C.topk; ++j) {
            const uint32_t p = t * C.topk + j;
            const bool valid = (uint32_t)C.ids[p] < C.E;
            const u32x2 raw = *reinterpret_cast<const u32x2*>(C.d + (p * C.N + col));  // < 2^31: validated
            const u32x2 dv = valid ? raw : u32x2{0u, 0u};
            float w;
            if (C.rw_f32) w = rne16<DT>(reinterpret_cast<const float*>(C.rw)[p]);  // what .to(dtype) does
            else w = widen16<DT>(reinterpret_cast<const uint16_t*>(C.rw)[p]);
            const float dl[4] = {widen16<DT>((uint16_t)dv.x), widen16<DT>((uint16_t)(dv.x >> 16)),
                                 widen16<DT>((uint16_t)dv.y), widen16<DT>((uint16_t)(dv.y >> 16))};
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[i] += rne16<DT>(dl[i] * w);  // the fp32 product of two 16-bit values is exact
        }
        if (e0 < total)
            *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(C.out) + (t * C.N + col)) =
                u32x2{pack2<DT>(sum[0], sum[1]), pack2<DT>(sum[2], sum[3])};
    }
}

// A launch's arguments: the expert GEMM's, and with DOWN the combine's behind them.
struct MoeDownArgs {
    MoeArgsT<1> g;
    MoeCombine c;
};
template <bool DOWN, int W>
using MoeKernArgs = std::conditional_t<DOWN, MoeDownArgs, MoeArgsT<W>>;
template <int W>
__device__ __forceinline__ const MoeArgsT<W>& moe_gemm_args(const MoeArgsT<W>& a) { return a; }
__device__ __forceinline__ const MoeArgsT<1>& moe_gemm_args(const MoeDownArgs& a) { return a.g; }

// (the second launch bound, waves per SIMD: with two row tiles the kernel needs no more than 256
// registers, so a CU holds two workgroups of 4 waves -- what the plan's K-slice rule counts on,
// moe_resident(); more than two would spill)
// (one kernel template, not a shared body behind several kernels: inlined from a function of its
// own the expert GEMM did not keep its registers and spills.  Where W = 1 and W = 2 place a
// statement differently -- the offset loads, the row and block index in wload, the slab address --
// each has the order of the kernel it was merged from: with one order for both, the other's
// instruction streams move and the 128-pair SwiGLU launch measured up to 1 % slower,
// profiles/gemm_moe_family/README.md)
template <int DT, int MT, int SM, int WV, bool DOWN = false, int W = 1, bool RB = false>
__global__ __launch_bounds__(64 * WV, MT <= 2 ? 2 : 1) void nf4_gemm_moe_kernel(const MoeKernArgs<DOWN, W> KA) {
    static_assert(!DOWN || W == 1, "the routed sum is behind one stack's products");
    static_assert(!RB || (!DOWN && W == 1), "row blocks: the plain expert GEMM alone");
    using Strips = MtStrips<W>;
    using Out = std::conditional_t<W == 2, SgOut<DT>, MtSumOut<DT>>;
    const MoeArgsT<W>& A = moe_gemm_args(KA);
    constexpr uint32_t T = 64u * WV;
    constexpr uint32_t kBuf = 16u * MT * kMtRowBytes;
    constexpr int NP = 16 * MT * 16 / (int)T;  // 16-byte pieces of a stage per thread
    constexpr uint32_t COLS = Strips::kWaveCols * WV;
    static_assert(16 * MT * 16 % T == 0, "a stage divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2 x W][codes][flag][x rows][y rows]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * kBuf);
    float* lut = c2tab + 256 * W;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);
    uint32_t* srow = flag + 4;                       // staged row -> row of x
    uint32_t* prow = srow + NF4DQ_MOE_MAX_PAIRS;     // staged row -> pair (row of y)

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t ks = blockIdx.x % A.ksplit, et = blockIdx.x / A.ksplit;
    // (RB: et = (row block * E + expert) * tiles + tile, which is also the ticket's index)
    const uint32_t tile = et % A.tiles, ex = RB ? et / A.tiles % A.E : et / A.tiles;

    // the routing up to 128 pairs (!RB): every wave reads all P ids (in-bounds repeats past P), two
    // per lane, and ballots.  (Declared here and filled ahead of `arrive`, where the kernels this
    // template was merged from had them: with the statements in another order the DOWN
    // instantiations' instruction streams move, profiles/gemm_moe_rb/README.md)
    uint32_t p0, p1, cnt0;
    int32_t id0, id1;
    bool in0, in1;
    uint64_t m0, m1;
    uint32_t cnt;  // the rows this workgroup stages: the expert's pairs, or (RB) its pairs in this row block
    if constexpr (!RB) {
        p0 = lane, p1 = lane + 64u;
        id0 = A.ids[p0 < A.P ? p0 : A.P - 1u], id1 = A.ids[p1 < A.P ? p1 : A.P - 1u];
        in0 = p0 < A.P, in1 = p1 < A.P;
        m0 = __ballot(in0 && id0 == (int32_t)ex), m1 = __ballot(in1 && id1 == (int32_t)ex);
        cnt0 = (uint32_t)__popcll(m0), cnt = cnt0 + (uint32_t)__popcll(m1);
    }

    // DOWN: this expert's arrival at the tile's ticket; the last of the E arrivals combines the tile
    auto arrive = [&]() {
        if constexpr (DOWN)
            if (mt_publish_last(KA.c.tile_ticket + tile, A.E, flag)) moe_combine<DT, T, COLS>(KA.c, tile * COLS);
    };
    if constexpr (RB) {
        // Row blocks: up to NF4DQ_MOE_RB_MAX_PAIRS ids in rounds of 64 (in-bounds repeats past P),
        // one wave-uniform mask a round and a running count; the workgroup owns entries
        // [lo, lo + 128) of the expert's ascending pair list and writes only those to LDS.
        const uint32_t lo = NF4DQ_MOE_MAX_PAIRS * (et / A.tiles / A.E);
        if (lo == 0u && ex == 0u && ks == 0u) {  // rows of ids outside [0, E), over all P: zeros in this tile's columns
            for (uint32_t base = 0; base < A.P; base += 64u) {
                const uint32_t p = base + lane;
                const int32_t id = A.ids[p < A.P ? p : A.P - 1u];
                for (uint64_t b = __ballot(p < A.P && (uint32_t)id >= A.E); b; b &= b - 1u) {
                    const uint32_t pz = base + (uint32_t)__builtin_ctzll(b);
                    if (tid < COLS / 4u)
                        *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.y) + (pz * A.N + tile * COLS + 4u * tid)) = u32x2{0u, 0u};
                }
            }
        }
        const uint64_t below = (uint64_t(1) << lane) - 1u;
        uint32_t seen = 0;  // the expert's pairs below `base`
        for (uint32_t base = 0; base < A.P && seen < lo + NF4DQ_MOE_MAX_PAIRS; base += 64u) {
            const uint32_t p = base + lane;
            const int32_t id = A.ids[p < A.P ? p : A.P - 1u];
            const uint64_t m = __ballot(p < A.P && id == (int32_t)ex);
            const uint32_t r = seen + (uint32_t)__popcll(m & below) - lo;  // the pair's entry in this block, if it has one
            if (wave == 0u && ((m >> lane) & 1u) && r < (uint32_t)NF4DQ_MOE_MAX_PAIRS) {
                prow[r] = p;
                srow[r] = p / A.x_div;
            }
            seen += (uint32_t)__popcll(m);
        }
        // an idle expert, or a row block past its pairs: no weight, no statistics, no ticket
        if (seen <= lo) return;
        cnt = seen - lo < (uint32_t)NF4DQ_MOE_MAX_PAIRS ? seen - lo : (uint32_t)NF4DQ_MOE_MAX_PAIRS;
    } else {
        if constexpr (DOWN) {
            if (cnt == 0u) {  // an idle expert: no weight, no statistics; slice 0 arrives for it
                if (ks == 0u) arrive();
                return;
            }
        }
        if (!DOWN && ex == 0u && ks == 0u) {  // rows of ids outside [0, E): zeros in this tile's columns
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
    }
    const uint32_t my_tiles = (cnt + 15u) >> 4;  // row tiles this expert (RB: this row block) fills

    const uint32_t col0 = tile * COLS + wave * Strips::kWaveCols;
    const uint32_t c_begin = ks * A.cps < A.chunks ? ks * A.cps : A.chunks;
    const uint32_t c_end = c_begin + A.cps < A.chunks ? c_begin + A.cps : A.chunks;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;
    Strips st{};
    st.c2tab = c2tab;
#pragma unroll
    for (int wt = 0; wt < W; ++wt) {
        st.packed[wt] = A.packed[wt] + (int64_t)ex * A.packed_stride[wt];
        st.a1[wt] = SM == kScaleBnb ? A.a1[wt] + (int64_t)ex * A.nb_stride[wt] : nullptr;
        st.a2[wt] = A.a2[wt] + (int64_t)ex * A.n2_stride[wt];
        st.sh2[wt] = A.sh2[wt];
        if constexpr (SM == kScaleBnb) {
            const float* code2 = A.code2[wt] + (int64_t)ex * A.code2_stride[wt];
            for (uint32_t i = tid; i < 256u; i += T) c2tab[256u * wt + i] = code2[i];
        }
        if constexpr (W == 2) st.off[wt] = load_offset<SM>(A.offset[wt] ? A.offset[wt] + ex : nullptr);
    }
    write_lut(lut);
    if constexpr (W == 1) st.off[0] = load_offset<SM>(A.offset[0] ? A.offset[0] + ex : nullptr);
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
    // r: the strip's weight row, f: its 64-block on the expert's flat stream.  W = 2: one row and
    // one block for both strips, ahead of the loads; W = 1: a row per strip, the block behind the
    // packed load -- where the two kernels this template was merged from had them, which is what
    // their instruction streams were measured with.
    auto wload = [&](auto S, uint32_t c) {
        uint32_t r = col0 + nl, f = 0;
        if constexpr (W == 2) f = r * bpr + 2u * c + (kh >> 1);
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) {
            const int wt = Strips::wt(nt);
            if constexpr (W == 1) r = col0 + 16u * nt + nl;
            w[S].w[nt] = *reinterpret_cast<const u32x4*>(st.packed[wt] + (r * kb + c * 64u + 16u * kh));  // < 2^31: validated
            if constexpr (W == 1) f = r * bpr + 2u * c + (kh >> 1);
            if constexpr (SM == kScaleBnb) {
                w[S].qa[nt] = st.a1[wt][f];
                w[S].qb[nt] = st.a2[wt][f >> st.sh2[wt]];
            } else {
                w[S].qa[nt] = 0u;
                w[S].qb[nt] = st.a2[wt][f];
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
        for (int nt = 0; nt < kMtStrips; ++nt) sc[nt] = block_scale<SM>(c2tab + 256 * Strips::wt(nt), cur.qa[nt], cur.qb[nt], st.off[Strips::wt(nt)]);
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

    // acc[mt][nt][i]: strip nt's sum for the pair of staged row 16 mt + 4 kh + i -- W = 1:
    // y[pair][col0 + 16 nt + nl]; W = 2: g (nt 0) and u (nt 1) of h[pair][col0 + nl]
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
                if (m < cnt) Out::store(A.y, prow[m] * A.N + col0, nl, acc[mt][0][i], acc[mt][1][i]);
            }
        arrive();
        return;
    }
    const uint32_t plane = A.P * A.N;  // floats per plane; every slice's planes < 2^30 floats: validated
    float* mine = A.slab + (W == 2 ? (size_t)ks * Out::kPlanes * plane : (size_t)ks * A.P * A.N);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
            if (m < cnt) {
                const uint32_t at = prow[m] * A.N + col0 + nl;
#pragma unroll
                for (int nt = 0; nt < kMtStrips; ++nt) mine[at + Out::slab_at(nt, plane)] = acc[mt][nt][i];
            }
        }
    // publish, ticket, acquire and the slice-order reducer: the family's (nf4_gemm_mt_dev.h), with
    // the rows taken from the pair list and the ticket of this (expert, column tile)
    const MtJob job{A.x, A.y, A.slab, A.counters + et, smem, lut, flag, A.P, A.N, A.K, tile, ks, A.ksplit, A.cps, A.chunks};
    if (mt_publish_last(job.ticket, A.ksplit, flag)) {
        mt_reduce<DT, MT, WV, Strips, Out>(job, MtListedRows{cnt, prow});
        arrive();
    }
}

}  // namespace
