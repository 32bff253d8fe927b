// nf4_gemm_mt_dev.h -- the device pipeline of the row-tiled fused NF4 dequant + GEMM family in
// bitsandbytes semantics, once.  nf4_gemm_mt.hip (33..128 dense rows) and nf4_gemm_mt_swiglu.hip
// (gate/up with the SwiGLU chain behind them) are this pipeline under two sets of compile-time
// policies.  nf4_gemm_moe_dev.h (one expert's listed rows: the one kernel template of
// nf4_gemm_moe.hip, of nf4_gemm_moe_down.hip with the routed sum behind it, and of
// nf4_gemm_moe_swiglu.hip over MtStrips<2> with the SwiGLU chain) shares the ring entry, the
// rotation, the decode, the MFMA call, the strip and output policies, the split-K hand-off and
// the reducer, and keeps its own chunk loop: its row-tile guards are run-time, and built from the
// shared loop it did not keep the registers, spills and speed it had
// (profiles/gemm_mt_family/README.md).
//
// y[M][N] = x[M][K] . W[N][K]^T with W the 16-bit weights nf4_dequant_bnb writes, bit for
// bit.  The families of nf4_gemm_dev.h hold x whole (LDS or registers) and at most two row
// tiles; here M reaches 128, so
//  * a workgroup (WV waves) owns a column tile, ALL MT row tiles and one K slice;
//  * a wave owns two 16-row strips of weight.  Per 128-deep chunk a lane loads 16 packed bytes
//    of its row in each strip (one 64-block, one scale) straight into registers, decodes each
//    dword once into one MFMA B fragment (fp32 product, RNE to 16 bits: the oracle's weight)
//    and multiplies it with every row tile: the decode cost per weight does not grow with M;
//  * x goes through LDS one chunk at a time, two buffers, one barrier per chunk.  Global loads
//    run ahead in registers: the weights (HBM) three chunks, x (L2) two, landing in the other
//    buffer after the current chunk's MFMAs.  An x fragment read (ds_read_b128) feeds the two
//    strips' MFMAs, so the LDS read rate stays at half the MFMA issue rate's demand;
//  * a CU holds one wave per SIMD of these kernels (64 KiB of x buffers at 128 rows, up to 256
//    registers), so the wave hides its own LDS round trips: the x fragments of an MFMA step
//    are read as one batch and the weights of the next step decoded while this step's MFMAs
//    run;
//  * a staged row is one 256-byte bank row; its sixteen 16-byte slots are rotated by
//    (row & 3) | (row & 4) << 1 slots, which puts the 16 lanes of every ds_read_b128 lane
//    group (rows 0-3 / 12-15 of one 32-deep K quarter with rows 4-11 of the next) on 16
//    different slots;
//  * the k permutation of nf4_gemm_dev.h: a lane's packed dword is its B fragment of one
//    MFMA step, and the A fragment is x at the same 8 k, so nothing is shuffled.
// Split-K: every slice stores its fp32 partials to its slab, waits for the stores, and after
// the workgroup barrier one lane releases at agent scope and draws the tile's ticket.  The
// workgroup that draws the last ticket acquires, sums the slabs in slice order, stores y and
// puts the slab and the ticket back to 0.  Nobody waits for anybody: there is no poll.
//
// What every change here has to keep:
//  * no branch around a global load.  Staged rows past the row count repeat the last row's load
//    and are zeros in LDS, chunk numbers past the slice's end repeat its last chunk, reducer
//    elements past the tile repeat its last one: in-bounds repeats, so the compiler counts the
//    loads in flight exactly and its wait counts stay exact;
//  * ring slots are compile-time (the chunk loop is unrolled by kWD), so the ring is registers;
//  * every row tile is live here: the chunk loop has no liveness guard at all.  A kernel whose
//    row tiles can be idle (the expert GEMM) guards its LDS stores, fragment reads and MFMAs
//    under wave-uniform branches in its own loop -- never a global load;
//  * the sched_barrier(0) after a batch of x fragment reads is a per-kernel flag (SB) that
//    records each kernel's measured state, not a tuning knob of this header;
//  * the x buffers are the first 2 * 16 MT * 256 bytes of the kernel's dynamic LDS; what follows
//    them (tables, codes, flag, row lists) is the kernel's own and pinned by its plan header;
//  * the summation order: MFMA order over the chunks of a slice, slice order in the reducer,
//    the first slice assigns.  The result is a function of the inputs and the cfg alone.
//
// The pipeline's stages (mt_accumulate, mt_finish, mt_publish_last, mt_reduce, mt_pipeline) are
// plain `inline`, not __forceinline__: each has one call site per kernel and internal linkage,
// so the inliner takes it -- after simplifying it, as it does the lambdas.  Forced inlining runs
// before any simplification and moved the kernels' AGPR counts off the ones they were measured
// with.  The assembly must hold no call: tools/gemm_mt_family_asm.py asserts it.
//
// The policies:
//  * rows (MtDenseRows; MtListedRows for the hand-off and the reducer alone): how many rows are
//    staged, which row of x a staged row is loaded from and which row of y it is stored to;
//  * strips (MtStrips<1>, MtStrips<2>): what a wave's two strips are -- two column strips
//    of one weight, or the same 16 rows of two weights, each with its own statistics;
//  * output (MtSumOut; SgOut, the SwiGLU chain of nf4_gemm_mt_swiglu.hip and
//    nf4_gemm_moe_swiglu.hip): how many fp32 planes a slice stores and what becomes of the two
//    strips' sums.
#pragma once

#include "nf4_gemm_launch.h"
#include "nf4_gemm_mt_plan.h"

namespace {

// ---- host side: what the three launchers share ------------------------------------------

// log2(blocksize2) of a nested weight (a validated power of two); 0 for single.
inline uint32_t mt_log2_blocksize2(bool single, int32_t blocksize2) {
    uint32_t sh = 0;
    while (!single && (1 << sh) < blocksize2) ++sh;
    return sh;
}

// The workspace: the tickets at its head, the fp32 slabs (ksplit > 1) behind the header.
inline uint32_t* mt_counters(void* workspace) { return reinterpret_cast<uint32_t*>(workspace); }
inline float* mt_slab(void* workspace, const nf4_gemm_cfg& cfg) {
    return cfg.ksplit > 1 ? reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + kHeaderBytes) : nullptr;
}

// ---- device side ------------------------------------------------------------------------

// One chunk of a lane's two strips: the packed bytes and the raw statistics.
struct MtW {
    u32x4 w[kMtStrips];
    uint32_t qa[kMtStrips];
    float qb[kMtStrips];
};

// x register sets of a stage (NP 16-byte pieces per thread).  Two-wave workgroups with 6 or 8 row
// tiles stage 12 or 16 pieces per thread, and eight row tiles need their registers for the MFMA
// operands: one set, x one chunk ahead in two halves, or the sets would spill.  Else two sets.
template <int MT, int WV>
constexpr int kMtXSets = 16 * MT * 16 / (64 * WV) > 8 || MT >= 8 ? 1 : 2;

// Slot rotation of a staged row (see the header comment).
__device__ __forceinline__ uint32_t mt_rot(uint32_t row) { return (row & 3u) | ((row & 4u) << 1); }

// One packed dword -> one MFMA B fragment: the exact weights nf4_dequant_bnb writes, fp32
// product of code and block scale, RNE to 16 bits.  t: the 16 codes in LDS.
template <int DT>
__device__ __forceinline__ u32x4 mt_decode(const char* t, uint32_t wd, float sc) {
    const uint32_t hi4 = (wd >> 2) & 0x3C3C3C3Cu;
    const uint32_t lo4 = (wd << 2) & 0x3C3C3C3Cu;
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = *reinterpret_cast<const float*>(t + ((hi4 >> (8 * k)) & 0xFFu)) * sc;
        v[2 * k + 1] = *reinterpret_cast<const float*>(t + ((lo4 >> (8 * k)) & 0xFFu)) * sc;
    }
    return u32x4{pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]), pack2<DT>(v[4], v[5]), pack2<DT>(v[6], v[7])};
}

template <int DT>
__device__ __forceinline__ f32x4 mt_mfma(const u32x4& a, const u32x4& b, const f32x4& c) {
    if constexpr (DT == NF4DQ_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// Row policy, dense: staged row r is row r of x and of y.
struct MtDenseRows {
    uint32_t count;  // M
    __device__ __forceinline__ uint32_t x_row(uint32_t r) const { return r; }
    __device__ __forceinline__ uint32_t y_row(uint32_t r) const { return r; }
};

// Row policy of the reducer for listed rows: staged row r is row prow[r] of y (a list in LDS).
struct MtListedRows {
    uint32_t count;
    const uint32_t* prow;
    __device__ __forceinline__ uint32_t y_row(uint32_t r) const { return prow[r]; }
};

// Strip policy: what a wave's two strips are.  W = 1: two 16-column strips of ONE weight (32
// columns of y per wave; one code2 table, offset and blocksize2).  W = 2: the same 16 rows of
// TWO weights (16 columns per wave), each with its own statistics, table (c2tab + 256 nt),
// offset and blocksize2.  wt(nt) is strip nt's weight, row(col, nt) its weight row for column col.
template <int W>
struct MtStrips {
    static constexpr uint32_t kWaveCols = 32u / W;
    const uint8_t* packed[W];  // [N][K/2]
    const uint8_t* a1[W];      // nested: absmax bytes [N K / 64]
    const float* a2[W];        // nested: absmax2; single: the fp32 absmax
    const float* c2tab;        // nested: the code2 table(s) in LDS
    float off[W];
    uint32_t sh2[W];           // log2(blocksize2)
    static __device__ __forceinline__ constexpr int wt(int nt) { return W == 2 ? nt : 0; }
    static __device__ __forceinline__ uint32_t row(uint32_t col, int nt) { return W == 2 ? col : col + 16u * nt; }
};

// Output policy, sum: the strips are columns col and col + 16 of y; one fp32 plane per slice.
template <int DT>
struct MtSumOut {
    static constexpr uint32_t kPlanes = 1;
    // where strip nt's partial goes, relative to its row's element in plane 0
    static __device__ __forceinline__ uint32_t slab_at(int nt, uint32_t /*plane*/) { return 16u * nt; }
    static __device__ __forceinline__ void store(void* y, uint32_t at, uint32_t nl, float s0, float s1) {
        store_y<DT>(y, at + nl, s0);
        store_y<DT>(y, at + 16u + nl, s1);
    }
    static __device__ __forceinline__ u32x2 pack4(const f32x4 (&s)[1]) {
        return u32x2{pack2<DT>(s[0].x, s[0].y), pack2<DT>(s[0].z, s[0].w)};
    }
};

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

// Output policy, SwiGLU: the strips are g and u of ONE column of h; two fp32 planes per slice
// (g, u), the chain behind the two sums.
template <int DT>
struct SgOut {
    static constexpr uint32_t kPlanes = 2;
    static __device__ __forceinline__ uint32_t slab_at(int nt, uint32_t plane) { return (uint32_t)nt * plane; }
    static __device__ __forceinline__ void store(void* h, uint32_t at, uint32_t nl, float g, float u) {
        store_y<DT>(h, at + nl, swiglu16<DT>(g, u));  // exact: a 16-bit value
    }
    static __device__ __forceinline__ u32x2 pack4(const f32x4 (&s)[2]) {
        const f32x4 g = s[0], u = s[1];
        return u32x2{pack2<DT>(swiglu16<DT>(g.x, u.x), swiglu16<DT>(g.y, u.y)),
                     pack2<DT>(swiglu16<DT>(g.z, u.z), swiglu16<DT>(g.w, u.w))};
    }
};

// What the pipeline needs to know of a launch, whatever the kernel's own argument struct.
struct MtJob {
    const void* x;      // [.][K]
    void* y;            // [rows][N]
    float* slab;        // [ksplit][planes][rows][N] (ksplit > 1)
    uint32_t* ticket;   // this tile's ticket
    char* smem;         // the two x buffers
    const float* lut;   // the 16 codes in LDS
    uint32_t* flag;     // 4 bytes of LDS for "I am the last slice"
    uint32_t yrows, N, K;            // yrows: rows of y and of a slab plane
    uint32_t tile;                   // column tile
    uint32_t ks, ksplit, cps, chunks;  // this K slice, K slices, chunks per slice, K / 128
};

// The chunk loop of one K slice: acc[mt][nt] += x tile mt . strip nt.  SB: keep a
// sched_barrier(0) behind every batch of x fragment reads.  Ends behind a workgroup barrier.
template <int DT, int MT, int SM, int WV, bool SB, class Rows, class Strips>
__device__ inline void mt_accumulate(f32x4 (&acc)[MT][kMtStrips], const MtJob& job, const Rows& rows, const Strips& st) {
    constexpr uint32_t T = 64u * WV;
    constexpr uint32_t kBuf = 16u * MT * kMtRowBytes;
    constexpr int NP = 16 * MT * 16 / (int)T;  // 16-byte pieces of a stage per thread
    static_assert(16 * MT * 16 % T == 0, "a stage divides over the threads");
    char* smem = job.smem;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t col0 = job.tile * (Strips::kWaveCols * WV) + wave * Strips::kWaveCols;
    const uint32_t c_begin = job.ks * job.cps < job.chunks ? job.ks * job.cps : job.chunks;
    const uint32_t c_end = c_begin + job.cps < job.chunks ? c_begin + job.cps : job.chunks;
    const uint32_t bpr = job.K >> 6, kb = job.K >> 1;

    // Loads run ahead of the MFMAs in registers: the weights (HBM) kWD chunks, x (L2) two.
    // Slots are compile-time (the chunk loop is unrolled by kWD), chunk numbers past the
    // slice's end are clamped to its last chunk -- a repeated load, never a branch, so the
    // compiler's wait counts stay exact.
    constexpr int kWD = 4;
    constexpr int kXS = kMtXSets<MT, WV>;
    constexpr int NPR = kXS == 2 ? NP : NP / 2;  // one set: the stage in two halves, half the registers
    u32x4 xr[kXS][NPR];
    MtW w[kWD];
    const uint32_t n = c_end - c_begin;  // chunks of this slice
    auto chunk_at = [&](uint32_t i) { return c_begin + (i < n ? i : n - 1u); };
    // (staged rows >= count load the last row again and are zeroed on their way into LDS: an
    // in-bounds repeat, no branch around a load, so the compiler counts the loads in flight exactly)
    auto xload = [&](auto S, uint32_t c, int half = 0) {
        const char* xg = reinterpret_cast<const char*>(job.x);
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const uint32_t p = tid + (uint32_t)(i + half * NPR) * T, row = p >> 4, seg = p & 15u;
            const uint32_t r = rows.x_row(row < rows.count ? row : rows.count - 1u);
            xr[S][i] = *reinterpret_cast<const u32x4*>(xg + (r * job.K + c * kChunkK + seg * 8u) * 2u);  // < 2^31: validated
        }
    };
    auto xstore = [&](auto S, char* buf, int half = 0) {
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const uint32_t p = tid + (uint32_t)(i + half * NPR) * T, row = p >> 4, seg = p & 15u;
            const u32x4 v = row < rows.count ? xr[S][i] : u32x4{0u, 0u, 0u, 0u};  // rows >= count: zeros in LDS
            *reinterpret_cast<u32x4*>(buf + row * kMtRowBytes + ((seg + mt_rot(row)) & 15u) * 16u) = v;
        }
    };
    auto wload = [&](auto S, uint32_t c) {
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) {
            const uint32_t r = st.row(col0, nt) + nl;
            w[S].w[nt] = *reinterpret_cast<const u32x4*>(st.packed[st.wt(nt)] + (r * kb + c * 64u + 16u * kh));  // < 2^31: validated
            const uint32_t f = r * bpr + 2u * c + (kh >> 1);  // 64-block on the weight's flat stream
            if constexpr (SM == kScaleBnb) {
                w[S].qa[nt] = st.a1[st.wt(nt)][f];
                w[S].qb[nt] = st.a2[st.wt(nt)][f >> st.sh2[st.wt(nt)]];
            } else {
                w[S].qa[nt] = 0u;
                w[S].qb[nt] = st.a2[st.wt(nt)][f];
            }
        }
    };

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

    const char* t = reinterpret_cast<const char*>(job.lut);
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
        for (int nt = 0; nt < kMtStrips; ++nt) sc[nt] = block_scale<SM>(st.c2tab + 256 * st.wt(nt), cur.qa[nt], cur.qb[nt], st.off[st.wt(nt)]);
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
            for (int nt = 0; nt < kMtStrips; ++nt) bw[nt] = mt_decode<DT>(t, cur.w[nt][s], sc[nt]);
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
                if constexpr (SB) __builtin_amdgcn_sched_barrier(0);  // the batch is issued here, not where it is used
            }
            if (s < 3) {
                if constexpr (kAF == 2) {
                    aread(af[(s + 1) & 1], s + 1);
                    if constexpr (SB) __builtin_amdgcn_sched_barrier(0);
                }
                decode(bw[(s + 1) & 1], s + 1);
            }
            if constexpr (kXS == 1)
                if (s == 2) {  // first half of x[i + 1] lands in the other buffer, the second half sets out
                    xstore(I0{}, smem + (uint32_t)((j + 1) & 1) * kBuf, 0);
                    xload(I0{}, chunk_at(i + 1u), 1);
                }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < kMtStrips; ++nt)
                    acc[mt][nt] = mt_mfma<DT>(af[s & (kAF - 1)][mt], bw[s & 1][nt], acc[mt][nt]);
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
}

// Publish a slice's slab stores and draw the tile's ticket: every wave's stores done, then ONE
// agent-scope release ahead of the ticket.  True in the whole workgroup of the slice that drew
// the last ticket: it has acquired every slice's stores and put the ticket back to 0.
__device__ inline bool mt_publish_last(uint32_t* ticket_at, uint32_t ksplit, uint32_t* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(ticket_at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = ticket == ksplit - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket_at, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next call
        }
        *flag = last ? 1u : 0u;
    }
    __syncthreads();
    return *flag != 0u;
}

// The reducer: every slice's tile in slice order, 4 columns per thread and element, cleared
// behind it.  The slabs come from other XCDs' stores: a thread's loads of one slice (all its kE
// elements of every plane) are in flight together, so the tile costs one round trip per slice;
// each element's sum still runs in slice order.  Elements past the tile repeat its last one (an
// in-bounds load, no branch) and are not stored.
template <int DT, int MT, int WV, class Strips, class Out, class Rows>
__device__ inline void mt_reduce(const MtJob& job, const Rows& rows) {
    constexpr uint32_t T = 64u * WV, COLS = Strips::kWaveCols * WV, PL = Out::kPlanes;
    constexpr int kE = 16 * MT * (int)(COLS / 4u) / (int)T;  // elements per thread and plane at 16 MT rows
    const uint32_t tid = threadIdx.x;
    const uint32_t total = rows.count * (COLS / 4u);
    const uint32_t plane = job.yrows * job.N;  // floats per plane; every slice's planes < 2^30 floats: validated
    uint32_t at[kE];
    f32x4 sum[kE][PL];
#pragma unroll
    for (int j = 0; j < kE; ++j) {
        const uint32_t e0 = tid + (uint32_t)j * T, e = e0 < total ? e0 : total - 1u;
        at[j] = rows.y_row(e / (COLS / 4u)) * job.N + job.tile * COLS + 4u * (e % (COLS / 4u));
    }
    for (uint32_t sl = 0; sl < job.ksplit; ++sl) {
        f32x4 v[kE][PL];
#pragma unroll
        for (int j = 0; j < kE; ++j)
#pragma unroll
            for (uint32_t pl = 0; pl < PL; ++pl)
                v[j][pl] = *reinterpret_cast<const f32x4*>(job.slab + (PL * sl + pl) * plane + at[j]);
#pragma unroll
        for (int j = 0; j < kE; ++j)
#pragma unroll
            for (uint32_t pl = 0; pl < PL; ++pl) {
                if (sl == 0u) sum[j][pl] = v[j][pl];  // the first slice starts the sum: -0 stays -0
                else {
                    sum[j][pl].x += v[j][pl].x;
                    sum[j][pl].y += v[j][pl].y;
                    sum[j][pl].z += v[j][pl].z;
                    sum[j][pl].w += v[j][pl].w;
                }
            }
    }
#pragma unroll
    for (int j = 0; j < kE; ++j)
        if (tid + (uint32_t)j * T < total) {
            for (uint32_t sl = 0; sl < PL * job.ksplit; ++sl)
                *reinterpret_cast<f32x4*>(job.slab + sl * plane + at[j]) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(job.y) + at[j]) = Out::pack4(sum[j]);
        }
}

// What becomes of the accumulators: acc[mt][nt][i] is strip nt's sum for staged row
// 16 mt + 4 kh + i.  One slice: stored through the output policy.  More: to this slice's slab,
// and the slice that draws the last ticket reduces.
template <int DT, int MT, int WV, class Strips, class Out, class Rows>
__device__ inline void mt_finish(const f32x4 (&acc)[MT][kMtStrips], const MtJob& job, const Rows& rows) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t col0 = job.tile * (Strips::kWaveCols * WV) + wave * Strips::kWaveCols;
    if (job.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
                if (m < rows.count) Out::store(job.y, rows.y_row(m) * job.N + col0, nl, acc[mt][0][i], acc[mt][1][i]);
            }
        return;
    }
    const uint32_t plane = job.yrows * job.N;
    float* mine = job.slab + (size_t)job.ks * Out::kPlanes * plane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
            if (m < rows.count) {
                const uint32_t at = rows.y_row(m) * job.N + col0;
#pragma unroll
                for (int nt = 0; nt < kMtStrips; ++nt) mine[at + Out::slab_at(nt, plane) + nl] = acc[mt][nt][i];
            }
        }
    if (mt_publish_last(job.ticket, job.ksplit, job.flag)) mt_reduce<DT, MT, WV, Strips, Out>(job, rows);
}

// The whole pipeline of one workgroup: its K slice's chunk loop, then the accumulators' way out.
template <int DT, int MT, int SM, int WV, bool SB, class Out, class Rows, class Strips>
__device__ inline void mt_pipeline(const MtJob& job, const Rows& rows, const Strips& st) {
    f32x4 acc[MT][kMtStrips];
    mt_accumulate<DT, MT, SM, WV, SB>(acc, job, rows, st);
    mt_finish<DT, MT, WV, Strips, Out>(acc, job, rows);
}

}  // namespace
