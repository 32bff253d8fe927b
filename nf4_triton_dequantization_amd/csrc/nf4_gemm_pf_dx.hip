// nf4_gemm_pf_dx.hip -- the fused input-gradient GEMM of an NF4 weight in bitsandbytes semantics
// for 1..8192 rows (nf4_gemm_bnb_pf_dx, nf4_gemm_bnb_pf_dx_single): kernel, launcher and C
// entries.  The plan -- validation, cfg, geometry, LDS, workspace -- is nf4_gemm_pf_dx_plan.h.
//
// dx[M][K] = g[M][N] . W[N][K] with W the 16-bit weights nf4_dequant_bnb writes, bit for bit: the
// whole backward of a frozen Linear4bit.  It is the prefill GEMM (nf4_gemm_pf.hip) with the
// reduction over N and the output columns along K -- and that turns the weight side round.  A
// weight row is contiguous along k (one packed byte holds k and k + 1 of ONE n, one statistics
// block covers 64 k of ONE n), while the MFMA's A fragment wants eight consecutive n of one k.
// So:
//  * a workgroup of WV waves (4 / 8) owns BM = 32 WV rows of g (128 / 256), 128 output columns
//    k0 .. k0 + 127 and one slice of N; a wave 64 x 64 of it as 4 x 4 MFMA tiles of 16 x 16
//    (f32_16x16x32), 64 accumulator registers over the whole loop -- as the prefill kernel;
//  * N moves in steps of 64 weight rows.  g is staged as the prefill kernel stages x: BM x 64
//    values per step as 16-byte loads, four per thread, into rotated 128-byte rows;
//  * the step's packed weights W[n0 .. n0 + 63][k0 .. k0 + 127] are 64 rows of 64 bytes, loaded
//    row-wise (16 bytes per thread under 4 waves, 8 under 8: every row one coalesced 64-byte
//    read) and staged RAW in LDS, 4 KiB per buffer.  A row sits at
//        (n >> 2) * 256 + ((n + (n >> 3)) & 3) * 64, its 16-byte pieces rotated by 2 (n >> 5),
//    which puts the eight rows n = 8 q + r (q = 0 .. 7) a wave's decode reads at once on eight
//    different groups of four banks;
//  * the step's 128 block scales -- block (n0 + n) K / 64 + k0 / 64 + kb, gathered at a stride of
//    K / 64 -- are formed ONCE, by 128 threads, into an LDS table [2 kb][64 n] of floats:
//    code2[a1[f]] * a2[f >> sh2] + offset, or a2[f] for single statistics;
//  * the decode transposes.  Thread (q, kg) of the workgroup reads the packed bytes of its
//    1024 / T output columns (4 or 2 k: two bytes or one) in the eight rows n = 8 q .. 8 q + 7 and
//    their eight scales, and makes one 16-byte slot per k: eight consecutive n of one k, each
//    mt_decode's arithmetic -- the fp32 product of code and that ROW's block scale, RNE to 16
//    bits, the oracle's weight.  The tile is written as [128 k][64 n] in the prefill kernel's
//    layout: row k is 128 bytes, slot q (n = 8 q .. 8 q + 7 of the step) rotated by (k >> 1) & 3.
//    A weight is decoded once per workgroup and step, whatever BM is; no lane shuffles;
//  * the MFMA loop is the prefill kernel's: the decoded tile is the A operand, g the B operand,
//    both read with ds_read_b128 at slot 4 (kh & 1) + 2 (kh >> 1) + s -- the same permutation of
//    the step's n on both, so the sum is the plain one -- and a lane holds FOUR CONSECUTIVE
//    COLUMNS of one row of dx: 8-byte stores to dx, 16-byte stores to the slab;
//  * two buffers of each staged array, ONE barrier per step.  In step i the waves multiply step
//    i's buffers, decode step i + 1 from its raw buffer into the other decoded buffer, land g of
//    step i + 1 and the raw bytes and scales of step i + 2; the global loads of g (step i + 3)
//    and of the packed bytes and statistics (step i + 4) run ahead in two register sets each.
// Rows of a block past M repeat row M - 1 (an in-bounds load, no branch) and are never stored;
// steps past the slice's end repeat its last step into buffers nobody reads.
// Slices of N meet as the family's K slices do: fp32 slab per slice, one ticket per (row block,
// column tile) drawn through mt_publish_last; the workgroup drawing the last ticket sums the
// slabs in slice order (the first slice assigns), stores dx and puts the slab back to 0.  No
// poll, no float atomics.  The result is a function of the inputs and the cfg alone, and a row's
// bits do not depend on the rows around it: the n order of a row's sum is fixed by the cfg.
// (dx_rot, dx_reduce and the MFMA step repeat nf4_gemm_pf.hip's: that file's code is not touched.)
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_pf_dx_plan.h"

namespace {

struct DxArgs {
    const uint8_t* packed;  // [N][K/2]
    const uint8_t* a1;      // nested: absmax bytes [N K / 64]
    const float* a2;        // nested: absmax2; single: the fp32 absmax
    const float* code2;     // nested: [256]
    const float* offset;    // nested: [1] or null (= 0)
    const void* g;          // [M][N]
    void* dx;               // [M][K]
    float* slab;            // [ksplit][M][K] (ksplit > 1)
    uint32_t* counters;     // one ticket per (row block, column tile)
    uint32_t M, N, K;
    uint32_t ksplit, sps, steps, tiles;  // slices of N, steps per slice, N / 64, K / 128
    uint32_t sh2;           // log2(blocksize2)
};

// Slot rotation of a staged row of g or of decoded weights (the prefill kernel's).
__device__ __forceinline__ uint32_t dx_rot(uint32_t row) { return (row >> 1) & 3u; }

// Where piece `seg` (16 bytes) of packed row n of the step sits in a raw buffer (see the header comment).
__device__ __forceinline__ uint32_t dx_raw_at(uint32_t n, uint32_t seg) {
    return (n >> 2) * 256u + ((n + (n >> 3)) & 3u) * 64u + ((seg + 2u * (n >> 5)) & 3u) * 16u;
}

// The transposed decode of one thread: SPT slots (output columns kg SPT .. kg SPT + SPT - 1) of
// the eight weight rows n = 8 q .. 8 q + 7.  t: the 16 codes in LDS; raw, sb: the step's packed
// bytes and block scales; wb: the decoded tile [128 k][64 n].
template <int DT, int SPT>
__device__ __forceinline__ void dx_decode(const char* t, const char* raw, const float* sb, char* wb, uint32_t q, uint32_t kg) {
    constexpr uint32_t BPT = SPT / 2;  // packed bytes per row: 2 / 1
    static_assert(SPT == 4 || SPT == 2, "two bytes or one per row");
    const uint32_t k0 = kg * SPT, cb = kg * BPT, seg = cb >> 4, within = cb & 15u;
    const float* sp = sb + (k0 >> 6) * kDxStepN + 8u * q;  // the rows' scales in this k's statistics block
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
    const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    uint32_t hi4[8], lo4[8];  // code * 4 of the even / odd k of every byte
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        const char* p = raw + dx_raw_at(8u * q + r, seg) + within;
        const uint32_t w = BPT == 2 ? (uint32_t)*reinterpret_cast<const uint16_t*>(p) : (uint32_t)*reinterpret_cast<const uint8_t*>(p);
        hi4[r] = (w >> 2) & 0x3C3Cu;
        lo4[r] = (w << 2) & 0x3C3Cu;
    }
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)SPT; ++j) {
        float v[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
            const uint32_t at = (((j & 1u) ? lo4[r] : hi4[r]) >> (8u * (j >> 1))) & 0xFFu;
            v[r] = *reinterpret_cast<const float*>(t + at) * sc[r];
        }
        const uint32_t k = k0 + j;
        *reinterpret_cast<u32x4*>(wb + k * kPfRowBytes + ((q + dx_rot(k)) & 7u) * 16u) =
            u32x4{pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]), pack2<DT>(v[4], v[5]), pack2<DT>(v[6], v[7])};
    }
}

// The reducer of one (row block, column tile): `live` rows of 32 float4, four elements per
// thread in flight per slice, each element summed in slice order, cleared behind the sum.
// Elements past the tile repeat its last one (an in-bounds load, no branch) and are not stored.
template <int DT, int WV>
__device__ inline void dx_reduce(const DxArgs& A, uint32_t row0, uint32_t live, uint32_t col0) {
    constexpr uint32_t T = 64u * WV, kE = 4;
    const uint32_t total = live * (kDxCols / 4u), plane = A.M * A.K;  // < 2^30 floats: validated
    for (uint32_t b0 = 0; b0 < total; b0 += kE * T) {  // (a workgroup-uniform trip count)
        const uint32_t base = b0 + threadIdx.x;
        uint32_t at[kE];
        f32x4 sum[kE];
#pragma unroll
        for (uint32_t j = 0; j < kE; ++j) {
            const uint32_t e0 = base + j * T, e = e0 < total ? e0 : total - 1u;
            at[j] = (row0 + e / (kDxCols / 4u)) * A.K + col0 + 4u * (e % (kDxCols / 4u));
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
                *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.dx) + at[j]) =
                    u32x2{pack2<DT>(sum[j].x, sum[j].y), pack2<DT>(sum[j].z, sum[j].w)};
            }
    }
}

// (two waves per SIMD, as the prefill kernel: two 128-row workgroups or one 256-row one on a CU)
template <int DT, int SM, int WV>
__global__ __launch_bounds__(64 * WV, 2) void nf4_gemm_pf_dx_kernel(const DxArgs A) {
    constexpr uint32_t T = 64u * WV, BM = 32u * WV;
    constexpr uint32_t kGBuf = BM * kPfRowBytes, kWBuf = kDxCols * kPfRowBytes;
    constexpr int NP = 4;                         // 16-byte pieces of g per thread and step: BM * 8 / T
    constexpr uint32_t RP = T / kDxStepN;         // threads per packed row: 4 / 8
    constexpr int RD = 16 / (int)RP;              // packed dwords per thread and step: 4 / 2
    constexpr int SPT = (int)(kDxCols * 8u / T);  // decoded slots per thread and step: 4 / 2
    static_assert(BM * 8u == NP * T && RP * RD == 16 && SPT * T == kDxCols * 8u, "a step divides over the threads");
    // [g 0][g 1][w 0][w 1][raw 0][raw 1][scales 0][scales 1][code2][codes][flag]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* gs = smem;
    char* ws = smem + 2u * kGBuf;
    char* rs = ws + 2u * kWBuf;
    float* ss = reinterpret_cast<float*>(rs + 2u * kDxRawBytes);
    float* c2tab = ss + 2u * (kDxScaleBytes / 4u);
    float* lut = c2tab + 256;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nl = lane & 15u, kh = lane >> 4;
    const uint32_t wr = wave >> 1, wc = wave & 1u;  // the wave's 64 x 64 of the tile
    const uint32_t ks = blockIdx.x % A.ksplit, rest = blockIdx.x / A.ksplit;
    const uint32_t tile = rest % A.tiles, rb = rest / A.tiles;
    const uint32_t row0 = rb * BM, col0 = tile * kDxCols;

    if constexpr (SM == kScaleBnb)
        for (uint32_t i = tid; i < 256u; i += T) c2tab[i] = A.code2[i];
    write_lut(lut);
    const float off = load_offset<SM>(A.offset);

    const uint32_t s_begin = ks * A.sps < A.steps ? ks * A.sps : A.steps;
    const uint32_t s_end = s_begin + A.sps < A.steps ? s_begin + A.sps : A.steps;
    const uint32_t n = s_end - s_begin;  // steps of this slice
    auto step_at = [&](uint32_t i) { return s_begin + (i < n ? i : n - 1u); };

    // what a thread moves per step: NP pieces of g, RD packed dwords of weight row pn, and the
    // statistics of block (row sn, k0 / 64 + sk) -- every thread loads one (threads 128 and up
    // repeat the first 128's: no branch around a load), the first 128 put its scale into the table
    const uint32_t pn = tid / RP, ph = tid % RP;
    const uint32_t sn = tid & 63u, sk = (tid >> 6) & 1u;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;
    u32x4 gr[2][NP];
    uint32_t wq[2][RD], qa[2];
    float qb[2];
    auto loadg = [&](auto S, uint32_t st) {
        const char* gg = reinterpret_cast<const char*>(A.g);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t p = tid + (uint32_t)i * T, row = p >> 3, seg = p & 7u;
            const uint32_t r = row0 + row < A.M ? row0 + row : A.M - 1u;  // past M: row M - 1 again, never stored
            gr[S][i] = *reinterpret_cast<const u32x4*>(gg + (r * A.N + st * kDxStepN + seg * 8u) * 2u);  // < 2^31: validated
        }
    };
    auto loadw = [&](auto S, uint32_t st) {
        const uint8_t* wp = A.packed + ((st * kDxStepN + pn) * kb + (col0 >> 1) + ph * (4u * RD));  // < 2^31: validated
        if constexpr (RD == 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(wp);
            wq[S][0] = v.x, wq[S][1] = v.y, wq[S][2] = v.z, wq[S][3] = v.w;
        } else {
            const u32x2 v = *reinterpret_cast<const u32x2*>(wp);
            wq[S][0] = v.x, wq[S][1] = v.y;
        }
        const uint32_t f = (st * kDxStepN + sn) * bpr + (col0 >> 6) + sk;  // 64-block on the weight's flat stream
        if constexpr (SM == kScaleBnb) {
            qa[S] = A.a1[f];
            qb[S] = A.a2[f >> A.sh2];
        } else {
            qa[S] = 0u;
            qb[S] = A.a2[f];
        }
    };
    auto storeg = [&](auto S, uint32_t b) {
        char* gb = gs + b * kGBuf;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t p = tid + (uint32_t)i * T, row = p >> 3, seg = p & 7u;
            *reinterpret_cast<u32x4*>(gb + row * kPfRowBytes + ((seg + dx_rot(row)) & 7u) * 16u) = gr[S][i];
        }
    };
    auto storew = [&](auto S, uint32_t b) {
        char* rw = rs + b * kDxRawBytes;
        if constexpr (RD == 4) {
            *reinterpret_cast<u32x4*>(rw + dx_raw_at(pn, ph)) = u32x4{wq[S][0], wq[S][1], wq[S][2], wq[S][3]};
        } else {
            *reinterpret_cast<u32x2*>(rw + dx_raw_at(pn, ph >> 1) + 8u * (ph & 1u)) = u32x2{wq[S][0], wq[S][1]};
        }
        if (tid < 2u * kDxStepN) ss[b * (kDxScaleBytes / 4u) + sk * kDxStepN + sn] = block_scale<SM>(c2tab, qa[S], qb[S], off);
    };
    const char* t = reinterpret_cast<const char*>(lut);
    const uint32_t dq = tid & 7u, dkg = tid >> 3;  // the thread's patch of the transposed decode
    auto decode = [&](uint32_t b) {
        dx_decode<DT, SPT>(t, rs + b * kDxRawBytes, ss + b * (kDxScaleBytes / 4u), ws + b * kWBuf, dq, dkg);
    };

    f32x4 acc[4][4];  // [g row tile][column tile]
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    if (n > 0u) {
        loadg(I0{}, step_at(0));
        loadw(I0{}, step_at(0));
        loadg(I1{}, step_at(1));
        loadw(I1{}, step_at(1));
    }
    __syncthreads();  // the tables
    if (n > 0u) {
        storew(I0{}, 0u);
        loadw(I0{}, step_at(2));
        storew(I1{}, 1u);
        loadw(I1{}, step_at(3));
        storeg(I0{}, 0u);
        loadg(I0{}, step_at(2));
    }
    __syncthreads();  // the raw bytes and scales of steps 0 and 1, g of step 0
    if (n > 0u) decode(0u);
    __syncthreads();  // the first decoded tile

    const uint32_t q0 = 4u * (kh & 1u) + 2u * (kh >> 1) + dx_rot(nl);  // row 16 t + nl: the rotation depends on nl alone
    const uint32_t wfrag = (wc * 64u + nl) * kPfRowBytes, gfrag = (wr * 64u + nl) * kPfRowBytes;
    // step i of the slice (J = i & 1): its g and decoded weights are in buffers J, the raw bytes
    // and scales of step i + 1 in raw buffer J ^ 1, g of step i + 1 in register set J ^ 1, the
    // packed bytes and statistics of step i + 2 in set J (landed or in flight)
    auto step = [&](auto J, uint32_t i) {
        constexpr int j = decltype(J)::value;
        const char* gb = gs + (uint32_t)j * kGBuf + gfrag;
        const char* wb = ws + (uint32_t)j * kWBuf + wfrag;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t slot = ((q0 + (uint32_t)s) & 7u) * 16u;
            u32x4 a[4], b[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) a[ct] = *reinterpret_cast<const u32x4*>(wb + 16u * ct * kPfRowBytes + slot);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) b[mt] = *reinterpret_cast<const u32x4*>(gb + 16u * mt * kPfRowBytes + slot);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[mt][ct] = mt_mfma<DT>(a[ct], b[mt], acc[mt][ct]);
            __builtin_amdgcn_sched_barrier(0);  // one set of fragments live at a time, as in the prefill kernel
        }
        // step i + 1: its weights decoded into the other buffer, its g landed there (both last
        // read one barrier ago); step i + 2: its raw bytes and scales into raw buffer J, last read
        // by the decode of step i one barrier ago.  The freed registers take steps i + 3 and i + 4.
        decode((uint32_t)(j ^ 1));
        storeg(std::integral_constant<int, j ^ 1>{}, (uint32_t)(j ^ 1));
        loadg(std::integral_constant<int, j ^ 1>{}, step_at(i + 3u));
        storew(J, (uint32_t)j);
        loadw(J, step_at(i + 4u));
        __syncthreads();
    };
    for (uint32_t i = 0; i < n; i += 2u) {
        step(I0{}, i);
        if (i + 1u >= n) break;
        step(I1{}, i + 1u);
    }

    // acc[mt][ct][i] is dx[row0 + 64 wr + 16 mt + nl][col0 + 64 wc + 16 ct + 4 kh + i]
    const uint32_t ycol = col0 + wc * 64u + 4u * kh;
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const uint32_t m = row0 + wr * 64u + 16u * mt + nl;
            if (m < A.M)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.dx) + m * A.K + ycol + 16u * ct) =
                        u32x2{pack2<DT>(acc[mt][ct].x, acc[mt][ct].y), pack2<DT>(acc[mt][ct].z, acc[mt][ct].w)};
        }
        return;
    }
    float* mine = A.slab + ks * (A.M * A.K);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const uint32_t m = row0 + wr * 64u + 16u * mt + nl;
        if (m < A.M)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<f32x4*>(mine + m * A.K + ycol + 16u * ct) = acc[mt][ct];
    }
    if (mt_publish_last(A.counters + rb * A.tiles + tile, A.ksplit, flag))
        dx_reduce<DT, WV>(A, row0, (A.M - row0 < BM ? A.M - row0 : BM), col0);
}

template <int SM>
int launch_dx(const nf4gemm::MtCall& a, const nf4_gemm_cfg& cfg, const float* offset, hipStream_t st) {
    const PfPlan p = dx_plan(cfg, a.M, a.N, a.K);
    DxArgs A{};
    A.packed = a.packed;
    A.a1 = a.a1;
    A.a2 = a.a2;
    A.code2 = a.code2;
    A.offset = offset;
    A.g = a.x;
    A.dx = a.y;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.M = (uint32_t)a.M;
    A.N = (uint32_t)a.N;
    A.K = (uint32_t)a.K;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.sps = p.sps;
    A.steps = p.steps;
    A.tiles = p.tiles;
    A.sh2 = mt_log2_blocksize2(a.single, a.blocksize2);
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<8, 4>(cfg.waves, [&](auto WV) {
            launch_lds<&nf4_gemm_pf_dx_kernel<DT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
            rc = hip_rc2(hipGetLastError());
        });
    });
    return rc;
}

int gemm_dx_impl(const nf4gemm::MtCall& a, const float* offset, hipStream_t st) {
    nf4_gemm_cfg cfg{};
    bool launch = false;
    const int rc = dx_check(a, device_cus(), &cfg, &launch);
    if (rc || !launch) return rc;
    return a.single ? launch_dx<kScaleBnbSingle>(a, cfg, nullptr, st) : launch_dx<kScaleBnb>(a, cfg, offset, st);
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_pf_dx_workspace_bytes(int64_t M, int64_t N, int64_t K, const nf4_gemm_cfg* cfg) {
    nf4_gemm_cfg c = cfg ? *cfg : dx_default_cfg(M, N, K, device_cus());
    if (cfg && c.kernel == 0) c.kernel = NF4DQ_GEMM_PF_DX;
    return valid_dx_cfg(c, M, N, K) ? dx_workspace_need(M, N, K, c) : 0;
}

int nf4_gemm_bnb_pf_dx(const void* g, int64_t M, const uint8_t* packed, int64_t packed_len, const uint8_t* absmax_q,
                       int64_t nb, const float* code2, const float* absmax2, int64_t n2, const float* offset,
                       int32_t blocksize, int32_t blocksize2, void* dx, int32_t out_dtype, int64_t N, int64_t K,
                       void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{false, g,          M,  packed,    packed_len, absmax_q,  nb, code2,           absmax2, n2,
                            blocksize, blocksize2, dx, out_dtype, N,          K,         workspace, workspace_bytes, cfg};
    return gemm_dx_impl(a, offset, reinterpret_cast<hipStream_t>(hip_stream));
}

int nf4_gemm_bnb_pf_dx_single(const void* g, int64_t M, const uint8_t* packed, int64_t packed_len, const float* absmax,
                              int64_t nabs, int32_t blocksize, void* dx, int32_t out_dtype, int64_t N, int64_t K,
                              void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MtCall a{true,      g, M,  packed,    packed_len, nullptr, nabs, nullptr,   absmax,          nabs,
                            blocksize, 1, dx, out_dtype, N,          K,       workspace, workspace_bytes, cfg};
    return gemm_dx_impl(a, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
