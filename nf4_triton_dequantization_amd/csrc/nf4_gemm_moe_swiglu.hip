// nf4_gemm_moe_swiglu.hip -- the fused expert SwiGLU launch of a mixture-of-experts block in
// bitsandbytes semantics (nf4_gemm_bnb_moe_swiglu): kernel, launcher and C entries.  The plan --
// validation, cfg, geometry, LDS, workspace -- is nf4_gemm_moe_swiglu_plan.h.
//
// h[p][I] = silu(g) * u with g = x[p / x_div] . Wg_e^T, u = x[p / x_div] . Wu_e^T and
// e = expert_ids[p] read ON THE DEVICE: g and u what nf4_gemm_bnb_moe stores for the gate and the
// up stack (exact 16-bit weights, fp32 MFMA sums, one RNE), the chain nf4_gemm_bnb_mt_swiglu's
// (swiglu16 of nf4_gemm_mt_dev.h).  The anatomy is the expert GEMM's (nf4_gemm_moe.hip: its
// header comment gives the routing ballot, the ascending pair list, the gather and scatter, the
// zeroing of invalid-id rows by expert 0 / K slice 0 and the idle-row-tile guards -- all of them
// hold here unchanged) with the SwiGLU launch's strips:
//  * a workgroup (WV waves) owns ONE expert, 16 WV columns of h, all the expert's rows and one
//    K slice;
//  * in each wave strip 0 is rows col .. col + 15 of the expert's gate weight and strip 1 the
//    same rows of its up weight, each from its own stack: base pointers (base + e * stride),
//    statistics, blocksize2, offset (offset[e]) and code2 table (two tables in LDS, each from
//    code2 + e * code2_stride of its own stack).  acc[mt][0][i] and acc[mt][1][i] are g and u
//    of ONE element of h in one lane.
// The chunk loop is nf4_gemm_moe.hip's over MtStrips<2>, a copy of its own: the run-time
// row-tile guards keep it out of the shared loop of nf4_gemm_mt_dev.h, and the expert GEMM's
// instantiations keep the loop they were measured with.
// Split-K: two fp32 planes per slice ([ksplit][2][P][I], indexed by pair), one ticket per
// (expert, column tile); the slice that draws the last ticket sums each plane in slice order
// over the expert's listed rows and applies the chain.  Nobody waits for anybody: no poll.
#include "nf4_gemm_mt_dev.h"
#include "nf4_gemm_moe_swiglu_plan.h"

namespace {

struct MsgArgs {
    const uint8_t* packed[2];  // gate, up: [E] x [I][K/2], packed_stride bytes apart
    const uint8_t* a1[2];      // nested: absmax bytes [I K / 64] per expert, nb_stride apart
    const float* a2[2];        // nested: absmax2; single: the fp32 absmax; n2_stride floats apart
    const float* code2[2];     // nested: [256], code2_stride floats apart (0: shared)
    const float* offset[2];    // nested: [E] or null (= 0)
    const int32_t* ids;        // [P]
    const void* x;             // [ceil(P / x_div)][K]
    void* h;                   // [P][I]
    float* slab;               // [ksplit][2][P][I] (ksplit > 1)
    uint32_t* counters;        // one ticket per (expert, column tile)
    int64_t packed_stride[2], nb_stride[2], n2_stride[2], code2_stride[2];
    uint32_t P, E, I, K, x_div;
    uint32_t tiles, ksplit, cps, chunks;  // column tiles, K slices, chunks per slice, K / 128
    uint32_t sh2[2];           // log2(blocksize2)
};

// (the second launch bound, waves per SIMD: as the expert GEMM, two workgroups of 4 waves to a CU
// with two row tiles -- what the plan's K-slice rule counts on, msg_resident())
template <int DT, int MT, int SM, int WV>
__global__ __launch_bounds__(64 * WV, MT <= 2 ? 2 : 1) void nf4_gemm_moe_swiglu_kernel(const MsgArgs A) {
    using Strips = MtStrips<2>;
    constexpr uint32_t T = 64u * WV;
    constexpr uint32_t kBuf = 16u * MT * kMtRowBytes;
    constexpr int NP = 16 * MT * 16 / (int)T;  // 16-byte pieces of a stage per thread
    constexpr uint32_t COLS = Strips::kWaveCols * WV;
    static_assert(16 * MT * 16 % T == 0, "a stage divides over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [x buffer 0][x buffer 1][code2 gate][code2 up][codes][flag][x rows][h rows]
    float* c2tab = reinterpret_cast<float*>(smem + 2u * kBuf);
    float* lut = c2tab + 512;
    uint32_t* flag = reinterpret_cast<uint32_t*>(lut + 16);
    uint32_t* srow = flag + 4;                       // staged row -> row of x
    uint32_t* prow = srow + NF4DQ_MOE_MAX_PAIRS;     // staged row -> pair (row of h)

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

    if (ex == 0u && ks == 0u) {  // rows of ids outside [0, E): zero bits in this tile's columns
        const uint64_t z0 = __ballot(in0 && (uint32_t)id0 >= A.E), z1 = __ballot(in1 && (uint32_t)id1 >= A.E);
        for (int hf = 0; hf < 2; ++hf)
            for (uint64_t b = hf ? z1 : z0; b; b &= b - 1u) {
                const uint32_t p = (uint32_t)__builtin_ctzll(b) + 64u * (uint32_t)hf;
                if (tid < COLS / 4u)
                    *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(A.h) + (p * A.I + tile * COLS + 4u * tid)) = u32x2{0u, 0u};
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

    const uint32_t col0 = tile * COLS + wave * Strips::kWaveCols;
    const uint32_t c_begin = ks * A.cps < A.chunks ? ks * A.cps : A.chunks;
    const uint32_t c_end = c_begin + A.cps < A.chunks ? c_begin + A.cps : A.chunks;
    const uint32_t bpr = A.K >> 6, kb = A.K >> 1;
    Strips st{};
    st.c2tab = c2tab;
#pragma unroll
    for (int wt = 0; wt < 2; ++wt) {
        st.packed[wt] = A.packed[wt] + (int64_t)ex * A.packed_stride[wt];
        st.a1[wt] = SM == kScaleBnb ? A.a1[wt] + (int64_t)ex * A.nb_stride[wt] : nullptr;
        st.a2[wt] = A.a2[wt] + (int64_t)ex * A.n2_stride[wt];
        st.sh2[wt] = A.sh2[wt];
        if constexpr (SM == kScaleBnb) {
            const float* code2 = A.code2[wt] + (int64_t)ex * A.code2_stride[wt];
            for (uint32_t i = tid; i < 256u; i += T) c2tab[256u * wt + i] = code2[i];
        }
        st.off[wt] = load_offset<SM>(A.offset[wt] ? A.offset[wt] + ex : nullptr);
    }
    write_lut(lut);
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
        const uint32_t r = col0 + nl;                     // the same weight row in both stacks
        const uint32_t f = r * bpr + 2u * c + (kh >> 1);  // 64-block on the expert's flat stream
#pragma unroll
        for (int nt = 0; nt < kMtStrips; ++nt) {
            w[S].w[nt] = *reinterpret_cast<const u32x4*>(st.packed[nt] + (r * kb + c * 64u + 16u * kh));  // < 2^31: validated
            if constexpr (SM == kScaleBnb) {
                w[S].qa[nt] = st.a1[nt][f];
                w[S].qb[nt] = st.a2[nt][f >> st.sh2[nt]];
            } else {
                w[S].qa[nt] = 0u;
                w[S].qb[nt] = st.a2[nt][f];
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
        for (int nt = 0; nt < kMtStrips; ++nt) sc[nt] = block_scale<SM>(c2tab + 256 * nt, cur.qa[nt], cur.qb[nt], st.off[nt]);
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

    // acc[mt][0][i], acc[mt][1][i] = g, u of h[pair of staged row 16 mt + 4 kh + i][col0 + nl]
    using Out = SgOut<DT>;
    if (A.ksplit == 1u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
                if (m < cnt) Out::store(A.h, prow[m] * A.I + col0, nl, acc[mt][0][i], acc[mt][1][i]);
            }
        return;
    }
    const uint32_t plane = A.P * A.I;  // floats per plane; every slice's planes < 2^30 floats: validated
    float* mine = A.slab + (size_t)ks * Out::kPlanes * plane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t m = 16u * mt + 4u * kh + (uint32_t)i;
            if (m < cnt) {
                const uint32_t at = prow[m] * A.I + col0 + nl;
#pragma unroll
                for (int nt = 0; nt < kMtStrips; ++nt) mine[at + Out::slab_at(nt, plane)] = acc[mt][nt][i];
            }
        }
    // publish, ticket, acquire and the slice-order reducer with the chain behind it: the family's
    // (nf4_gemm_mt_dev.h), with the rows taken from the pair list and the ticket of this
    // (expert, column tile)
    const MtJob job{A.x, A.h, A.slab, A.counters + et, smem, lut, flag, A.P, A.I, A.K, tile, ks, A.ksplit, A.cps, A.chunks};
    if (mt_publish_last(job.ticket, A.ksplit, flag))
        mt_reduce<DT, MT, WV, Strips, Out>(job, MtListedRows{cnt, prow});
}

template <int SM>
int launch_msg(const nf4gemm::MsgCall& a, const nf4_gemm_cfg& cfg, hipStream_t st) {
    const nf4_moe_experts& g = a.ex[0];
    const MoePlan p = msg_plan(cfg, a.P, g.experts, g.N, g.K);
    MsgArgs A{};
    for (int i = 0; i < 2; ++i) {
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
    A.h = a.h;
    A.counters = mt_counters(a.workspace);
    A.slab = mt_slab(a.workspace, cfg);
    A.P = (uint32_t)a.P;
    A.E = (uint32_t)g.experts;
    A.I = (uint32_t)g.N;
    A.K = (uint32_t)g.K;
    A.x_div = (uint32_t)a.x_div;
    A.tiles = p.tiles;
    A.ksplit = (uint32_t)cfg.ksplit;
    A.cps = p.cps;
    A.chunks = p.chunks;
    int rc = NF4DQ_ERR_ARG;
    pick<NF4DQ_BF16, NF4DQ_F16>(a.dtype, [&](auto DT) {
        pick<2, 4, 6, 8>((int)p.row_tiles, [&](auto MT) {
            pick<4, 2>(cfg.waves, [&](auto WV) {
                launch_lds<&nf4_gemm_moe_swiglu_kernel<DT, MT, SM, WV>>(kLdsPerCu, dim3(p.grid), dim3(p.block), p.dyn, st, A);
                rc = hip_rc2(hipGetLastError());
            });
        });
    });
    return rc;
}

}  // namespace

extern "C" {

size_t nf4_gemm_bnb_moe_swiglu_workspace_bytes(int64_t P, const void* gate_up, const nf4_gemm_cfg* cfg) {
    if (!gate_up) return 0;
    const nf4_moe_experts& g = *reinterpret_cast<const nf4_moe_experts*>(gate_up);
    if (g.experts < 1 || g.experts > NF4DQ_MOE_MAX_EXPERTS) return 0;
    return msg_workspace_need(P, g.N, g.K, cfg ? *cfg : msg_default_cfg(P, g.experts, g.N, g.K, device_cus()));
}

int nf4_gemm_bnb_moe_swiglu(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* gate_up,
                            int32_t act, void* h, int32_t out_dtype, void* workspace, size_t workspace_bytes,
                            const nf4_gemm_cfg* cfg, void* hip_stream) {
    const nf4gemm::MsgCall a{x, expert_ids, P, x_div, reinterpret_cast<const nf4_moe_experts*>(gate_up), act, h, out_dtype,
                             workspace, workspace_bytes, cfg};
    nf4_gemm_cfg c{};
    bool launch = false;
    const int rc = msg_check(a, device_cus(), &c, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    return a.ex[0].single ? launch_msg<kScaleBnbSingle>(a, c, st) : launch_msg<kScaleBnb>(a, c, st);
}

}  // extern "C"
