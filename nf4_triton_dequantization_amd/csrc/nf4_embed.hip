// nf4_embed.hip -- MI355X (gfx950 / CDNA4) NF4 embedding gather: rows ids[i] of a
// [rows, dim] bitsandbytes NF4 table, dequantized into out[count][dim], bit for bit what
// nf4_dequant_bnb / nf4_dequant_bnb_single write for those elements (nf4_dequant.hip, bnb
// mode).  Only the selected rows' packed bytes and statistics are read; the offset is read
// on the device; an id outside [0, rows) gives a row of zero bits and reads nothing.
//
// Both kernels walk the OUTPUT, which is one contiguous stream of count * dim elements; only
// the source is indexed.
//  * aligned form (dim % 64 == 0): a 64-element output block never crosses a row or a
//    statistics block.  The 8 lanes of a group own output block u: row slot u / (dim / 64)
//    (nf4_fastdiv.h), source block ids[slot] * (dim / 64) + u % (dim / 64) in 64 bits, 4
//    packed bytes per lane, the block scale once per lane (the group's loads hit one
//    address), and for 16-bit outputs the per-block LDS table of the flat dequant kernel
//    (block_table_write / block_table_decode): 16 bytes stored per lane, a wave's store
//    instruction writing 1 KiB contiguous.  fp32 outputs multiply per element and store two
//    16-byte pieces per lane.  A group walks STEPS blocks (1 at decode sizes, kEmbedSteps for
//    large outputs: nf4_embed_plan.h), all of their loads issued before the first decode;
//    the 256-entry nested code and the 16 codes are staged in LDS once per workgroup and the
//    offset is one scalar load at entry.
//  * general form (any other dim, or pointers off the aligned form's alignment): one thread
//    per output element in the manner of nf4_bnb_bytes_kernel, so that rows starting
//    mid-byte or mid-block are handled per element.  Exact, not fast.
// Plain loads and stores: the output is read next by the layer that follows, and the few
// table rows a call touches are not a stream.  What a call launches is decided in
// nf4_embed_plan.h (plain C++, pinned without a GPU by tests/test_embed_plan_cpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nf4_dequant.h"
#include "nf4_common.h"
#include "nf4_embed_plan.h"

namespace {

using namespace nf4dq;

// ids[slot], sign-extended (so that the range check below is the one of the id's own signed type).
template <int IDT>
__device__ __forceinline__ int64_t load_id(const void* ids, uint32_t slot) {
    if constexpr (IDT == NF4DQ_IDS_I64) return reinterpret_cast<const int64_t*>(ids)[slot];
    else return (int64_t) reinterpret_cast<const int32_t*>(ids)[slot];
}

__device__ __forceinline__ bool id_in_range(int64_t id, int64_t rows) { return id >= 0 && id < rows; }

// Scale of statistics block b.  (-ffp-contract=off: the product and the sum round apart.)
template <bool SINGLE>
__device__ __forceinline__ float block_scale(const EmbedArgs& A, int64_t b, const float* code2s, float off) {
    if constexpr (SINGLE) {
        return A.a2[b];
    } else {
        return code2s[A.a1[b]] * A.a2[b >> A.blk2_shift] + off;
    }
}

template <int DT, int IDT, bool SINGLE, int STEPS>
__global__ __launch_bounds__(kEmbedWg) void nf4_embed_aligned_kernel(const EmbedArgs A) {
    __shared__ __attribute__((aligned(16))) float lut[16];
    __shared__ __attribute__((aligned(16))) float code2s[SINGLE ? 1 : 256];
    constexpr bool kTbl = DT != NF4DQ_F32;
    __shared__ __attribute__((aligned(256))) char tbl[kTbl ? (kEmbedWg / 64) * 2048 : 4];  // 8 block tables per wave
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = lane & 7u;
    float off = 0.0f;
    float c2w = 0.0f;
    if constexpr (!SINGLE) {
        if (A.offset) off = *A.offset;
        c2w = A.code2[threadIdx.x & 255u];
    }
    // This group's output blocks: step j of wave w of workgroup g owns blocks
    // ((g * waves + w) * STEPS + j) * 8 .. + 7, one per group of 8 lanes.
    const uint32_t u0 = ((blockIdx.x * (kEmbedWg / 64) + (threadIdx.x >> 6)) * STEPS) * 8u + (lane >> 3);
    // The ids go out first; the code tables are staged and the workgroup meets under their
    // latency (the code word was issued before them, so its wait does not cover them), and
    // only then does anything wait for an id.
    int64_t id[STEPS];
    uint32_t col[STEPS];  // this block's index within its row
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
        // (past the end of the output: the last block's id, loaded without a branch -- a
        // branch would make the wait below cover the ids -- and never used)
        const uint32_t u = min(u0 + 8u * j, A.blocks - 1u);
        const uint32_t slot = fdiv(u, A.bpr);
        col[j] = u - slot * A.bpr.d;
        id[j] = load_id<IDT>(A.ids, slot);
    }
    write_lut(lut);
    if constexpr (!SINGLE) code2s[threadIdx.x & 255u] = c2w;
    __syncthreads();
    bool ok[STEPS];
    uint32_t w[STEPS];
    uint32_t q[STEPS];
    float a2[STEPS];
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
        ok[j] = u0 + 8u * j < A.blocks && id_in_range(id[j], A.rows);
        w[j] = 0u;
        q[j] = 0u;
        a2[j] = 0.0f;
        if (ok[j]) {  // an id out of range reads nothing from the table
            const int64_t sb = id[j] * (int64_t)A.bpr.d + (int64_t)col[j];  // source block of the table's stream
            w[j] = reinterpret_cast<const uint32_t*>(A.packed)[sb * 8 + k];
            const int64_t b = sb >> (A.blk_shift - 6u);
            if constexpr (SINGLE) {
                a2[j] = A.a2[b];
            } else {
                q[j] = A.a1[b];
                a2[j] = A.a2[b >> A.blk2_shift];
            }
        }
    }
    const uint32_t tb = ((threadIdx.x >> 6) << 11) + ((lane >> 3) << 8);
    const f32x2 c01 = *reinterpret_cast<const f32x2*>(lut + 2u * k);
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
        const uint32_t u = u0 + 8u * j;
        float s;
        if constexpr (SINGLE) s = a2[j];
        else s = code2s[q[j]] * a2[j] + off;
        const uint32_t e = u * 64u + 8u * k;  // this lane's first output element (< 2^31)
        if constexpr (kTbl) {
            block_table_write<DT>(tbl, tb, k, c01, s);
            u32x4 o = block_table_decode(tbl, tb, w[j]);
            if (!ok[j]) o = u32x4{0u, 0u, 0u, 0u};  // zero bits, not the -0 of a zero scale
            if (u < A.blocks) reinterpret_cast<u32x4*>(A.out)[e >> 3] = o;
        } else {
            const uint32_t hi4 = (w[j] >> 2) & 0x3C3C3C3Cu;
            const uint32_t lo4 = (w[j] << 2) & 0x3C3C3C3Cu;
            const char* t = reinterpret_cast<const char*>(lut);
            uint32_t v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = __float_as_uint(*reinterpret_cast<const float*>(t + ((hi4 >> (8 * i)) & 0xFFu)) * s);
                v[2 * i + 1] = __float_as_uint(*reinterpret_cast<const float*>(t + ((lo4 >> (8 * i)) & 0xFFu)) * s);
            }
            if (!ok[j]) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = 0u;
            }
            if (u < A.blocks) {
                u32x4* dst = reinterpret_cast<u32x4*>(A.out) + (e >> 2);
                dst[0] = u32x4{v[0], v[1], v[2], v[3]};
                dst[1] = u32x4{v[4], v[5], v[6], v[7]};
            }
        }
    }
}

// Any dim and alignment: one thread per output element.
template <int DT, int IDT, bool SINGLE>
__global__ __launch_bounds__(kEmbedWg) void nf4_embed_general_kernel(const EmbedArgs A) {
    __shared__ __attribute__((aligned(16))) float lut[16];
    write_lut(lut);
    __syncthreads();
    const uint32_t o = blockIdx.x * (uint32_t)kEmbedWg + threadIdx.x;
    if (o >= A.elems) return;
    const uint32_t dim = (uint32_t)A.dim;  // dim <= count * dim < 2^31
    const uint32_t slot = o / dim;
    const uint32_t col = o - slot * dim;
    const int64_t id = load_id<IDT>(A.ids, slot);
    float x = 0.0f;
    if (id_in_range(id, A.rows)) {
        const int64_t e = id * A.dim + (int64_t)col;
        const uint32_t byte = A.packed[e >> 1];
        const uint32_t nib = (e & 1) ? (byte & 15u) : (byte >> 4);
        float off = 0.0f;
        if constexpr (!SINGLE) {
            if (A.offset) off = *A.offset;
        }
        x = lut[nib] * block_scale<SINGLE>(A, e >> A.blk_shift, A.code2, off);
    }
    store1<DT>(A.out, (int64_t)o, x);
}

inline int hip_rc(hipError_t e) { return e == hipSuccess ? NF4DQ_OK : NF4DQ_ERR_HIP_BASE + (int)e; }

template <int DT, int IDT, bool SINGLE>
void launch(const EmbedPlan& P, hipStream_t st) {
    if (P.form == kEmbedAligned && P.steps == 1)
        hipLaunchKernelGGL((nf4_embed_aligned_kernel<DT, IDT, SINGLE, 1>), dim3(P.grid), dim3(P.block), 0, st, P.args);
    else if (P.form == kEmbedAligned)
        hipLaunchKernelGGL((nf4_embed_aligned_kernel<DT, IDT, SINGLE, kEmbedSteps>), dim3(P.grid), dim3(P.block), 0, st,
                           P.args);
    else
        hipLaunchKernelGGL((nf4_embed_general_kernel<DT, IDT, SINGLE>), dim3(P.grid), dim3(P.block), 0, st, P.args);
}

template <int DT, bool SINGLE>
void launch_ids(const EmbedPlan& P, int32_t ids_dtype, hipStream_t st) {
    if (ids_dtype == NF4DQ_IDS_I64) launch<DT, NF4DQ_IDS_I64, SINGLE>(P, st);
    else launch<DT, NF4DQ_IDS_I32, SINGLE>(P, st);
}

// The entry points only ask the plan and launch.
template <bool SINGLE>
int run(const EmbedCall& c, void* hip_stream) {
    const EmbedPlan P = plan_embed(c);
    if (P.rc != NF4DQ_OK || P.launches == 0) return P.rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (c.out_dtype == NF4DQ_BF16) launch_ids<NF4DQ_BF16, SINGLE>(P, c.ids_dtype, st);
    else if (c.out_dtype == NF4DQ_F16) launch_ids<NF4DQ_F16, SINGLE>(P, c.ids_dtype, st);
    else launch_ids<NF4DQ_F32, SINGLE>(P, c.ids_dtype, st);
    return hip_rc(hipGetLastError());
}

}  // namespace

extern "C" {

int nf4_embedding_bnb(const void* ids, int32_t ids_dtype, int64_t count, const uint8_t* packed,
                      const uint8_t* absmax_q, int64_t nb, const float* code2, const float* absmax2, int64_t n2,
                      const float* offset, int32_t blocksize, int32_t blocksize2, void* out, int32_t out_dtype,
                      int64_t rows, int64_t dim, void* hip_stream) {
    const EmbedCall c{ids, ids_dtype, count, packed, absmax_q, nb, code2, absmax2, n2, offset,
                      blocksize, blocksize2, out, out_dtype, rows, dim, false};
    return run<false>(c, hip_stream);
}

int nf4_embedding_bnb_single(const void* ids, int32_t ids_dtype, int64_t count, const uint8_t* packed,
                             const float* absmax, int64_t nabs, int32_t blocksize, void* out, int32_t out_dtype,
                             int64_t rows, int64_t dim, void* hip_stream) {
    const EmbedCall c{ids, ids_dtype, count, packed, nullptr, nabs, nullptr, absmax, 0, nullptr,
                      blocksize, 0, out, out_dtype, rows, dim, true};
    return run<true>(c, hip_stream);
}

}  // extern "C"
