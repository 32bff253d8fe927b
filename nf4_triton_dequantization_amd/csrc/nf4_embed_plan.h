// nf4_embed_plan.h -- the host-side plan of the NF4 embedding gather (nf4_embedding_bnb*),
// plain C++17 (no HIP): the kernel-argument image, the entry points' validation and the
// form, grid and constants of the launch a call makes.  Pure arithmetic of the call's
// arguments (pointers only for null and alignment, never read through), shared by the
// kernels and device entries (nf4_embed.hip), the host entries (nf4_dequant_cpu.cpp) and a
// CPU check (tests/plan/embed_plan_check.cpp) that pins the choices without a GPU.
//
// Forms:
//   aligned   dim % 64 == 0 (and packed 4-byte, out 16-byte aligned: every torch tensor):
//             a 64-element output block lies in one row and one statistics block; 8 lanes
//             own it and walk `steps` blocks: 1 while the output has at most
//             kEmbedSmallBlocks blocks (decode sizes: four times the workgroups, each lane's
//             chain of loads, table and store once), kEmbedSteps above (the staging of the
//             nested code is shared by four times the output).  A workgroup covers
//             (kEmbedWg / 8) * steps consecutive output blocks.
//   general   any other dim or alignment: one thread per output element.
//
// The too-large rule: a call is ONE launch, and the kernels index the output with 32 bits
// (and divide with nf4_fastdiv.h, exact below 2^31), so count * dim > kEmbedMaxElems
// = 2^31 - 1 is NF4DQ_ERR_TOO_LARGE -- refused, never split: a caller that gathers more
// than 2^31 elements at once splits `ids` itself.  So is a table whose rows * dim does not
// fit 2^62 (row bases are formed in int64).
#pragma once

#include <stdint.h>

#include "../../include/nf4_dequant.h"
#include "nf4_fastdiv.h"

namespace nf4dq {

enum EmbedForm : int { kEmbedAligned = 0, kEmbedGeneral = 1 };

constexpr int kEmbedWg = 256;          // both forms: 4 waves per workgroup
constexpr int kEmbedSteps = 4;         // aligned: output blocks per 8-lane group of a large launch
constexpr int64_t kEmbedSmallBlocks = 32768;  // aligned: up to here one block per group (512 rows of 4096)
constexpr int64_t kEmbedMaxElems = (int64_t(1) << 31) - 1;
constexpr int64_t kEmbedMaxTable = int64_t(1) << 62;

// Kernel-argument image (both forms).
struct EmbedArgs {
    const void* ids;        // int32 / int64 [count]
    const uint8_t* packed;  // the table's flat stream
    const uint8_t* a1;      // nested: uint8 absmax
    const float* a2;        // nested: absmax2; single: the fp32 absmax
    const float* code2;     // nested: 256 fp32
    const float* offset;    // nested: one fp32 or null (= 0); read by the kernel
    void* out;
    int64_t rows, dim;
    uint32_t elems;         // count * dim
    uint32_t blocks;        // aligned: count * dim / 64
    FastDiv bpr;            // aligned: dim / 64, 64-element blocks per row
    uint32_t blk_shift;     // log2(blocksize)
    uint32_t blk2_shift;    // log2(blocksize2)
};

// What a call does: an error, nothing (count == 0), or one launch over output elements
// [elem_begin, elem_end).
struct EmbedPlan {
    int rc;
    int launches;  // 0 or 1
    int form;
    int steps;  // aligned: output blocks per 8-lane group (1 or kEmbedSteps)
    uint32_t grid, block;
    int64_t elem_begin, elem_end;
    EmbedArgs args;
};

// The call as the entry points receive it (`single`: a2 / n2 are the fp32 absmax and its
// length, a1 / code2 / offset / blocksize2 ignored).
struct EmbedCall {
    const void* ids;
    int32_t ids_dtype;
    int64_t count;
    const uint8_t* packed;
    const uint8_t* a1;
    int64_t nb;
    const float* code2;
    const float* a2;
    int64_t n2;
    const float* offset;
    int32_t blocksize, blocksize2;
    void* out;
    int32_t out_dtype;
    int64_t rows, dim;
    bool single;
};

inline bool embed_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

inline uint32_t embed_log2(uint64_t v) {
    uint32_t s = 0;
    while ((uint64_t(1) << s) < v) ++s;
    return s;
}

inline bool embed_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline EmbedPlan plan_embed(const EmbedCall& c) {
    EmbedPlan P{};
    auto fail = [&](int rc) {
        P.rc = rc;
        return P;
    };
    if (c.ids_dtype != NF4DQ_IDS_I32 && c.ids_dtype != NF4DQ_IDS_I64) return fail(NF4DQ_ERR_ARG);
    if (c.out_dtype != NF4DQ_F16 && c.out_dtype != NF4DQ_BF16 && c.out_dtype != NF4DQ_F32) return fail(NF4DQ_ERR_ARG);
    if (c.blocksize < 64 || c.blocksize > 4096 || !embed_pow2(c.blocksize)) return fail(NF4DQ_ERR_ARG);
    if (!c.single && (c.blocksize2 < 4 || !embed_pow2(c.blocksize2))) return fail(NF4DQ_ERR_ARG);
    if (c.count < 0 || c.rows < 0 || c.dim < 0 || c.nb < 0 || (!c.single && c.n2 < 0)) return fail(NF4DQ_ERR_SHAPE);
    if (c.count == 0) return P;  // NF4DQ_OK, nothing launched
    if (!c.ids || !c.packed || !c.out || !c.a2) return fail(NF4DQ_ERR_ARG);
    if (!c.single && (!c.a1 || !c.code2)) return fail(NF4DQ_ERR_ARG);
    if (c.dim < 1) return fail(NF4DQ_ERR_SHAPE);
    if (c.rows > kEmbedMaxTable / c.dim) return fail(NF4DQ_ERR_TOO_LARGE);
    const int64_t numel = c.rows * c.dim;
    const int64_t nblk = (numel + c.blocksize - 1) / c.blocksize;
    if (c.nb < nblk) return fail(NF4DQ_ERR_SHAPE);
    if (!c.single && c.n2 < (nblk + c.blocksize2 - 1) / c.blocksize2) return fail(NF4DQ_ERR_SHAPE);
    if (c.count > kEmbedMaxElems / c.dim) return fail(NF4DQ_ERR_TOO_LARGE);
    const int64_t elems = c.count * c.dim;
    const int64_t esize = c.out_dtype == NF4DQ_F32 ? 4 : 2;
    // ids and out aligned to their elements: anything less is not a tensor of that type
    if (!embed_aligned(c.ids, c.ids_dtype == NF4DQ_IDS_I64 ? 8 : 4) || !embed_aligned(c.out, (uintptr_t)esize) ||
        !embed_aligned(c.a2, 4) || (!c.single && (!embed_aligned(c.code2, 4) || !embed_aligned(c.offset, 4))))
        return fail(NF4DQ_ERR_ARG);

    EmbedArgs& A = P.args;
    A.ids = c.ids;
    A.packed = c.packed;
    A.a1 = c.single ? nullptr : c.a1;
    A.a2 = c.a2;
    A.code2 = c.single ? nullptr : c.code2;
    A.offset = c.single ? nullptr : c.offset;
    A.out = c.out;
    A.rows = c.rows;
    A.dim = c.dim;
    A.elems = (uint32_t)elems;
    A.blk_shift = embed_log2((uint64_t)c.blocksize);
    A.blk2_shift = c.single ? 0u : embed_log2((uint64_t)c.blocksize2);
    P.launches = 1;
    P.block = (uint32_t)kEmbedWg;
    P.elem_begin = 0;
    P.elem_end = elems;
    if (c.dim % 64 == 0 && embed_aligned(c.packed, 4) && embed_aligned(c.out, 16)) {
        P.form = kEmbedAligned;
        A.blocks = (uint32_t)(elems / 64);
        A.bpr = make_fastdiv((uint32_t)(c.dim / 64));
        P.steps = elems / 64 <= kEmbedSmallBlocks ? 1 : kEmbedSteps;
        const int64_t wg_blocks = (kEmbedWg / 8) * P.steps;
        P.grid = (uint32_t)((elems / 64 + wg_blocks - 1) / wg_blocks);
    } else {
        P.form = kEmbedGeneral;
        P.steps = 1;
        A.blocks = 0;
        A.bpr = FastDiv{1u, 0u, 0u};
        P.grid = (uint32_t)((elems + kEmbedWg - 1) / kEmbedWg);  // < 2^23
    }
    return P;
}

}  // namespace nf4dq
