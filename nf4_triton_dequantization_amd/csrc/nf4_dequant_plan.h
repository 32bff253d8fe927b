// nf4_dequant_plan.h -- the host-side plan of the dequant library, plain C++17 (no HIP):
// the constants host and kernels agree on, the kernel-argument images, every entry point's
// validation and the choice of kernel, grid and arguments of every launch a call makes.
// Pure arithmetic of the call's arguments (pointers only for their alignment, never read
// through) and the CU count, shared by the kernels and entry points (nf4_dequant.hip) and
// a CPU check (tests/plan/dequant_plan_check.cpp) that pins the choices without a GPU.
//
// Each plan_* function validates as its entry point always did and then hands every launch
// of the call, in order, to a sink `emit(const Launch&) -> int`; a non-zero answer ends the
// call with that code.  Which kernel a matrix takes (plan_matrix, top to bottom):
//   flat    n % 64 == 0, dense rows, aligned pointers: one byte stream (flat1: one matrix
//           under the default grid); above kSegBytes as several segments of one launch
//   chunk-dense / piece / piece32 / chunk<LW, SW>   every other shape (plan_chunks)
//   rows    past the chunk kernels' 32-bit limits, or NF4DQ_CFG_ROWS
// and the bitsandbytes stream: flat (numel % 8 == 0, aligned), else bnb-bytes.
#pragma once

#include <stdint.h>

#include "../../include/nf4_dequant.h"
#include "nf4_fastdiv.h"

// Hooks of tools/dq_variants.hip and the stamps build that the host side sees too (the
// rest, and what they mean, are in nf4_dequant.hip).
#ifndef NF4_FLAT_STAMPS
#define NF4_FLAT_STAMPS 0
#endif
#ifndef NF4_DQ_FLAT1
#define NF4_DQ_FLAT1 1
#endif
#ifndef NF4_DQ_FLAT_WAVES
#define NF4_DQ_FLAT_WAVES 4
#endif
#ifndef NF4_DQ_U
#define NF4_DQ_U 4
#endif

namespace nf4dq {

enum Mode : int { kRef = 0, kSingle = 1, kBnb = 2, kBnbSingle = 3 };

constexpr int kWg = 256;   // rows / bitsandbytes-bytes kernels: 4 waves per workgroup
constexpr int kFlatWaves = NF4_DQ_FLAT_WAVES;  // the flat kernel's workgroup
constexpr int kFlatWg = 64 * kFlatWaves;
constexpr int kU = NF4_DQ_U;  // packed dwords (fp32 output: words) per lane per tile

template <int DT>
constexpr uint32_t out_bytes_per_packed_byte() { return DT == NF4DQ_F32 ? 8u : 4u; }
// Packed bytes a lane loads per step j: 4 (-> 8 outputs = 16 B of fp16/bf16) or,
// for fp32 output, 2 (-> 4 outputs = 16 B).  Either way every lane stores 16 B
// per step and a wave store instruction covers 1 KiB contiguous.
template <int DT>
constexpr uint32_t lane_bytes() { return DT == NF4DQ_F32 ? 2u : 4u; }
template <int DT>
constexpr uint32_t tile_bytes() { return 64u * lane_bytes<DT>() * kU; }

constexpr nf4_launch_cfg kDefaultCfg = {4, 0, 1, 0};  // measured best at 4096^2 (tools/tune.py)

// Buffer descriptors address < 4 GiB: one flat descriptor holds < 2^29 packed bytes
// (2 GiB of 16-bit / 4 GiB of fp32 output).  Bigger matrices (a 70B model's
// 128256 x 8192 lm_head) go as several segments of one launch, each carrying its
// first scale block (Desc::blk_base); block indices stay < 2^31.
constexpr int64_t kSegBytes = int64_t(1) << 29;
constexpr int64_t kMaxFlatBlocks = int64_t(1) << 31;

// Kernel-argument image of one matrix (or one segment of it) on the flat path.
struct Desc {
    const uint32_t* packed;  // dense packed stream (4-byte aligned)
    const uint8_t* a1;       // uint8 absmax (ref, bnb)
    const float* a2;         // nested absmax (ref, bnb) or fp32 absmax (single modes)
    const float* code2;      // bnb nested code book (256 fp32)
    void* out;               // 16-byte aligned output
    float offset;            // bnb offset
    uint32_t nbytes;         // packed bytes (multiple of 4)
    uint32_t tile_begin;     // first tile of this matrix within the launch
    uint32_t groups;         // ceil(bpr/4) (ref)
    FastDiv nb;              // ref: modulus of A1 index
    FastDiv n2;              // ref: modulus of A2 index; single: .d = row stride
    FastDiv bpr;             // blocks per row
    uint32_t blk_shift;      // log2(bytes per scale block)
    uint32_t blk2_shift;     // bnb: log2(blocksize2)
    uint32_t blk_base;       // scale blocks before this segment
};

template <int MAXB>
struct Batch {
    Desc d[MAXB];
    uint32_t count;
    uint32_t total_tiles;
#if NF4_FLAT_STAMPS
    unsigned long long* stamps;  // diagnostic build only (tools/Makefile `stamps`)
#endif
};

// Any shape, reference / single-quant semantics: one thread per packed byte.
struct RowsArgs {
    const uint8_t* packed;
    const uint8_t* a1;
    const float* a2;
    void* out;
    int64_t m, n, stride, cols_b;  // cols_b = ceil(n/2) packed bytes used per row
    int64_t nb, n2, bpr, groups, rs;
};

struct ChunkArgs {
    const uint8_t* packed;
    const uint8_t* a1;
    const float* a2;
    void* out;
    uint64_t packed_len;  // bytes (the load range)
    uint64_t out_elems;   // m * n
    uint32_t stride;      // packed bytes per row
    uint32_t n;           // columns
    uint32_t chunks;      // m * L
    FastDiv L;            // chunks per row
    FastDiv bpr;          // 64-column blocks per row
    uint32_t groups;      // ceil(bpr / 4)
    FastDiv nb, n2;       // ref: moduli of the absmax / nested-absmax indices
    uint32_t rs;          // single: absmax per row
};

struct PieceArgs {
    const uint8_t* packed;  // the packed weight aligned down to 4 bytes
    const uint8_t* a1;
    const float* a2;
    void* line;             // the output's first 128-byte line
    void* out;
    uint32_t prange;        // load range from `packed` (bytes)
    uint32_t kb;            // the weight's first byte, from `packed` (0..3)
    uint32_t sa;            // the output's first element, from `line` (0..63)
    uint32_t elems;         // m * n
    uint32_t n, half;       // columns; ceil(n / 2)
    uint32_t stride;        // packed bytes per row (>= half; > half: padded rows)
    FastDiv nf, bpr;        // n; 64-column blocks per row
    uint32_t groups;        // ceil(bpr / 4)
    FastDiv nb, n2;         // ref: moduli of the absmax / nested-absmax indices
    uint32_t rs;            // single: absmax per row
};

// Any length, bitsandbytes semantics: one thread per packed byte.
struct BnbBytesArgs {
    const uint8_t* packed;
    const uint8_t* a1;
    const float* code2;
    const float* a2;
    void* out;
    float offset;
    int64_t numel;
    int32_t blk_shift_elems, blk2_shift;
    int32_t single;
};

// One launch: the kernel family, its template parameters, the launch shape and the
// argument image (valid while the sink that receives it runs).
enum Family : int { kFlat1 = 0, kFlat, kChunkDense, kPiece, kPiece32, kChunk, kRows, kBnbBytes };

struct Launch {
    int family, dtype, mode;
    int p0, p1;  // kFlat: MAXB, -; kChunk: LW, SW; kPiece / kPiece32: RE, TRI
    uint32_t grid, block;
    uint32_t count;    // matrices in the launch
    const void* args;  // Batch<MAXB> (kFlat1: Batch<1>), ChunkArgs, PieceArgs, RowsArgs or BnbBytesArgs
    template <class T>
    const T& as() const { return *static_cast<const T*>(args); }
};

inline bool valid_dtype(int32_t d) { return d == NF4DQ_F16 || d == NF4DQ_BF16 || d == NF4DQ_F32; }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int ilog2(uint64_t v) {
    int s = 0;
    while ((uint64_t(1) << s) < v) ++s;
    return s;
}

inline FastDiv clamped_fastdiv(int64_t d) {  // moduli above 2^31 never wrap for indices < 2^31
    return make_fastdiv((uint32_t)(d > (int64_t(1) << 31) ? (int64_t(1) << 31) : d));
}

inline unsigned rows_grid(int64_t work) {
    int64_t b = (work + kWg - 1) / kWg;
    if (b > 65536) b = 65536;  // grid-stride beyond this
    if (b < 1) b = 1;
    return (unsigned)b;
}

// ---- the flat path -------------------------------------------------------------
// One flat launch of the descriptors callers filled (nothing when there are none): their
// tile offsets for the dtype's tile, and the grid.  cfg: grid cap (blocks_per_cu),
// validated by the caller.
template <int MAXB, class Emit>
int emit_flat(Batch<MAXB>& b, int dtype, int mode, const nf4_launch_cfg& cfg, int cus, Emit& emit) {
    if (b.count == 0) return NF4DQ_OK;
    const uint32_t tb = dtype == NF4DQ_F32 ? tile_bytes<NF4DQ_F32>() : tile_bytes<NF4DQ_BF16>();
    b.total_tiles = 0;
    for (uint32_t i = 0; i < b.count; ++i) {
        b.d[i].tile_begin = b.total_tiles;
        b.total_tiles += (b.d[i].nbytes + tb - 1u) / tb;
    }
    uint64_t blocks = (b.total_tiles + kFlatWaves - 1) / kFlatWaves;
    // nf4_flat1_kernel for the default grid only: a call that names a cap (nf4_dequant_ref_cfg)
    // keeps nf4_flat_kernel whether or not the cap binds, so tuning runs and the tests have
    // the loop kernel to compare against at any size
    const bool flat1 = MAXB == 1 && NF4_DQ_FLAT1 && cfg.blocks_per_cu <= 0;
    if (cfg.blocks_per_cu > 0) {
        const uint64_t cap = (uint64_t)cfg.blocks_per_cu * (uint64_t)cus;
        if (blocks > cap) blocks = cap;
    }
    return emit(Launch{flat1 ? kFlat1 : kFlat, dtype, mode, MAXB, 0, (uint32_t)blocks, (uint32_t)kFlatWg, b.count, &b});
}

// Append one flat stream of `nbytes` packed bytes (`proto`: the descriptor of its start) to
// the batch, as segments of `seg` bytes -- whole rows, whole scale blocks -- launching the
// batch whenever it is full.  (A full batch is the only flush: 24 descriptors of < 2^29
// bytes are < 2^25 tiles of 512 bytes, far from any 32-bit tile count.)
template <class Emit>
int append_segments(Batch<NF4DQ_BATCH_MAX>& b, const Desc& proto, int64_t nbytes, int64_t seg, int dtype, int mode,
                    Emit& emit) {
    const int64_t ob = dtype == NF4DQ_F32 ? 8 : 4;  // output bytes per packed byte
    for (int64_t p0 = 0; p0 < nbytes; p0 += seg) {
        Desc& d = b.d[b.count++];
        d = proto;
        d.packed = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(proto.packed) + p0);
        d.out = reinterpret_cast<uint8_t*>(proto.out) + p0 * ob;
        d.nbytes = (uint32_t)(nbytes - p0 < seg ? nbytes - p0 : seg);
        d.blk_base = (uint32_t)(p0 >> proto.blk_shift);
        if (b.count == NF4DQ_BATCH_MAX) {
            const int rc = emit_flat(b, dtype, mode, kDefaultCfg, 0, emit);
            if (rc) return rc;
            b.count = 0;
        }
    }
    return NF4DQ_OK;
}

// A flat stream on its own: one descriptor (the only case a cfg applies to), or segments.
template <class Emit>
int plan_flat_stream(const Desc& proto, int64_t nbytes, int64_t seg, int dtype, int mode, const nf4_launch_cfg& cfg,
                     int cus, Emit& emit) {
    if (nbytes < kSegBytes) {
        Batch<1> b{};
        b.d[0] = proto;
        b.d[0].nbytes = (uint32_t)nbytes;
        b.count = 1;
        return emit_flat(b, dtype, mode, cfg, cus, emit);
    }
    Batch<NF4DQ_BATCH_MAX> b{};
    const int rc = append_segments(b, proto, nbytes, seg, dtype, mode, emit);
    return rc ? rc : emit_flat(b, dtype, mode, kDefaultCfg, 0, emit);
}

// ---- reference / single semantics -------------------------------------------------
// Validation shared by the reference-semantics entry points (mirrors what the
// reference's .view(m, -1) and slicing accept, kernel_optimized.py:229, :288-312).
inline int check_common(const uint8_t* packed, int64_t packed_len, const void* out, int32_t dtype, int64_t m,
                        int64_t n) {
    if (!valid_dtype(dtype)) return NF4DQ_ERR_ARG;
    if (m < 0 || n < 0 || packed_len < 0) return NF4DQ_ERR_ARG;
    if (m == 0 || n == 0) return NF4DQ_OK;
    if (!packed || !out) return NF4DQ_ERR_ARG;
    if (packed_len % m) return NF4DQ_ERR_SHAPE;
    if (packed_len / m < (n + 1) / 2) return NF4DQ_ERR_SHAPE;
    return NF4DQ_OK;
}

// nf4_dequant_ref_cfg's cfg: null = the default
inline int check_cfg(const nf4_launch_cfg* cfg, nf4_launch_cfg& c) {
    c = cfg ? *cfg : kDefaultCfg;
    if (c.tile_dwords != 4 || c.nontemporal != 1 || c.blocks_per_cu < 0) return NF4DQ_ERR_ARG;
    if (c.flags & ~(NF4DQ_CFG_ROWS | NF4DQ_CFG_CHUNKS)) return NF4DQ_ERR_ARG;
    if ((c.flags & NF4DQ_CFG_ROWS) && (c.flags & NF4DQ_CFG_CHUNKS)) return NF4DQ_ERR_ARG;
    return NF4DQ_OK;
}

// One validated, non-empty matrix.  Reference mode: a1[nb], a2[n2]; single mode: a2 is the
// fp32 absmax with rs entries per row (a1 null, nb = n2 = 0).
struct Matrix {
    const uint8_t* packed;
    int64_t packed_len;
    const uint8_t* a1;
    int64_t nb;
    const float* a2;
    int64_t n2, rs;
    void* out;
    int64_t m, n;
};

inline bool flat_eligible(const uint8_t* packed, int64_t packed_len, const void* out, int64_t m, int64_t n) {
    return n % 64 == 0 && packed_len == m * (n / 2) && n / 2 < kSegBytes && packed_len / 32 < kMaxFlatBlocks &&
           aligned(packed, 4) && aligned(out, 16);
}

// A flat-eligible matrix's descriptor (of the whole matrix: segments set their own
// range) and its segment size, as many whole rows as stay under kSegBytes.
inline Desc flat_desc(const Matrix& x, int mode) {
    Desc d{reinterpret_cast<const uint32_t*>(x.packed), x.a1, x.a2, nullptr, x.out};
    const int64_t bpr = (x.n + 63) / 64;
    d.groups = (uint32_t)((bpr + 3) / 4);
    d.nb = clamped_fastdiv(mode == kRef ? x.nb : 1);
    d.n2 = clamped_fastdiv(mode == kRef ? x.n2 : x.rs);
    d.bpr = make_fastdiv((uint32_t)bpr);
    d.blk_shift = 5;  // 64 elements = 32 packed bytes
    return d;
}
inline int64_t row_segment(int64_t n) { return (kSegBytes - 1) / (n / 2) * (n / 2); }

// Fill the chunk kernel's shape fields, or return false when the matrix is past its
// limits: every index it forms is 32-bit (chunks, blocks, scale indices, offsets within
// the rows one wave's 256 chunks touch) and its stores need element-aligned output.
inline bool chunk_args(ChunkArgs& A, const Matrix& x, int32_t dtype) {
    const int64_t stride = x.packed_len / x.m;
    const int64_t L = ((x.n + 1) / 2 + 3) / 4;
    const int64_t bpr = (x.n + 63) / 64;
    const int64_t ob = dtype == NF4DQ_F32 ? 4 : 2;
    const int64_t span = 256 / L + 2;  // rows one wave touches, at most
    const int64_t lim = int64_t(1) << 31;
    if (x.m * L >= lim - 1024 || x.m * bpr >= lim || x.n >= (int64_t(1) << 28) || span * stride >= lim ||
        span * x.n * ob >= lim || !aligned(x.out, (uintptr_t)ob))
        return false;
    A.packed = x.packed;
    A.a1 = x.a1;
    A.a2 = x.a2;
    A.out = x.out;
    A.packed_len = (uint64_t)x.packed_len;
    A.out_elems = (uint64_t)(x.m * x.n);
    A.stride = (uint32_t)stride;
    A.n = (uint32_t)x.n;
    A.chunks = (uint32_t)(x.m * L);
    A.L = make_fastdiv((uint32_t)L);
    A.bpr = make_fastdiv((uint32_t)bpr);
    A.groups = (uint32_t)((bpr + 3) / 4);
    return true;
}

// The dense form's shapes (checked first).
inline bool dense_eligible(const ChunkArgs& A, int32_t dtype) {
    return dtype != NF4DQ_F32 && A.L.d >= 64u && A.stride == 4u * A.L.d && A.n % 8u == 0 && aligned(A.packed, 4) &&
           aligned(A.out, 16) && A.chunks < (1u << 27);
}

// The piece kernels' shapes: rows of >= 512 elements (a step then crosses at most one row end)
// the dense form does not take (16-bit output: n % 8 != 0, padded rows, the output off
// 16-byte alignment or the packed weight off 4-byte alignment; fp32: every such shape), and
// offsets below 2^31.
inline bool piece_eligible(const ChunkArgs& A, int32_t dtype) {
    const uint64_t half = (A.n + 1u) / 2u;
    const uint64_t rows = A.out_elems / A.n;
    const uint64_t ob = dtype == NF4DQ_F32 ? 4u : 2u;
    // (padded 16-bit rows the chunk kernel stores whole, n % 8 == 0 and an aligned output,
    // stay there: the same time, two loads fewer per piece; profiles/r06/chunk/s22)
    if (A.stride != half && dtype != NF4DQ_F32 && A.n % 8u == 0 && aligned(A.out, 16)) return false;
    return A.stride >= half && A.packed_len == rows * A.stride && A.n >= 512u &&
           ob * (A.out_elems + 64u) < (uint64_t(1) << 31) && A.packed_len + 8u < (uint64_t(1) << 31);
}

// A piece kernel's launch, its arguments from the chunk kernel's.
template <class Emit>
int plan_pieces(const ChunkArgs& A, int32_t dtype, int mode, Emit& emit) {
    const uint32_t ob = dtype == NF4DQ_F32 ? 4u : 2u, per = 16u / ob;  // output bytes, elements per piece
    const uintptr_t pw = (uintptr_t)A.packed, ow = (uintptr_t)A.out;
    const uint32_t kb = (uint32_t)(pw & 3u), sa = (uint32_t)((ow & 127u) / ob);
    const PieceArgs P{reinterpret_cast<const uint8_t*>(pw & ~uintptr_t(3)), A.a1, A.a2,
                      reinterpret_cast<void*>(ow & ~uintptr_t(127)), A.out,
                      (uint32_t)((kb + A.packed_len + 3u) & ~uint64_t(3)), kb, sa,  // prange, kb, sa
                      (uint32_t)A.out_elems, A.n, (A.n + 1u) / 2u, A.stride,        // elems, n, half, stride
                      make_fastdiv(A.n), A.bpr, A.groups, A.nb, A.n2, A.rs};        // nf, bpr, groups, nb, n2, rs
    const uint32_t pieces = (P.sa + P.elems + per - 1u) / per;
    const unsigned g = (pieces + 1023u) / 1024u;  // 4 waves x 256 pieces
    // RE, a piece's elements past its row's end: 2 padded rows, 1 odd n (a pad nibble), 0 the stream runs on
    const int re = P.stride != P.half ? 2 : (P.n & 1u) ? 1 : 0;
    // TRI: the last block of a row is shorter than a piece (a piece can hold three blocks)
    const uint32_t tail = P.n % 64u;
    const int tri = tail != 0u && tail < per;
    return emit(Launch{dtype == NF4DQ_F32 ? kPiece32 : kPiece, dtype, mode, re, tri, g, (uint32_t)kWg, 1u, &P});
}

// The kernel of a matrix off the flat path and within chunk_args' limits.
template <class Emit>
int plan_chunks(const ChunkArgs& A, int32_t dtype, int mode, Emit& emit) {
    const unsigned g = (unsigned)((A.chunks + 1023u) / 1024u);  // 4 waves x 256 chunks
    if (dense_eligible(A, dtype)) return emit(Launch{kChunkDense, dtype, mode, 0, 0, g, (uint32_t)kWg, 1u, &A});
    if (piece_eligible(A, dtype)) return plan_pieces(A, dtype, mode, emit);
    // LW 4: dword loads; 1: two aligned dwords per chunk joined.  SW 16: a chunk's outputs in
    // 16-byte stores; 4: 16-bit outputs staged through LDS, fp32 stored by element
    const int lw = aligned(A.packed, 4) && A.stride % 4 == 0 ? 4 : 1;
    const int sw = A.n % (dtype == NF4DQ_F32 ? 4 : 8) == 0 && aligned(A.out, 16) ? 16 : 4;
    return emit(Launch{kChunk, dtype, mode, lw, sw, g, (uint32_t)kWg, 1u, &A});
}

template <class Emit>
int plan_matrix(const Matrix& x, int32_t dtype, int mode, const nf4_launch_cfg& cfg, int cus, Emit& emit) {
    const bool single = mode == kSingle;
    const bool absmax32 = !single || x.m * x.rs < (int64_t(1) << 31);  // single: 32-bit absmax indices
    if (!cfg.flags && absmax32 && flat_eligible(x.packed, x.packed_len, x.out, x.m, x.n))
        return plan_flat_stream(flat_desc(x, mode), x.packed_len, row_segment(x.n), dtype, mode, cfg, cus, emit);
    ChunkArgs C{};
    if (!(cfg.flags & NF4DQ_CFG_ROWS) && absmax32 && chunk_args(C, x, dtype)) {
        if (single) {
            C.rs = (uint32_t)x.rs;
        } else {
            C.nb = clamped_fastdiv(x.nb);
            C.n2 = clamped_fastdiv(x.n2);
        }
        return plan_chunks(C, dtype, mode, emit);
    }
    const int64_t bpr = (x.n + 63) / 64;
    const RowsArgs A{x.packed, x.a1, x.a2, x.out, x.m, x.n, x.packed_len / x.m, (x.n + 1) / 2,
                     x.nb,     x.n2, bpr,  single ? 0 : (bpr + 3) / 4, x.rs};
    return emit(Launch{kRows, dtype, mode, 0, 0, rows_grid(x.m * A.cols_b), (uint32_t)kWg, 1u, &A});
}

// nf4_dequant_ref and, with a cfg that passed check_cfg, nf4_dequant_ref_cfg.
template <class Emit>
int plan_ref(const uint8_t* packed, int64_t packed_len, const uint8_t* a1, int64_t nb, const float* a2, int64_t n2,
             void* out, int32_t dtype, int64_t m, int64_t n, const nf4_launch_cfg& cfg, int cus, Emit& emit) {
    const int rc = check_common(packed, packed_len, out, dtype, m, n);
    if (rc || m == 0 || n == 0) return rc;
    if (!a1 || !a2 || nb <= 0 || n2 <= 0) return NF4DQ_ERR_ARG;
    return plan_matrix(Matrix{packed, packed_len, a1, nb, a2, n2, 0, out, m, n}, dtype, kRef, cfg, cus, emit);
}

template <class Emit>
int plan_single(const uint8_t* packed, int64_t packed_len, const float* absmax, int64_t absmax_len, void* out,
                int32_t dtype, int64_t m, int64_t n, Emit& emit) {
    const int rc = check_common(packed, packed_len, out, dtype, m, n);
    if (rc || m == 0 || n == 0) return rc;
    if (!absmax || absmax_len < 0) return NF4DQ_ERR_ARG;
    if (absmax_len % m || absmax_len / m < (n + 63) / 64) return NF4DQ_ERR_SHAPE;
    return plan_matrix(Matrix{packed, packed_len, nullptr, 0, absmax, 0, absmax_len / m, out, m, n}, dtype, kSingle,
                       kDefaultCfg, 0, emit);
}

// Flat matrices share launches, in order; any other one is launched where it stands.
template <class Emit>
int plan_ref_batched(const nf4_matrix_desc* descs, int32_t count, int32_t dtype, Emit& emit) {
    if (count < 0 || (count > 0 && !descs)) return NF4DQ_ERR_ARG;
    if (!valid_dtype(dtype)) return NF4DQ_ERR_ARG;
    // Validate everything before launching anything.
    for (int32_t i = 0; i < count; ++i) {
        const nf4_matrix_desc& d = descs[i];
        const int rc = check_common(d.packed, d.packed_len, d.out, dtype, d.m, d.n);
        if (rc) return rc;
        if (d.m == 0 || d.n == 0) continue;
        if (!d.absmax_q || !d.absmax2 || d.nb <= 0 || d.n2 <= 0) return NF4DQ_ERR_ARG;
    }
    Batch<NF4DQ_BATCH_MAX> b{};
    for (int32_t i = 0; i < count; ++i) {
        const nf4_matrix_desc& d = descs[i];
        if (d.m == 0 || d.n == 0) continue;
        const Matrix x{d.packed, d.packed_len, d.absmax_q, d.nb, d.absmax2, d.n2, 0, d.out, d.m, d.n};
        const int rc = flat_eligible(d.packed, d.packed_len, d.out, d.m, d.n)
                           ? append_segments(b, flat_desc(x, kRef), d.packed_len, row_segment(d.n), dtype, kRef, emit)
                           : plan_matrix(x, dtype, kRef, kDefaultCfg, 0, emit);
        if (rc) return rc;
    }
    return emit_flat(b, dtype, kRef, kDefaultCfg, 0, emit);
}

// ---- bitsandbytes semantics --------------------------------------------------------
// nf4_dequant_bnb and (single: a2 is the fp32 absmax, blocksize2 = 1) nf4_dequant_bnb_single.
template <class Emit>
int plan_bnb(const uint8_t* packed, const uint8_t* a1, int64_t nb, const float* code2, const float* a2, int64_t n2,
             float offset, void* out, int32_t dtype, int64_t numel, int32_t blocksize, int32_t blocksize2, bool single,
             Emit& emit) {
    if (!valid_dtype(dtype)) return NF4DQ_ERR_ARG;
    if (numel < 0) return NF4DQ_ERR_ARG;
    if (numel == 0) return NF4DQ_OK;
    if (!packed || !out || !a2) return NF4DQ_ERR_ARG;
    if (blocksize < 64 || (blocksize & (blocksize - 1))) return NF4DQ_ERR_ARG;
    const int64_t nblk = (numel + blocksize - 1) / blocksize;
    if (nb < nblk) return NF4DQ_ERR_SHAPE;
    if (!single) {
        if (!a1 || !code2) return NF4DQ_ERR_ARG;
        if (blocksize2 <= 0 || (blocksize2 & (blocksize2 - 1))) return NF4DQ_ERR_ARG;
        if (n2 < (nblk + blocksize2 - 1) / blocksize2) return NF4DQ_ERR_SHAPE;
    }
    const int mode = single ? kBnbSingle : kBnb;
    if (numel % 8 == 0 && nblk < kMaxFlatBlocks && blocksize <= (1 << 28) && aligned(packed, 4) && aligned(out, 16)) {
        Desc d{reinterpret_cast<const uint32_t*>(packed), a1, a2, code2, out, offset};
        d.blk_shift = (uint32_t)ilog2((uint64_t)blocksize / 2);
        d.blk2_shift = single ? 0u : (uint32_t)ilog2((uint64_t)blocksize2);
        // (segments of kSegBytes / 2: a multiple of every block's byte count)
        return plan_flat_stream(d, numel / 2, kSegBytes / 2, dtype, mode, kDefaultCfg, 0, emit);
    }
    const BnbBytesArgs A{packed, a1, code2, a2, out, offset, numel, ilog2((uint64_t)blocksize),
                         single ? 0 : ilog2((uint64_t)blocksize2), single ? 1 : 0};
    return emit(Launch{kBnbBytes, dtype, mode, 0, 0, rows_grid((numel + 1) / 2), (uint32_t)kWg, 1u, &A});
}

}  // namespace nf4dq
