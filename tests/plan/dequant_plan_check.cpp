// dequant_plan_check.cpp -- prints what the dequant library's host plan (nf4_dequant_plan.h)
// decides for a fixed list of cases, one compact JSON line each, integers only:
//   c   the case: [group, index within the group, entry, dtype, entry-specific shape ...]
//       entry: 0 nf4_dequant_ref, 1 _ref_cfg, 2 _single, 3 _ref_batched, 4 _bnb, 5 _bnb_single
//   pl  packed bytes of each matrix of the call (the bitsandbytes stream: ceil(numel / 2))
//   rc  what the entry returns (no launch fails here)
//   l   the launches in order, each {"k": [family, dtype, mode, p0, p1, grid, block, matrices]}
//       family: 0 flat1, 1 flat, 2 chunk-dense, 3 piece, 4 piece32, 5 chunk, 6 rows, 7 bnb-bytes;
//       p0, p1: MAXB, 0 (flat) / LW, SW (chunk) / RE, TRI (piece, piece32); and
//       flat:   "t": total tiles, "d": per descriptor [packed offset, output offset, nbytes,
//               blk_base, tile_begin, blk_shift, blk2_shift, groups, nb.d, n2.d, bpr.d]
//       others: "a": the scalar fields of the argument image, in declaration order, pointers
//               as offsets (see print_launch)
// Pointers are invented and never read through: matrix i's packed weight sits at
// kPB + (i << 38) + its low bits, its output at kOB + (i << 40) + its low bits, and the
// offsets printed are from kPB / kOB.  tests/test_dequant_plan_cpu.py builds this for the
// host (no GPU, no HIP), runs it and compares with tests/plan/dequant_plan_snapshot.jsonl.
#include <stdio.h>

#include <initializer_list>

#include "../../nf4_triton_dequantization_amd/csrc/nf4_dequant_plan.h"

using namespace nf4dq;

static const uint64_t kPB = uint64_t(1) << 46, kOB = uint64_t(1) << 52;
static const uint8_t* const kA1 = reinterpret_cast<const uint8_t*>(uintptr_t(1) << 30);
static const float* const kA2 = reinterpret_cast<const float*>(uintptr_t(1) << 31);
static const float* const kCode2 = reinterpret_cast<const float*>(uintptr_t(1) << 32);
static const int kDts[3] = {NF4DQ_BF16, NF4DQ_F16, NF4DQ_F32};

static const uint8_t* pk(int i, int64_t low) { return reinterpret_cast<const uint8_t*>(kPB + (uint64_t(i) << 38) + low); }
static void* ob(int i, int64_t low) { return reinterpret_cast<void*>(kOB + (uint64_t(i) << 40) + low); }
static long long poff(const void* p) { return (long long)(reinterpret_cast<uintptr_t>(p) - kPB); }
static long long ooff(const void* p) { return (long long)(reinterpret_cast<uintptr_t>(p) - kOB); }
static int64_t esz(int dt) { return dt == NF4DQ_F32 ? 4 : 2; }

static int g_launches;

template <int MAXB>
static void print_flat(const Batch<MAXB>& b) {
    printf(",\"t\":%u,\"d\":[", b.total_tiles);
    for (uint32_t i = 0; i < b.count; ++i) {
        const Desc& d = b.d[i];
        printf("%s[%lld,%lld,%u,%u,%u,%u,%u,%u,%u,%u,%u]", i ? "," : "", poff(d.packed), ooff(d.out), d.nbytes,
               d.blk_base, d.tile_begin, d.blk_shift, d.blk2_shift, d.groups, d.nb.d, d.n2.d, d.bpr.d);
    }
    printf("]}");
}

static int print_launch(const Launch& L) {
    printf("%s{\"k\":[%d,%d,%d,%d,%d,%u,%u,%u]", g_launches++ ? "," : "", L.family, L.dtype, L.mode, L.p0, L.p1, L.grid,
           L.block, L.count);
    if (L.family == kFlat1 || L.family == kFlat) {
        if (L.p0 == 1) print_flat(L.as<Batch<1>>());
        else print_flat(L.as<Batch<NF4DQ_BATCH_MAX>>());
    } else if (L.family == kChunkDense || L.family == kChunk) {
        const ChunkArgs& A = L.as<ChunkArgs>();
        printf(",\"a\":[%lld,%lld,%llu,%llu,%u,%u,%u,%u,%u,%u,%u,%u,%u]}", poff(A.packed), ooff(A.out),
               (unsigned long long)A.packed_len, (unsigned long long)A.out_elems, A.stride, A.n, A.chunks, A.L.d,
               A.bpr.d, A.groups, A.nb.d, A.n2.d, A.rs);
    } else if (L.family == kPiece || L.family == kPiece32) {
        const PieceArgs& A = L.as<PieceArgs>();
        printf(",\"a\":[%lld,%lld,%lld,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u]}", poff(A.packed), ooff(A.line),
               ooff(A.out), A.prange, A.kb, A.sa, A.elems, A.n, A.half, A.stride, A.nf.d, A.bpr.d, A.groups, A.nb.d,
               A.n2.d, A.rs);
    } else if (L.family == kRows) {
        const RowsArgs& A = L.as<RowsArgs>();
        printf(",\"a\":[%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld]}", poff(A.packed), ooff(A.out),
               (long long)A.m, (long long)A.n, (long long)A.stride, (long long)A.cols_b, (long long)A.nb,
               (long long)A.n2, (long long)A.bpr, (long long)A.groups, (long long)A.rs);
    } else {
        const BnbBytesArgs& A = L.as<BnbBytesArgs>();
        printf(",\"a\":[%lld,%lld,%lld,%d,%d,%d]}", poff(A.packed), ooff(A.out), (long long)A.numel, A.blk_shift_elems,
               A.blk2_shift, A.single);
    }
    return NF4DQ_OK;
}

static void open_case(int group, int idx, int entry, int dt, std::initializer_list<long long> shape,
                      std::initializer_list<long long> pl) {
    printf("{\"c\":[%d,%d,%d,%d", group, idx, entry, dt);
    for (long long v : shape) printf(",%lld", v);
    printf("],\"pl\":[");
    int i = 0;
    for (long long v : pl) printf("%s%lld", i++ ? "," : "", v);
    printf("],\"l\":[");
    g_launches = 0;
}
static void close_case(int rc) { printf("],\"rc\":%d}\n", rc); }

// ---- entries -----------------------------------------------------------------
// nf4_dequant_ref / _ref_cfg / _single of one m x n matrix: `pad` extra packed bytes per
// row, the packed weight `pb` bytes and the output `obytes` bytes off their alignment;
// nb / n2 (0: as many as the matrix has blocks / groups); single: absmax_len = m * rs
struct Mat {
    int64_t m, n, pad = 0, pb = 0, obytes = 0, nb = 0, n2 = 0, rs = 0;
};

static void ref_case(int group, int idx, int dt, const Mat& x, const nf4_launch_cfg* cfg = nullptr, int cus = 256) {
    const int64_t stride = (x.n + 1) / 2 + x.pad, plen = x.m * stride, bpr = (x.n + 63) / 64;
    const int64_t nb = x.nb ? x.nb : x.m * bpr, n2 = x.n2 ? x.n2 : x.m * ((bpr + 3) / 4);
    open_case(group, idx, cfg ? 1 : 0, dt,
              {x.m, x.n, x.pad, x.pb, x.obytes, nb, n2, cfg ? cfg->blocks_per_cu : 0, cfg ? cfg->flags : 0, cus}, {plen});
    auto emit = print_launch;
    nf4_launch_cfg c = kDefaultCfg;
    int rc = cfg ? check_cfg(cfg, c) : NF4DQ_OK;
    if (!rc) rc = plan_ref(pk(0, x.pb), plen, kA1, nb, kA2, n2, ob(0, x.obytes), dt, x.m, x.n, c, cus, emit);
    close_case(rc);
}

static void single_case(int group, int idx, int dt, const Mat& x) {
    const int64_t stride = (x.n + 1) / 2 + x.pad, plen = x.m * stride, rs = x.rs ? x.rs : (x.n + 63) / 64;
    open_case(group, idx, 2, dt, {x.m, x.n, x.pad, x.pb, x.obytes, x.m * rs}, {plen});
    auto emit = print_launch;
    close_case(plan_single(pk(0, x.pb), plen, kA2, x.m * rs, ob(0, x.obytes), dt, x.m, x.n, emit));
}

static void batched_case(int group, int idx, int dt, const Mat* xs, int count) {
    nf4_matrix_desc descs[32];
    printf("{\"c\":[%d,%d,3,%d", group, idx, dt);
    for (int i = 0; i < count; ++i) {
        const Mat& x = xs[i];
        const int64_t stride = (x.n + 1) / 2 + x.pad, bpr = (x.n + 63) / 64;
        descs[i] = nf4_matrix_desc{pk(i, x.pb), x.m * stride, kA1, x.m * bpr, kA2, x.m * ((bpr + 3) / 4),
                                   ob(i, x.obytes), x.m, x.n};
        printf(",%lld,%lld", (long long)x.m, (long long)x.n);
    }
    printf("],\"pl\":[");
    for (int i = 0; i < count; ++i) printf("%s%lld", i ? "," : "", (long long)descs[i].packed_len);
    printf("],\"l\":[");
    g_launches = 0;
    auto emit = print_launch;
    close_case(plan_ref_batched(descs, count, dt, emit));
}

static void bnb_case(int group, int idx, int dt, int64_t numel, int bs, int bs2, bool single, int64_t obytes = 0) {
    const int64_t nblk = (numel + bs - 1) / bs;
    open_case(group, idx, single ? 5 : 4, dt, {numel, bs, bs2, obytes}, {(numel + 1) / 2});
    auto emit = print_launch;
    close_case(plan_bnb(pk(0, 0), single ? nullptr : kA1, nblk, single ? nullptr : kCode2, kA2,
                        single ? 0 : (nblk + bs2 - 1) / bs2, 0.0f, ob(0, obytes), dt, numel, bs, single ? 1 : bs2,
                        single, emit));
}

// The rows of CASES in tests/test_gpu_chunks.py: (m, n, extra stride bytes, packed byte
// offset, output element offset).  tests/test_dequant_plan_cpu.py checks that the two agree.
static const int64_t kChunkCases[][5] = {
    {37, 1000, 0, 0, 0}, {5, 4080, 0, 0, 0},  {33, 1000, 4, 0, 0}, {33, 1002, 3, 0, 0}, {33, 504, 4, 0, 0},
    {33, 508, 4, 0, 0},  {9, 4080, 0, 0, 1},  {9, 4080, 4, 0, 1},  {9, 510, 4, 0, 1},   {9, 1002, 0, 0, 0},
    {9, 1002, 1, 0, 0},  {9, 506, 1, 0, 0},   {3, 6, 0, 0, 0},     {7, 77, 0, 0, 0},    {1, 1, 0, 0, 0},
    {4, 3, 0, 0, 0},     {11, 200, 3, 0, 0},  {11, 200, 4, 0, 0},  {6, 256, 2, 0, 0},   {6, 256, 0, 1, 0},
    {6, 256, 0, 2, 1},   {10, 1000, 0, 3, 3}, {10, 1000, 2, 3, 3}, {10, 510, 2, 3, 3},  {3000, 2, 0, 0, 0},
    {300, 18, 5, 0, 1},  {129, 4100, 4, 0, 0}, {129, 509, 1, 0, 0}, {9, 4090, 0, 0, 0}, {9, 4095, 0, 0, 0},
    {7, 1007, 0, 1, 37}, {5, 520, 0, 2, 63},  {6, 4096, 0, 3, 5},  {1, 600, 0, 0, 9},   {70, 521, 0, 0, 0},
    {9, 4096, 0, 1, 0},  {129, 4100, 0, 0, 0}, {9, 4097, 0, 1, 3}, {5, 577, 0, 2, 17},  {8, 515, 0, 3, 1},
    {33, 508, 2, 0, 0},  {9, 510, 1, 0, 1},
};
// The entries of FORMS in tests/test_gpu_edges.py, sorted by name: (n, extra packed bytes
// per row, packed byte offset, output element offset); every one at m = 300, every dtype.
static const int64_t kEdgeForms[][4] = {
    {510, 2, 0, 0},  {504, 4, 1, 0},  {1000, 0, 0, 0}, {509, 1, 0, 0},  {504, 4, 0, 0},   {1000, 0, 0, 0},
    {1002, 0, 0, 0}, {1007, 0, 1, 5}, {1002, 2, 0, 3}, {1027, 0, 1, 3}, {1000, 0, 0, 1},  {1002, 0, 0, 0},
    {520, 0, 3, 5},  {1007, 0, 0, 0}, {1007, 0, 1, 37}, {1002, 4, 0, 0}, {1007, 3, 1, 5}, {1029, 0, 0, 0},
    {1000, 0, 1, 0}, {77, 0, 0, 0},   {200, 0, 0, 0},  {504, 4, 0, 1},
};

int main() {
    const int64_t P29 = int64_t(1) << 29, P31 = int64_t(1) << 31;
    int idx;
    // ---- group 1: flat ----
    idx = 0;
    const int64_t flat_shapes[][2] = {{64, 64}, {1, 64}, {4096, 4096}, {2048, 8192}};
    for (int dt : kDts) {
        for (const auto& s : flat_shapes) {
            ref_case(1, idx++, dt, Mat{s[0], s[1]});
            single_case(1, idx++, dt, Mat{s[0], s[1]});
            for (int bpc : {1, 4})
                for (int cus : {256, 64}) {
                    const nf4_launch_cfg c = {4, bpc, 1, 0};
                    ref_case(1, idx++, dt, Mat{s[0], s[1]}, &c, cus);
                }
            for (int flags : {NF4DQ_CFG_CHUNKS, NF4DQ_CFG_ROWS}) {
                const nf4_launch_cfg c = {4, 0, 1, flags};
                ref_case(1, idx++, dt, Mat{s[0], s[1]}, &c);
            }
            // the packed weight off 4-byte alignment, the output off 16-byte alignment
            Mat x{s[0], s[1]};
            x.pb = 2;
            ref_case(1, idx++, dt, x);
            x.pb = 0;
            x.obytes = 8;
            ref_case(1, idx++, dt, x);
        }
        const nf4_launch_cfg null_default = kDefaultCfg;  // nf4_dequant_ref_cfg with the default cfg
        ref_case(1, idx++, dt, Mat{4096, 4096}, &null_default);
    }
    // ---- group 2: segments (n = 8192: 4096 packed bytes per row) ----
    idx = 0;
    for (int dt : kDts) {
        for (int64_t plen : {P29 - 4096, P29, P29 + 4096}) ref_case(2, idx++, dt, Mat{plen / 4096, 8192});
        ref_case(2, idx++, dt, Mat{140000, 8192});
        single_case(2, idx++, dt, Mat{140000, 8192});
        ref_case(2, idx++, dt, Mat{25 * (P29 / 4096) + 7, 8192});  // 26 segments: a flush inside the walk
        Mat small[30];
        const int64_t shapes[5][2] = {{64, 4096}, {1024, 64}, {5, 77}, {33, 11008}, {8, 96}};
        for (int i = 0; i < 30; ++i) small[i] = Mat{shapes[i % 5][0], shapes[i % 5][1]};
        batched_case(2, idx++, dt, small, 30);
        const Mat two[3] = {Mat{64, 4096}, Mat{140000, 8192}, Mat{1024, 64}};
        batched_case(2, idx++, dt, two, 3);
        const Mat mid[3] = {Mat{64, 4096}, Mat{9, 4090}, Mat{1024, 64}};  // the middle one is not flat
        batched_case(2, idx++, dt, mid, 3);
        Mat many[26];  // 23 small ones, then 2 segments: the batch fills inside a matrix
        for (int i = 0; i < 26; ++i) many[i] = Mat{64, 64};
        many[23] = Mat{140000, 8192};
        batched_case(2, idx++, dt, many, 26);
        // single mode: absmax_len just under 2^31 and at it (the flat path needs it below)
        Mat s{int64_t(1) << 21, 64};
        s.rs = 1023;
        single_case(2, idx++, dt, s);
        s.rs = 1024;
        single_case(2, idx++, dt, s);
    }
    // ---- group 3: tests/test_gpu_chunks.py CASES; group 4: tests/test_gpu_edges.py FORMS ----
    idx = 0;
    for (const auto& c : kChunkCases) {
        for (int dt : kDts) {
            Mat x{c[0], c[1], c[2], c[3], c[4] * esz(dt)};
            ref_case(3, idx, dt, x);
            single_case(3, idx, dt, x);
        }
        ++idx;
    }
    idx = 0;
    for (const auto& f : kEdgeForms) {
        for (int dt : kDts) {
            Mat x{300, f[0], f[1], f[2], f[3] * esz(dt)};
            ref_case(4, idx, dt, x);
            single_case(4, idx, dt, x);
        }
        ++idx;
    }
    // ---- group 5: the edges of the form choice ----
    idx = 0;
    for (int dt : kDts) {
        for (int64_t n : {511, 512, 513}) {  // the piece kernels take n >= 512 (512 itself only off the flat path)
            ref_case(5, idx++, dt, Mat{40, n});
            ref_case(5, idx++, dt, Mat{40, n, 0, 0, esz(dt)});
        }
        for (int64_t t : {3, 4, 5, 7, 8, 9}) ref_case(5, idx++, dt, Mat{40, 1024 + t});    // TRI: tail < 4 (fp32), < 8
        for (int64_t pad : {0, 3}) ref_case(5, idx++, dt, Mat{40, 1024 + 2, pad});         // TRI with even n, padded rows
        ref_case(5, idx++, dt, Mat{40, 1024 + 8, 4});  // padded 16-bit rows, n % 8 == 0, aligned: the chunk kernel
        Mat x{40, 1000};
        x.obytes = esz(dt) / 2;  // the output off its element alignment: the rows kernel
        ref_case(5, idx++, dt, x);
        // chunk_args' 32-bit limits, one step under and at each.  m * L (n = 8: L = bpr = 1, so
        // m * bpr never binds before it), n, span * stride (span = 258 rows at L = 1); span * n *
        // ob binds only from n = 2^28 on, for fp32, where n binds too.  Off the flat path.
        for (int64_t m : {P31 - 1025, P31 - 1024}) ref_case(5, idx++, dt, Mat{m, 8});
        for (int64_t n : {(int64_t(1) << 28) - 1, int64_t(1) << 28}) {
            Mat y{1, n};
            y.pb = 1;
            ref_case(5, idx++, dt, y);
        }
        for (int64_t stride : {8323580, 8323581}) ref_case(5, idx++, dt, Mat{2, 8, stride - 4});
        for (int64_t rs : {31, 32}) {  // single mode: m * rs below 2^31
            Mat y{int64_t(1) << 26, 8};
            y.rs = rs;
            single_case(5, idx++, dt, y);
        }
        // piece_eligible's two limits: ob * (elements + 64) and packed bytes + 8 below 2^31
        const int64_t mlim = dt == NF4DQ_F32 ? 535799 : 1071598;  // the last m under the first, n = 1002
        for (int64_t m : {mlim, mlim + 1}) ref_case(5, idx++, dt, Mat{m, 1002});
        const int64_t mp = int64_t(1) << (dt == NF4DQ_F32 ? 19 : 20);
        for (int64_t stride : {P31 / mp - 1, P31 / mp}) ref_case(5, idx++, dt, Mat{mp, 1002, stride - 501});
    }
    // ---- group 7: bitsandbytes ----
    idx = 0;
    for (int dt : kDts)
        for (int single = 0; single < 2; ++single) {
            for (int64_t numel : {int64_t(64), int64_t(4096) * 4096, int64_t(4096) * 4096 + 8, int64_t(4096) * 4096 + 4})
                for (int bs : {64, 128, 4096}) bnb_case(7, idx++, dt, numel, bs, 256, single);
            bnb_case(7, idx++, dt, 4096 * 4096, 64, 256, single, 8);  // the output off 16-byte alignment
            for (int64_t nbytes : {P29 - 4, P29, 25 * (P29 / 2) + 1024}) bnb_case(7, idx++, dt, 2 * nbytes, 64, 256, single);
            bnb_case(7, idx++, dt, 2 * (25 * (P29 / 2) + 1024), 4096, 16, single);
        }
    // ---- group 8: every error return of every entry, once ----
    idx = 0;
    auto emit = print_launch;
    const uint8_t* p = pk(0, 0);
    void* o = ob(0, 0);
    const nf4_launch_cfg d = kDefaultCfg;
    auto ref_err = [&](const uint8_t* pp, int64_t plen, const uint8_t* a1, int64_t nb, const float* a2, int64_t n2,
                       void* oo, int dt, int64_t m, int64_t n) {
        open_case(8, idx++, 0, dt, {m, n, plen, nb, n2, pp != nullptr, a1 != nullptr, a2 != nullptr, oo != nullptr}, {});
        close_case(plan_ref(pp, plen, a1, nb, a2, n2, oo, dt, m, n, d, 0, emit));
    };
    ref_err(p, 2048, kA1, 64, kA2, 64, o, 7, 64, 64);            // dtype
    ref_err(p, 2048, kA1, 64, kA2, 64, o, NF4DQ_F16, -1, 64);    // m < 0
    ref_err(p, 2048, kA1, 64, kA2, 64, o, NF4DQ_F16, 64, -1);    // n < 0
    ref_err(p, -1, kA1, 64, kA2, 64, o, NF4DQ_F16, 64, 64);      // packed_len < 0
    ref_err(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, NF4DQ_F16, 0, 64);  // m == 0: ok before any pointer
    ref_err(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, NF4DQ_F16, 64, 0);  // n == 0
    ref_err(nullptr, 2048, kA1, 64, kA2, 64, o, NF4DQ_F16, 64, 64);          // packed
    ref_err(p, 2048, kA1, 64, kA2, 64, nullptr, NF4DQ_F16, 64, 64);          // out
    ref_err(p, 2049, kA1, 64, kA2, 64, o, NF4DQ_F16, 64, 64);    // packed_len % m
    ref_err(p, 1984, kA1, 64, kA2, 64, o, NF4DQ_F16, 64, 64);    // rows shorter than ceil(n / 2)
    ref_err(p, 2048, nullptr, 64, kA2, 64, o, NF4DQ_F16, 64, 64);
    ref_err(p, 2048, kA1, 64, nullptr, 64, o, NF4DQ_F16, 64, 64);
    ref_err(p, 2048, kA1, 0, kA2, 64, o, NF4DQ_F16, 64, 64);
    ref_err(p, 2048, kA1, 64, kA2, 0, o, NF4DQ_F16, 64, 64);
    const nf4_launch_cfg bad[] = {{8, 0, 1, 0}, {4, 0, 0, 0}, {4, -1, 1, 0}, {4, 0, 1, 4},
                                  {4, 0, 1, NF4DQ_CFG_ROWS | NF4DQ_CFG_CHUNKS}};
    for (const nf4_launch_cfg& c : bad) {
        nf4_launch_cfg got;
        open_case(8, idx++, 1, NF4DQ_F16, {c.tile_dwords, c.blocks_per_cu, c.nontemporal, c.flags}, {});
        close_case(check_cfg(&c, got));
    }
    auto single_err = [&](const float* a, int64_t alen, int64_t m, int64_t n) {
        open_case(8, idx++, 2, NF4DQ_F16, {m, n, alen, a != nullptr}, {});
        close_case(plan_single(p, m * (n / 2), a, alen, o, NF4DQ_F16, m, n, emit));
    };
    single_err(kA2, 64, -1, 64);      // (check_common first)
    single_err(nullptr, 64, 0, 64);   // m == 0
    single_err(nullptr, 64, 64, 64);  // absmax
    single_err(kA2, -1, 64, 64);
    single_err(kA2, 65, 64, 64);      // absmax_len % m
    single_err(kA2, 64, 64, 128);     // fewer than blocks per row
    auto batched_err = [&](const nf4_matrix_desc* ds, int count, int dt) {
        open_case(8, idx++, 3, dt, {count, ds != nullptr}, {});
        close_case(plan_ref_batched(ds, count, dt, emit));
    };
    nf4_matrix_desc ds[2] = {{p, 2048, kA1, 64, kA2, 64, o, 64, 64}, {pk(1, 0), 2048, kA1, 64, kA2, 64, ob(1, 0), 64, 64}};
    batched_err(ds, -1, NF4DQ_F16);
    batched_err(nullptr, 1, NF4DQ_F16);
    batched_err(nullptr, 0, NF4DQ_F16);  // count == 0
    batched_err(ds, 2, 9);
    ds[1].packed_len = 2049;             // the second matrix is wrong: nothing is launched
    batched_err(ds, 2, NF4DQ_F16);
    ds[1].packed_len = 2048;
    ds[1].nb = 0;
    batched_err(ds, 2, NF4DQ_F16);
    ds[1].nb = 64;
    ds[0].m = 0;                         // an empty matrix is skipped
    batched_err(ds, 2, NF4DQ_F16);
    auto bnb_err = [&](const uint8_t* pp, const uint8_t* a1, int64_t nb, const float* c2, const float* a2, int64_t n2,
                       void* oo, int dt, int64_t numel, int bs, int bs2, bool single) {
        open_case(8, idx++, single ? 5 : 4, dt,
                  {numel, bs, bs2, nb, n2, pp != nullptr, a1 != nullptr, c2 != nullptr, a2 != nullptr, oo != nullptr}, {});
        close_case(plan_bnb(pp, a1, nb, c2, a2, n2, 0.0f, oo, dt, numel, bs, bs2, single, emit));
    };
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, 5, 4096, 64, 256, false);
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, -8, 64, 256, false);
    bnb_err(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, NF4DQ_BF16, 0, 64, 256, false);  // numel == 0
    bnb_err(nullptr, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 64, 256, false);
    bnb_err(p, kA1, 64, kCode2, kA2, 1, nullptr, NF4DQ_BF16, 4096, 64, 256, false);
    bnb_err(p, kA1, 64, kCode2, nullptr, 1, o, NF4DQ_BF16, 4096, 64, 256, false);
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 32, 256, false);   // blocksize < 64
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 96, 256, false);   // not a power of two
    bnb_err(p, kA1, 63, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 64, 256, false);   // nb short
    bnb_err(p, nullptr, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 64, 256, false);
    bnb_err(p, kA1, 64, nullptr, kA2, 1, o, NF4DQ_BF16, 4096, 64, 256, false);
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 64, 0, false);
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 64, 48, false);
    bnb_err(p, kA1, 64, kCode2, kA2, 1, o, NF4DQ_BF16, 4096, 64, 16, false);    // n2 short
    bnb_err(p, nullptr, 64, nullptr, nullptr, 0, o, NF4DQ_BF16, 4096, 64, 1, true);
    bnb_err(p, nullptr, 63, nullptr, kA2, 0, o, NF4DQ_BF16, 4096, 64, 1, true);
    return 0;
}
