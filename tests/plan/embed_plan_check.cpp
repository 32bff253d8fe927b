// embed_plan_check.cpp -- the host plan of the NF4 embedding gather (csrc/nf4_embed_plan.h)
// and the host entries (csrc/nf4_dequant_cpu.cpp, compiled into this program), checked
// without a GPU.  Built stand-alone under AddressSanitizer + UBSan by
// tests/test_embed_plan_cpu.py; prints one JSON line per case, which the test judges.
//   {"k":"plan", ...}  the plan of a valid call: form, grid, block, element range, constants
//   {"k":"err",  ...}  a call the plan must refuse (or accept with nothing launched)
//   {"k":"cpu",  ...}  the _cpu entries with ids outside [0, rows) among valid ones: tables
//                      are exact-size heap blocks, so a missing guard is a sanitizer report
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/nf4_dequant.h"
#include "../../nf4_triton_dequantization_amd/csrc/nf4_embed_plan.h"

using namespace nf4dq;

namespace {

// Non-null, aligned, never dereferenced by the plan.
void* const kFake = reinterpret_cast<void*>(uintptr_t(0x10000));

EmbedCall call(int64_t count, int64_t rows, int64_t dim, int32_t out_dt, int32_t ids_dt, int32_t bs, int32_t bs2,
               bool single) {
    EmbedCall c{};
    c.ids = kFake;
    c.ids_dtype = ids_dt;
    c.count = count;
    c.packed = reinterpret_cast<const uint8_t*>(kFake);
    c.a1 = single ? nullptr : reinterpret_cast<const uint8_t*>(kFake);
    c.code2 = single ? nullptr : reinterpret_cast<const float*>(kFake);
    c.a2 = reinterpret_cast<const float*>(kFake);
    c.offset = nullptr;
    c.blocksize = bs;
    c.blocksize2 = single ? 0 : bs2;
    c.out = kFake;
    c.out_dtype = out_dt;
    c.rows = rows;
    c.dim = dim;
    c.single = single;
    const int64_t numel = rows > 0 && dim > 0 && rows <= kEmbedMaxTable / dim ? rows * dim : 0;
    const int64_t nblk = bs > 0 ? (numel + bs - 1) / bs : 0;
    c.nb = nblk;
    c.n2 = single || bs2 <= 0 ? 0 : (nblk + bs2 - 1) / bs2;
    return c;
}

void print_plan(const char* tag, const EmbedCall& c) {
    const EmbedPlan P = plan_embed(c);
    // the fast division the aligned kernel makes, checked at the ends of its range
    int fd_ok = 1;
    if (P.rc == 0 && P.launches && P.form == kEmbedAligned) {
        const FastDiv f = P.args.bpr;
        const uint32_t probes[] = {0u, 1u, f.d - 1u, f.d, f.d + 1u, P.args.blocks - 1u, P.args.blocks / 2u};
        for (uint32_t n : probes) {
            if (n >= P.args.blocks && n != 0u) continue;
            const uint32_t q = (uint32_t)((((uint64_t)n * f.mul) >> 32) + n) >> f.shift;
            if (q != n / f.d) fd_ok = 0;
        }
    }
    printf("{\"k\":\"plan\",\"tag\":\"%s\",\"count\":%lld,\"rows\":%lld,\"dim\":%lld,\"dt\":%d,\"single\":%d,"
           "\"rc\":%d,\"launches\":%d,\"form\":%d,\"grid\":%u,\"block\":%u,\"e0\":%lld,\"e1\":%lld,"
           "\"elems\":%u,\"blocks\":%u,\"bpr\":%u,\"bsh\":%u,\"bsh2\":%u,\"steps\":%d,\"wg_blocks\":%d,\"fd_ok\":%d}\n",
           tag, (long long)c.count, (long long)c.rows, (long long)c.dim, c.out_dtype, c.single ? 1 : 0, P.rc,
           P.launches, P.form, P.grid, P.block, (long long)P.elem_begin, (long long)P.elem_end, P.args.elems,
           P.args.blocks, P.args.bpr.d, P.args.blk_shift, P.args.blk2_shift, P.steps, (kEmbedWg / 8) * P.steps, fd_ok);
}

void print_err(const char* name, const EmbedCall& c) {
    const EmbedPlan P = plan_embed(c);
    printf("{\"k\":\"err\",\"name\":\"%s\",\"rc\":%d,\"launches\":%d}\n", name, P.rc, P.launches);
}

uint32_t lcg(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

// The _cpu entries with bad ids among valid ones, against the same call with the bad ids
// replaced by row 0: bad rows must be zero bits, the others equal.
void cpu_case(int64_t rows, int64_t dim, int32_t bs, int32_t bs2, int32_t out_dt, bool single, bool ids64) {
    const int64_t numel = rows * dim;
    const int64_t nblk = (numel + bs - 1) / bs;
    const int64_t n2 = single ? 0 : (nblk + bs2 - 1) / bs2;
    uint32_t seed = (uint32_t)(rows * 131 + dim * 7 + bs + out_dt);
    std::vector<uint8_t> packed((size_t)((numel + 1) / 2));
    for (auto& b : packed) b = (uint8_t)lcg(seed);
    std::vector<uint8_t> a1((size_t)(single ? 0 : nblk));
    for (auto& b : a1) b = (uint8_t)lcg(seed);
    std::vector<float> code2(256);
    for (int i = 0; i < 256; ++i) code2[(size_t)i] = (float)(i - 128) / 128.0f;
    std::vector<float> a2((size_t)(single ? nblk : n2));
    for (auto& v : a2) v = 0.01f + (float)(lcg(seed) & 1023u) / 1024.0f;
    const float offset = 0.0371f;

    std::vector<int64_t> want64 = {0, rows - 1, 1};
    std::vector<int64_t> bad64 = {-1, rows, rows + 1};
    if (ids64) {
        bad64.push_back((int64_t(1) << 31) + 1);
        bad64.push_back((int64_t(1) << 32) + 1);  // its low half names a valid row
        bad64.push_back(-(int64_t(1) << 40));
        bad64.push_back(INT64_MIN);
    } else {
        bad64.push_back(INT32_MIN);
        bad64.push_back(INT32_MAX);
    }
    std::vector<int64_t> mixed, clean;
    std::vector<int> is_bad;
    for (size_t i = 0; i < bad64.size(); ++i) {
        mixed.push_back(want64[i % want64.size()]);
        clean.push_back(mixed.back());
        is_bad.push_back(0);
        mixed.push_back(bad64[i]);
        clean.push_back(0);
        is_bad.push_back(1);
    }
    mixed.push_back(rows / 2);
    clean.push_back(rows / 2);
    is_bad.push_back(0);
    const int64_t count = (int64_t)mixed.size();
    std::vector<int32_t> m32(mixed.begin(), mixed.end()), c32(clean.begin(), clean.end());
    const void* pm = ids64 ? (const void*)mixed.data() : (const void*)m32.data();
    const void* pc = ids64 ? (const void*)clean.data() : (const void*)c32.data();
    const int32_t idt = ids64 ? NF4DQ_IDS_I64 : NF4DQ_IDS_I32;
    const size_t esize = out_dt == NF4DQ_F32 ? 4 : 2;
    std::vector<uint8_t> om((size_t)(count * dim) * esize, 0xCD), oc((size_t)(count * dim) * esize, 0xCD);
    int rc1, rc2;
    if (single) {
        rc1 = nf4_embedding_bnb_single_cpu(pm, idt, count, packed.data(), a2.data(), nblk, bs, om.data(), out_dt, rows,
                                           dim, 2);
        rc2 = nf4_embedding_bnb_single_cpu(pc, idt, count, packed.data(), a2.data(), nblk, bs, oc.data(), out_dt, rows,
                                           dim, 1);
    } else {
        rc1 = nf4_embedding_bnb_cpu(pm, idt, count, packed.data(), a1.data(), nblk, code2.data(), a2.data(), n2,
                                    &offset, bs, bs2, om.data(), out_dt, rows, dim, 2);
        rc2 = nf4_embedding_bnb_cpu(pc, idt, count, packed.data(), a1.data(), nblk, code2.data(), a2.data(), n2,
                                    &offset, bs, bs2, oc.data(), out_dt, rows, dim, 1);
    }
    int zero_ok = 1, same_ok = 1, nonzero_valid = 0;
    const size_t rb = (size_t)dim * esize;
    for (int64_t i = 0; i < count; ++i) {
        const uint8_t* r = om.data() + (size_t)i * rb;
        if (is_bad[(size_t)i]) {
            for (size_t j = 0; j < rb; ++j) zero_ok &= r[j] == 0;
        } else {
            same_ok &= memcmp(r, oc.data() + (size_t)i * rb, rb) == 0;
            for (size_t j = 0; j < rb; ++j) nonzero_valid |= r[j] != 0;
        }
    }
    printf("{\"k\":\"cpu\",\"rows\":%lld,\"dim\":%lld,\"bs\":%d,\"dt\":%d,\"single\":%d,\"ids64\":%d,\"rc\":[%d,%d],"
           "\"bad\":%d,\"zero_ok\":%d,\"same_ok\":%d,\"nonzero_valid\":%d}\n",
           (long long)rows, (long long)dim, bs, out_dt, single ? 1 : 0, ids64 ? 1 : 0, rc1, rc2, (int)bad64.size(),
           zero_ok, same_ok, nonzero_valid);
}

}  // namespace

int main() {
    // ---- valid calls: form, tiling, grid -------------------------------------------------
    const int64_t dims[] = {1, 7, 63, 64, 77, 100, 128, 192, 1024, 4096, 4100, 8192};
    const int64_t counts[] = {1, 2, 8, 31, 32, 33, 64, 512, 8192};
    for (int64_t dim : dims)
        for (int64_t count : counts)
            for (int dt = 0; dt < 3; ++dt) {
                print_plan("grid", call(count, 1000, dim, dt, NF4DQ_IDS_I64, 64, 256, false));
                print_plan("grid", call(count, 1000, dim, dt, NF4DQ_IDS_I32, 128, 0, true));
            }
    print_plan("llama", call(32, 128256, 4096, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    print_plan("blocksizes", call(5, 64, 4096, NF4DQ_BF16, NF4DQ_IDS_I64, 4096, 4, false));
    print_plan("rows0", call(3, 0, 64, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    {  // pointers off the aligned form's alignment take the general form
        EmbedCall c = call(4, 10, 128, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false);
        c.out = reinterpret_cast<void*>(uintptr_t(0x10008));
        print_plan("misaligned_out", c);
        c = call(4, 10, 128, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false);
        c.packed = reinterpret_cast<const uint8_t*>(uintptr_t(0x10002));
        print_plan("misaligned_packed", c);
    }
    // ---- the too-large rule around 2^31 and 2^32 ------------------------------------------
    print_plan("large_ok", call((int64_t(1) << 31) / 4096 - 1, 1000, 4096, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    print_plan("large_ok", call((int64_t(1) << 31) - 1, 1000, 1, NF4DQ_F32, NF4DQ_IDS_I64, 64, 256, false));
    print_plan("large_ok", call(1, 4, (int64_t(1) << 31) - 64, NF4DQ_F32, NF4DQ_IDS_I64, 64, 256, false));
    print_err("too_large_2p31", call((int64_t(1) << 31) / 4096, 1000, 4096, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    print_err("too_large_2p31_dim1", call(int64_t(1) << 31, 1000, 1, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    print_err("too_large_2p32", call((int64_t(1) << 32) / 4096, 1000, 4096, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    print_err("too_large_2p32_plus", call((int64_t(1) << 32) / 64 + 1, 1000, 64, NF4DQ_BF16, NF4DQ_IDS_I32, 64, 256, true));
    print_err("too_large_count_max", call(INT64_MAX, 1000, 4096, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    print_err("too_large_table", call(1, int64_t(1) << 50, int64_t(1) << 13, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false));
    // ---- the error rules -------------------------------------------------------------------
    const EmbedCall ok = call(4, 10, 128, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 256, false);
    const EmbedCall oks = call(4, 10, 128, NF4DQ_BF16, NF4DQ_IDS_I64, 64, 0, true);
    print_err("ok", ok);
    print_err("ok_single", oks);
    EmbedCall c;
#define CASE(name_, base_, stmt_) \
    c = base_;                    \
    stmt_;                        \
    print_err(name_, c)
    CASE("arg_null_ids", ok, c.ids = nullptr);
    CASE("arg_null_packed", ok, c.packed = nullptr);
    CASE("arg_null_out", ok, c.out = nullptr);
    CASE("arg_null_absmax_q", ok, c.a1 = nullptr);
    CASE("arg_null_code2", ok, c.code2 = nullptr);
    CASE("arg_null_absmax2", ok, c.a2 = nullptr);
    CASE("arg_null_absmax_single", oks, c.a2 = nullptr);
    CASE("arg_ids_dtype", ok, c.ids_dtype = 2);
    CASE("arg_out_dtype", ok, c.out_dtype = 3);
    CASE("arg_out_dtype_neg", ok, c.out_dtype = -1);
    CASE("arg_bs_32", ok, c.blocksize = 32);
    CASE("arg_bs_96", ok, c.blocksize = 96);
    CASE("arg_bs_8192", ok, c.blocksize = 8192);
    CASE("arg_bs_0", ok, c.blocksize = 0);
    CASE("arg_bs2_0", ok, c.blocksize2 = 0);
    CASE("arg_bs2_3", ok, c.blocksize2 = 3);
    CASE("arg_bs2_2", ok, c.blocksize2 = 2);
    CASE("arg_bs_32_single", oks, c.blocksize = 32);
    CASE("shape_count_neg", ok, c.count = -1);
    CASE("shape_rows_neg", ok, c.rows = -1);
    CASE("shape_dim_neg", ok, c.dim = -1);
    CASE("shape_dim_0", ok, c.dim = 0);
    CASE("shape_nb_short", ok, c.nb -= 1);
    CASE("shape_n2_short", ok, c.n2 -= 1);
    CASE("shape_nabs_short", oks, c.nb -= 1);
    CASE("shape_nb_neg", ok, c.nb = -1);
    CASE("ok_count_0", ok, c.count = 0);
    CASE("ok_count_0_nulls", ok, (c.count = 0, c.ids = nullptr, c.packed = nullptr, c.out = nullptr, c.a1 = nullptr,
                                  c.a2 = nullptr, c.code2 = nullptr));
    CASE("ok_count_0_dim_0", ok, (c.count = 0, c.dim = 0));
    CASE("ok_null_offset", ok, c.offset = nullptr);
    CASE("ok_single_ignores_bs2", oks, c.blocksize2 = 3);
#undef CASE
    // ---- the host entries with ids outside [0, rows) -----------------------------------------
    for (int dt = 0; dt < 3; ++dt)
        for (int ids64 = 0; ids64 < 2; ++ids64) {
            cpu_case(7, 64, 64, 256, dt, false, ids64 != 0);
            cpu_case(11, 77, 128, 4, dt, false, ids64 != 0);
            cpu_case(9, 128, 256, 16, dt, true, ids64 != 0);
        }
    return 0;
}
