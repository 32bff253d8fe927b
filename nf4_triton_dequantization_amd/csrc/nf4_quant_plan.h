// nf4_quant_plan.h -- what the device quantizer (nf4_quant.hip) and its host twin
// (nf4_dequant_cpu.cpp) must agree on to give the same bits: the NF4 decision
// thresholds, the accepted block sizes, and the fixed order of the fp64 absmax sum.
#pragma once

#include <stdint.h>

namespace nf4q {

// Second-level block size (bitsandbytes' only value) = threads of a statistics workgroup.
constexpr int kBlock2 = 256;

// blocksize: a power of two in 64..4096 (bitsandbytes' 4-bit block sizes).
inline bool valid_blocksize(int32_t bs) { return bs >= 64 && bs <= 4096 && (bs & (bs - 1)) == 0; }

// The absmax sum, in fp64, in an order that depends on nblk alone:
//   part p     = sum_ordered(absmax[p*chunk .. min(nblk, (p+1)*chunk)))
//   total      = sum_ordered(part[0 .. parts))
//   sum_ordered(v[0..n)): slot t (0..255) adds v[t], v[t+256], ... in index order
//                starting from 0.0, then slots fold pairwise: for s = 128, 64, .. 1:
//                slot[t] += slot[t+s] (t < s); the result is slot[0].
// chunk: a multiple of 256, at least 4096, large enough for at most kMaxParts parts.
constexpr int kMaxParts = 1024;

struct SumPlan {
    int64_t chunk;
    int32_t parts;
};

inline SumPlan sum_plan(int64_t nblk) {
    int64_t chunk = (nblk + kMaxParts - 1) / kMaxParts;
    chunk = (chunk + 255) / 256 * 256;
    if (chunk < 4096) chunk = 4096;
    SumPlan p;
    p.chunk = chunk;
    p.parts = (int32_t)((nblk + chunk - 1) / chunk);
    return p;
}

// Workspace of the nested device call: fp32 absmax[nblk] (256-byte granules), then
// the fp64 partial sums.
inline int64_t ws_absmax_bytes(int64_t nblk) { return (nblk * 4 + 255) / 256 * 256; }
inline int64_t ws_bytes(int64_t nblk) { return ws_absmax_bytes(nblk) + (int64_t)kMaxParts * 8; }

}  // namespace nf4q
