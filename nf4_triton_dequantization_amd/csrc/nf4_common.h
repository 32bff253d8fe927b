// nf4_common.h -- device helpers shared by the dequant (nf4_dequant.hip) and
// fused dequant-GEMM (nf4_gemm.hip) kernels of libnf4dq.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nf4_dequant.h"
#include "nf4_fastdiv.h"

namespace nf4dq {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// FastDiv (nf4_fastdiv.h) on the device: q = (umulhi(n, mul) + n) >> shift.
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    return (__umulhi(n, f.mul) + n) >> f.shift;
}
__device__ __forceinline__ uint32_t fmodu(uint32_t n, const FastDiv& f) {
    return n - fdiv(n, f) * f.d;
}

// Keep an fp32 product opaque to the backend: without this, hipcc folds
// fptrunc(fmul) into v_fma_mix*_f16(a, b, +0), which rounds once instead of
// twice (fp32 product, then fp16 -- the reference's order) and turns -0 into +0.
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// The pair as one opaque 64-bit value (non-volatile: the scheduler may still
// move it; the products stay one v_pk_mul_f32).
__device__ __forceinline__ f32x2 opaque2(f32x2 v) {
    asm("" : "+v"(v));
    return v;
}

template <int DT>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    f32x2 v = {lo, hi};
    if constexpr (DT == NF4DQ_F16) v = opaque2(v);
    if constexpr (DT == NF4DQ_BF16) {
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
    } else {
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
    }
}

// The 16 NF4 code points: fp32 bit patterns of kernel_optimized.py:234-239.
constexpr uint32_t kNf4Bits[16] = {0xbf800000u, 0xbf3239b1u, 0xbf066b30u, 0xbeca32a0u, 0xbe91a24du, 0xbe3d353fu,
                                   0xbdba7871u, 0x00000000u, 0x3da2faffu, 0x3e24cae3u, 0x3e7c04ddu, 0x3ead033au,
                                   0x3ee1a4b8u, 0x3f1007abu, 0x3f3913b3u, 0x3f800000u};

// The code table into LDS from immediates (no global load on the kernel's
// critical path): thread 0 writes four 16-byte rows.
__device__ __forceinline__ void write_lut(float* lut) {
    if (threadIdx.x == 0) {
        u32x4* l4 = reinterpret_cast<u32x4*>(lut);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            l4[r] = u32x4{kNf4Bits[4 * r], kNf4Bits[4 * r + 1], kNf4Bits[4 * r + 2], kNf4Bits[4 * r + 3]};
    }
}

// Code point i: a constant for constant i, a select chain otherwise.
__device__ __forceinline__ float nf4_code(uint32_t i) {
    uint32_t v = kNf4Bits[0];
#pragma unroll
    for (uint32_t j = 1; j < 16; ++j) v = i == j ? kNf4Bits[j] : v;
    return __uint_as_float(v);
}

// Scalar store of one output element (the per-byte / per-element kernels).
template <int DT>
__device__ __forceinline__ void store1(void* out, int64_t i, float x) {
    if constexpr (DT == NF4DQ_BF16) {
        reinterpret_cast<__bf16*>(out)[i] = (__bf16)x;
    } else if constexpr (DT == NF4DQ_F16) {
        reinterpret_cast<_Float16*>(out)[i] = (_Float16)opaque(x);
    } else {
        reinterpret_cast<float*>(out)[i] = x;
    }
}

// Per-block table decode (16-bit outputs; the flat dequant kernel and the embedding gather).
// The 8 lanes that share a 64-element block round its 16 possible outputs into a 32-byte
// table at LDS byte `tb` (a multiple of 256, so byte 0 of tb is zero): lane k of the group
// writes the outputs of codes 2k and 2k+1 as dword k.  An output is then the 16-bit entry at
// tb + 2 * code, and 2 * code is a byte of (w >> 3) & 0x1E1E1E1E (high nibbles) or
// (w << 1) & 0x1E1E1E1E (low nibbles): v_perm_b32 moves that byte into tb's byte 0, one
// instruction per address.  A wave's LDS accesses complete in order, so the group needs no
// barrier between its writes and its reads.
typedef uint16_t __attribute__((may_alias)) u16_alias;  // table entries are written as dwords
typedef uint32_t __attribute__((may_alias)) u32_alias;
typedef uint32_t u32x4_alias __attribute__((ext_vector_type(4), may_alias));

template <int DT>
__device__ __forceinline__ void block_table_write(char* tbl, uint32_t tb, uint32_t k, f32x2 c01, float s) {
    *reinterpret_cast<u32_alias*>(tbl + tb + 4u * k) = pack2<DT>(c01.x * s, c01.y * s);
}

// The 8 outputs of packed dword w (high nibble -> even element), two per output dword.
__device__ __forceinline__ u32x4 block_table_decode(const char* tbl, uint32_t tb, uint32_t w) {
    const uint32_t hb = (w >> 3) & 0x1E1E1E1Eu;
    const uint32_t lb = (w << 1) & 0x1E1E1E1Eu;
    uint32_t o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t ah = __builtin_amdgcn_perm(hb, tb, 0x03020104u + b);
        const uint32_t al = __builtin_amdgcn_perm(lb, tb, 0x03020104u + b);
        const uint32_t vh = *reinterpret_cast<const u16_alias*>(tbl + ah);
        const uint32_t vl = *reinterpret_cast<const u16_alias*>(tbl + al);
        o[b] = vh | (vl << 16);
    }
    return u32x4{o[0], o[1], o[2], o[3]};
}

// Buffer-resource flags word (raw buffer, dword format) for gfx950.
constexpr int kRsrcFlags = 0x00020000;

}  // namespace nf4dq
