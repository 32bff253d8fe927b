"""The combine of nf4_gemm_bnb_moe_down / nf4_moe_down_bnb on the host, in numpy fp32 on bit
patterns -- the chain the entry documents, nothing else:

    y[t] = rn16( sum_j rn16( d[t k + j] * rn16(rw[t k + j]) ) )

with d the 16-bit products of the pairs (+0 where the id is outside 0..E-1), the product in fp32
(exact for two 16-bit values) rounded once, the sum in fp32 from +0.0 in the order j = 0 .. k-1,
rounded once.  rn16 is round-to-nearest-even to bf16 / fp16; a NaN stays a quiet NaN with its sign
and leading payload bits, as the hardware conversion keeps them."""
import numpy as np


def widen(bits, dt):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dt == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def rn16(f, dt):
    """fp32 array -> 16-bit patterns, round to nearest even."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if dt == "f16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), ((u >> 16) | np.uint32(0x40)).astype(np.uint16), r)


def chain(d_bits, ids, E, rw, k, dt):
    """d_bits [P, N] uint16, ids [P], rw [P] (np.float32 values, or np.uint16 patterns of dt)
    -> y bits [P / k, N]."""
    d_bits, ids = np.asarray(d_bits), np.asarray(ids).reshape(-1)
    P, N = d_bits.shape
    valid = (ids >= 0) & (ids < E)
    d = widen(np.where(valid[:, None], d_bits, np.uint16(0)), dt).reshape(P // k, k, N)
    rw = np.asarray(rw).reshape(-1)
    w = widen(rw if rw.dtype == np.uint16 else rn16(rw, dt), dt).reshape(P // k, k, 1)
    acc = np.zeros((P // k, N), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            acc = acc + widen(rn16(d[:, j] * w[:, j], dt), dt)
    return rn16(acc, dt)
