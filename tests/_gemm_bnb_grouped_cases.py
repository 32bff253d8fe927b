"""Inputs shared by the grouped bitsandbytes-semantics GEMM suites (test_gpu_gemm_bnb_grouped.py;
test_gemm_bnb_grouped_cases_cpu.py checks this module itself on the host).

A grouped launch (nf4_gemm_bnb_grouped) gives every weight its own code2 table, offset,
blocksize2 and flat statistics stream.  ``nested_group`` builds three nested weights that
differ in everything such a kernel could wrongly share:

    weight 0   drawn_weight_bnb        blocksize2 256   offset 0.0123   code2 = the dynamic map
    weight 1   sensitive_weight_bnb    blocksize2 16    offset 0.05     code2 = the dynamic map
    weight 2   drawn_weight_bnb        blocksize2 4     offset None     code2 = the map reversed

(None is a null offset pointer, = 0; the reversed map holds the same 256 finite values in
another order.)  Every statistics array has exactly the needed length.  ``misread_bits``
restates one weight's dequantization with another weight's code2, offset or blocksize2, or with
its flat block index starting at the launch-wide row instead of 0; the CPU test proves that each
such restatement changes the 16-bit weights in every 16-row strip, so an exact identity walk
tells the bugs apart.
"""
from __future__ import annotations

import functools

import numpy as np

from _gemm_bnb_cases import bnb_scale, code2_np, drawn_weight_bnb, sensitive_weight_bnb, single_weight_bnb
from _gemm_cases import weight_bits

OFFSETS = (0.0123, 0.05, None)
BLOCKSIZE2S = (256, 16, 4)
SMALL_NS = (64, 192, 64)


@functools.lru_cache(maxsize=None)
def nested_group(Ns, K, dt, seed=0):
    """((packed, a1, code2, a2, offset or None, blocksize2), ...) for three weights of Ns rows;
    cached and read-only."""
    assert len(Ns) == 3
    w0 = drawn_weight_bnb(Ns[0], K, seed=seed + 11, blocksize2=BLOCKSIZE2S[0])
    w1 = sensitive_weight_bnb(Ns[1], K, dt, seed=seed + 1)[:5]
    w2 = drawn_weight_bnb(Ns[2], K, seed=seed + 13, blocksize2=BLOCKSIZE2S[2])
    out = []
    for i, w in enumerate((w0, w1, w2)):
        packed, a1, code2, a2 = (np.ascontiguousarray(v).copy() for v in w[:4])
        if i == 2:
            code2 = np.ascontiguousarray(code2_np()[::-1]).copy()
        nblk = Ns[i] * K // 64
        assert a1.size == nblk and a2.size == -(-nblk // BLOCKSIZE2S[i]) and code2.size == 256
        for a in (packed, a1, code2, a2):
            a.setflags(write=False)
        out.append((packed, a1, code2, a2, OFFSETS[i], BLOCKSIZE2S[i]))
    return tuple(out)


def offset_value(off):
    return 0.0 if off is None else float(off)


def codes_of(packed, nblk):
    nib = np.empty(packed.size * 2, np.uint8)
    nib[0::2], nib[1::2] = packed >> 4, packed & 0xF
    return nib.reshape(nblk, 64).astype(np.int64)


def misread_bits(w, dt, *, code2=None, offset="own", blocksize2=None, first_block=0):
    """The 16-bit weights [nblk, 64] of nested weight `w` when its scale is made with another
    code2 table, offset or blocksize2, or its 64-blocks are numbered from `first_block` on.
    A statistics index beyond its array reads 0, what a range-checked buffer load returns
    (absmax byte 0, absmax2 0.0).  With no override: the oracle's formula."""
    packed, a1, c2, a2, off, bs2 = w
    nblk = a1.size
    c2 = c2 if code2 is None else code2
    off = off if offset == "own" else offset
    bs2 = bs2 if blocksize2 is None else blocksize2
    f = (np.arange(nblk, dtype=np.int64) + first_block)
    g = f // bs2
    q = np.where(f < nblk, a1[np.minimum(f, nblk - 1)], 0).astype(np.uint8)
    s2 = np.where(g < a2.size, a2[np.minimum(g, a2.size - 1)], np.float32(0.0)).astype(np.float32)
    s = bnb_scale(c2[q], s2, offset_value(off))
    return weight_bits(s[:, None], codes_of(packed, nblk), dt)


@functools.lru_cache(maxsize=None)
def single_group(Ns, K, seed=0):
    """((packed, absmax fp32), ...): a group with fp32 statistics (compress_statistics=False)."""
    return tuple(single_weight_bnb(N, K, seed=seed + 7 * i + N) for i, N in enumerate(Ns))
