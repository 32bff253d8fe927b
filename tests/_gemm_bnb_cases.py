"""Inputs shared by the bitsandbytes-semantics fused-GEMM suites (test_gpu_gemm_bnb.py,
test_gpu_redzones_bnb.py; test_gemm_bnb_cases_cpu.py checks this module itself on the host).

The bnb mode multiplies x by the weights nf4_dequant_bnb would write,

    s = fp32(fp32(code2[q] * a2) + offset)          two roundings
    w = RNE16(fp32(NF4[c] * s)),

and a float64 product inside the GEMM tolerance cannot tell that from a weight one 16-bit
ulp off.  ``sensitive_weight_bnb`` builds a real nested weight (blocksize 64, blocksize2 16,
one fixed nonzero offset, positive absmax2, the dynamic map as code2) in which one 64-block
of every nested group carries a found triple (q, a2, c) at which a near-miss restatement
gives another 16-bit value:

    fma_scale         s = fp32(code2[q] * a2 + offset)   one rounding (a fused multiply-add)
    single_rounding   RNE16(NF4[c] * s) with the product exact (one rounding, not two)

The search is directed as in _gemm_cases.sensitive_triples: the last product must land next
to a 16-bit rounding boundary, so a2 is solved for from a drawn boundary and its fp32
neighbours are tried.  Everything is judged by evaluating the oracle's formula and the
restatements; the aiming only makes hits frequent.  (float64 holds code2[q] * a2 exactly;
adding the offset may round, so test_gemm_bnb_cases_cpu.py re-judges the fused scale with
rational arithmetic.)
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

import nf4_oracle as O
from _gemm_cases import _CODES, _boundaries, _neighbours, single_rounding_bits, weight_bits

KINDS_BNB = ("fma_scale", "single_rounding")
OFFSET = np.float32(0.0371)  # the fixed offset of the sensitive weight
BLOCKSIZE2 = 16


@functools.lru_cache(maxsize=None)
def code2_np():
    """The 256-entry dynamic map (the nested code book the quantizer uses), fp32."""
    from nf4_triton_dequantization_amd.bnb_layout import dynamic_map

    return dynamic_map(signed=True).numpy().astype(np.float32)


def bnb_scale(c2, a2, off):
    """fp32(fp32(code2[q] * a2) + offset) (oracle/nf4_oracle.py::dequant_bnb_np)."""
    p = (np.asarray(c2, np.float32) * np.asarray(a2, np.float32)).astype(np.float32)
    return (p + np.float32(off)).astype(np.float32)


def fma_scale(c2, a2, off):
    """fp32(code2[q] * a2 + offset) with one rounding, up to float64's own (the product of
    two fp32 values is exact in float64; the sum may round once more)."""
    return (np.asarray(c2, np.float64) * np.asarray(a2, np.float64) + np.float64(off)).astype(np.float32)


def f32_rne(fr: Fraction) -> np.float32:
    """The fp32 nearest to a rational (ties to even), subnormals on their grid."""
    if fr == 0:
        return np.float32(0.0)
    a = abs(fr)
    sh = a.numerator.bit_length() - a.denominator.bit_length() - 23
    while a / Fraction(2) ** sh >= 1 << 24:
        sh += 1
    while a / Fraction(2) ** sh < 1 << 23:
        sh -= 1
    sh = max(sh, -149)
    m = a / Fraction(2) ** sh
    n = m.numerator // m.denominator
    r = m - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    v = math.ldexp(n, sh)  # exact: n <= 2^24
    return np.float32(-v if fr < 0 else v)


def fma_scale_exact(c2, a2, off):
    """fp32(code2[q] * a2 + offset) rounded once from the exact rational value."""
    c2, a2 = np.asarray(c2, np.float32), np.asarray(a2, np.float32)
    fo = Fraction(float(off))
    out = [f32_rne(Fraction(float(c)) * Fraction(float(a)) + fo) for c, a in zip(c2.ravel(), a2.ravel())]
    return np.array(out, np.float32).reshape(c2.shape)


def near_miss_bits_bnb(kind, c2, a2, off, c, dt):
    if kind == "fma_scale":
        return weight_bits(fma_scale(c2, a2, off), c, dt)
    if kind == "single_rounding":
        return single_rounding_bits(bnb_scale(c2, a2, off), c, dt)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def sensitive_triples_bnb(dt, per_kind=96, seed=1):
    """{kind: (q uint8, a2 fp32 > 0, c)} -- at least `per_kind` distinct triples per near miss
    at which that restatement's 16-bit weight differs from the oracle formula's, under OFFSET."""
    code2 = code2_np()
    rng = np.random.default_rng(seed)
    out = {k: ([], [], []) for k in KINDS_BNB}
    seen = {k: set() for k in KINDS_BNB}
    off64 = np.float64(OFFSET)
    for _ in range(400):
        if all(len(out[k][0]) >= per_kind for k in KINDS_BNB):
            break
        n = 8192
        q = rng.integers(0, 256, n).astype(np.uint8)
        c = rng.choice(_CODES, n)
        t = _boundaries(rng, n, dt)
        c2 = code2[q].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            a2c = (t / np.abs(O.NF4_LUT[c].astype(np.float64)) - off64) / c2
        # positive absmax2 of the size of real statistics; the product not dwarfed by the offset
        ok = np.isfinite(a2c) & (a2c > 2.0 ** -10) & (a2c < 2.0 ** 6) & (np.abs(c2) > 2.0 ** -10)
        q, c, a2c = q[ok], c[ok], a2c[ok]
        a2 = _neighbours(a2c.astype(np.float32), 3)
        qq = np.repeat(q[:, None], a2.shape[1], axis=1)
        cc = np.repeat(c[:, None], a2.shape[1], axis=1)
        c2q = code2[qq]
        want = weight_bits(bnb_scale(c2q, a2, OFFSET), cc, dt)
        for k in KINDS_BNB:
            hit = near_miss_bits_bnb(k, c2q, a2, OFFSET, cc, dt) != want
            for tr in zip(qq[hit].tolist(), a2[hit].tolist(), cc[hit].tolist()):
                if tr not in seen[k] and len(out[k][0]) < per_kind:
                    seen[k].add(tr)
                    for lst, v in zip(out[k], tr):
                        lst.append(v)
    for k in KINDS_BNB:
        assert len(out[k][0]) >= per_kind, (k, len(out[k][0]))
    return {k: (np.array(v[0], np.uint8), np.array(v[1], np.float32), np.array(v[2], np.int64))
            for k, v in out.items()}


def sensitive_weight_bnb(N, K, dt, seed=1):
    """(packed, a1, code2, a2, offset, kind_of_block): fresh copies of the cached arrays."""
    return tuple(a.copy() if isinstance(a, np.ndarray) else a for a in _sensitive_weight_bnb(N, K, dt, seed))


@functools.lru_cache(maxsize=None)
def _sensitive_weight_bnb(N, K, dt, seed):
    """A nested bnb weight on the flat stream: N K / 64 absmax bytes, one absmax2 per
    BLOCKSIZE2 = 16 of them (N = 128, K = 1024: 128 nested groups).  One 64-block of each
    nested group (its position rotating) takes a found triple -- its absmax byte, the group's
    absmax2 and all 64 codes -- and the other fifteen take drawn bytes and codes under that
    absmax2.  ``kind_of_block`` [N K / 64] is the index into KINDS_BNB of a block's triple, or
    -1.  Cached and read-only."""
    assert K % 64 == 0 and (N * K // 64) % BLOCKSIZE2 == 0
    tri = sensitive_triples_bnb(dt)
    rng = np.random.default_rng(2000 * seed + N + K)
    nblk = N * K // 64
    ng = nblk // BLOCKSIZE2
    a1 = rng.integers(0, 256, nblk).astype(np.uint8)
    codes = rng.integers(0, 16, (nblk, 64)).astype(np.uint8)
    a2 = np.empty(ng, np.float32)
    kind_of_block = np.full(nblk, -1, np.int8)
    for g in range(ng):
        k = g % len(KINDS_BNB)
        q, s, c = tri[KINDS_BNB[k]]
        j = (g // len(KINDS_BNB)) % len(q)
        b = g * BLOCKSIZE2 + (g * 5 + g // BLOCKSIZE2) % BLOCKSIZE2
        a1[b], a2[g], codes[b, :] = q[j], s[j], c[j]
        kind_of_block[b] = k
    flat = codes.reshape(-1)
    packed = ((flat[0::2] << 4) | flat[1::2]).astype(np.uint8)  # high nibble: even column
    out = (packed, a1, code2_np().copy(), a2, float(OFFSET), kind_of_block)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def drawn_weight_bnb(N, K, seed=0, blocksize=64, blocksize2=256, subnormal_scale=None):
    """(packed, a1, code2, a2, offset): an ordinary drawn nested weight, full statistics."""
    nblk = -(-N * K // blocksize)
    n2 = -(-nblk // blocksize2)
    packed = O.splitmix64_bytes(seed, N * K // 2, stream=1)
    a1 = O.splitmix64_bytes(seed, nblk, stream=2)
    a2 = O.uniform_f32(seed, n2, 1e-3, 1e-1, stream=3)
    offset = 0.0123
    if subnormal_scale is not None:
        a2 = (a2 * np.float32(subnormal_scale)).astype(np.float32)
        offset = float(np.float32(0.0123) * np.float32(subnormal_scale))
    return packed, a1, code2_np().copy(), a2, offset


def single_weight_bnb(N, K, seed=0, blocksize=64):
    """(packed, absmax): a drawn weight with fp32 statistics (compress_statistics=False)."""
    nblk = -(-N * K // blocksize)
    return O.splitmix64_bytes(seed, N * K // 2, stream=1), O.uniform_f32(seed, nblk, 1e-3, 1.0, stream=4)
