"""The acceptance set of the fused SwiGLU epilogue, shared by test_gpu_gemm_mt_swiglu.py,
test_gpu_swiglu_api.py and test_gpu_gemm_activations.py (test_swiglu_cpu.py checks this module
itself on the host, against torch's CPU chain).

The epilogue is defined on two 16-bit values g and u:

    s = rn(g / (1 + expf(-g)))   fp32, IEEE division            h = rn(s * u)   exact fp32 product

Everything here is computed on the CPU in float64 from bit patterns alone:

* ``s64 = g / (1 + exp(-g))`` in float64; ``s`` must be ``rn(s64)`` -- except where ``s64`` lies
  within 2^-21 relative of a 16-bit rounding tie, where either neighbour is allowed.  The margin
  is derived, not measured: fp32 ``expf`` has at most 1 ulp of error, the sum adds one rounding
  and the correctly rounded division one more, at most 2.5 * 2^-24 relative in all; 2^-21 is
  about three times that.
* ``h`` must be exactly ``rn(s * u)`` for an allowed ``s`` (the product of two 16-bit values is
  exact in float64, so this ``rn`` is computed exactly, ties to even).
* such near-tie elements may be at most 1 % of a case's elements (the reference alone gives
  0.06 - 0.11 % for N(0, 2) draws).
* the chain is fp32, so ``expf(-g)`` overflows to +inf once -g passes ln(FLT_MAX) = 88.7228 and
  ``s = g / inf = -0`` from there on, where a float64 silu would still give about -88.7 * 3e-39
  (a 16-bit subnormal in bf16).  ``silu64`` models that: exp(-g) at or above the fp32 overflow
  threshold (2 - 2^-24) * 2^127 counts as +inf.  The 1-ulp freedom of ``expf`` cannot change the
  outcome on either 16-bit grid: bf16 has no point near 88.7228 (its neighbours are 88.5, where
  exp is 0.80 of FLT_MAX, and 89.0, where it is 1.32 of it), and fp16's neighbours 88.6875 and
  88.75 give 0.965 and 1.028 of FLT_MAX, thousands of ulps from the threshold.
* non-finite g or u are judged only under ``accept(..., nonfinite=True)``: there ``h`` must have
  the class (NaN, +inf, -inf) that the same formula gives in numpy from an allowed 16-bit ``s``:
  silu(+inf) = +inf, silu(-inf) = -inf / inf = NaN, inf * 0 = NaN, anything with a NaN is NaN.
"""
from __future__ import annotations

import numpy as np

from _gemm_cases import bits_to_f64

_FMT = {"bf16": (8, -126), "f16": (11, -14)}  # significant bits, smallest normal exponent
TIE_MARGIN = 2.0 ** -21
NEAR_TIE_CAP = 0.01
EXPF_OVERFLOW = (2.0 - 2.0 ** -24) * 2.0 ** 127  # fp32 RNE gives +inf from here on


def neighbours(v, dt):
    """(lo, hi, spacing): the 16-bit grid points around float64 ``v`` (lo <= v <= hi, equal when
    ``v`` is on the grid) and the grid spacing there.  Exact: every step is a scaling by a power
    of two or a floor / ceil of a float64."""
    p, emin = _FMT[dt]
    v = np.asarray(v, np.float64)
    _, ex = np.frexp(np.abs(v))                         # |v| = m * 2^ex, m in [0.5, 1)
    e = np.maximum(ex - 1, emin)                        # zeros and subnormals: the subnormal grid
    sp = np.ldexp(1.0, e - (p - 1))
    return np.floor(v / sp) * sp, np.ceil(v / sp) * sp, sp


def rn16(v, dt):
    """Round-to-nearest-even of float64 ``v`` to the 16-bit format, as float64 (exact)."""
    lo, hi, sp = neighbours(v, dt)
    v = np.asarray(v, np.float64)
    dl, dh = v - lo, hi - v                             # exact: within one spacing of v
    even_lo = np.mod(np.abs(lo / sp), 2.0) == 0.0
    return np.where((dl < dh) | ((dl == dh) & even_lo), lo, hi)


def to_bits(v, dt):
    """The 16-bit pattern of a float64 that is on the format's grid (sign of zero kept)."""
    v = np.asarray(v, np.float64)
    if dt == "f16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    with np.errstate(over="ignore"):
        return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def silu64(g):
    """g / (1 + exp(-g)) in float64 with the fp32 overflow of ``expf`` modelled: where exp(-g) is
    at or above the fp32 overflow threshold the chain's divisor is +inf and s = g / inf, a zero
    with the sign of g (-0: only a negative g gets there); -inf gives -inf / inf = NaN."""
    g = np.asarray(g, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-g)
        e = np.where(e >= EXPF_OVERFLOW, np.inf, e)
        return g / (1.0 + e)


def allowed_s(g_bits, dt):
    """(s_a, s_b, near): the allowed 16-bit values of s as float64 -- s_a == s_b == rn(s64)
    except at near-tie elements (``near``), where they are the two neighbours."""
    s64 = silu64(bits_to_f64(np.asarray(g_bits, np.uint16), dt))
    lo, hi, _ = neighbours(s64, dt)
    tie = 0.5 * (lo + hi)                               # exact: one more bit than the grid
    near = (lo != hi) & (np.abs(s64 - tie) <= TIE_MARGIN * np.abs(tie))
    r = rn16(s64, dt)
    return np.where(near, lo, r), np.where(near, hi, r), near


def _cls(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    return np.where(np.isnan(v), 3, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 0)))


def accept(h_bits, g_bits, u_bits, dt, what="", nonfinite=False):
    """Fail unless every element of ``h_bits`` is in the acceptance set of (g_bits, u_bits) and
    at most 1 % of the elements are near a tie.  Returns the near-tie fraction.

    Non-finite g or u fail unless ``nonfinite`` is set; then, at those elements alone, ``h`` must
    have the class (NaN, +inf, -inf) of ``s * u`` for an allowed ``s`` (the 16-bit ``s`` of a
    finite g; silu64's own value of a non-finite one).  Such a product is never finite."""
    h_bits, g_bits, u_bits = (np.asarray(a, np.uint16) for a in (h_bits, g_bits, u_bits))
    assert h_bits.shape == g_bits.shape == u_bits.shape, (what, h_bits.shape, g_bits.shape, u_bits.shape)
    g, u = bits_to_f64(g_bits, dt), bits_to_f64(u_bits, dt)
    gfin = np.isfinite(g)
    fin = gfin & np.isfinite(u)
    assert nonfinite or fin.all(), f"{what}: non-finite g or u"
    sa, sb, near = allowed_s(np.where(gfin, g_bits, np.uint16(0)), dt)
    near = near & gfin
    with np.errstate(invalid="ignore"):
        sa, sb = np.where(gfin, sa, silu64(g)), np.where(gfin, sb, silu64(g))
        pa, pb = sa * u, sb * u
    ha, hb = (to_bits(rn16(np.where(fin, p, 0.0), dt), dt) for p in (pa, pb))
    ok = (h_bits == ha) | (h_bits == hb)
    if not fin.all():
        assert (_cls(pa)[~fin] != 0).all() and (_cls(pb)[~fin] != 0).all(), what
        hc = _cls(bits_to_f64(h_bits, dt))
        ok = np.where(fin, ok, (hc == _cls(pa)) | (hc == _cls(pb)))
    frac = float(near.mean())
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} elements outside the acceptance set, first at {i}: "
                             f"g {g_bits[i]:#06x} u {u_bits[i]:#06x} h {h_bits[i]:#06x}, allowed {ha[i]:#06x} / {hb[i]:#06x}")
    assert frac <= NEAR_TIE_CAP, f"{what}: {frac:.4%} of the elements are near a rounding tie (cap 1 %)"
    return frac


def swiglu_oracle(g_ref, g_tol, u_ref, u_tol, dt):
    """(h_ref, bound) of silu(g) * u in float64 from the float64 GEMM results and their bounds.

    With |g - g_ref| <= tg and |u - u_ref| <= tu (the suite's gemm_oracle bounds, which hold the
    16-bit rounding of g and u) and |silu'| <= 1.1 everywhere,
        |silu(g) - silu(g_ref)| <= 1.1 tg =: ts
        |silu(g) u - silu(g_ref) u_ref| <= ts |u_ref| + |silu(g_ref)| tu + ts tu =: e1.
    The chain rounds twice more -- s (half an ulp of s, so half an ulp's share of h) and h (half
    an ulp) -- one 16-bit ulp of |h| in all, taken at |h_ref| + e1: 2^-(p-1) of it plus the
    subnormal spacing.
    """
    p, emin = _FMT[dt]
    s_ref = silu64(g_ref)
    h_ref = s_ref * u_ref
    ts = 1.1 * g_tol
    e1 = ts * np.abs(u_ref) + np.abs(s_ref) * u_tol + ts * u_tol
    ulp = 2.0 ** -(p - 1) * (np.abs(h_ref) + e1) + 2.0 ** (emin - (p - 1))
    return h_ref, e1 + ulp
