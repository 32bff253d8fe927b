"""The GEMM suites' shared helpers (tests/_gemm_cases.py) checked on the host, no GPU.

The exact-weight probe on the GPU (test_gpu_gemm_exact.py) can only catch a kernel whose
weights are computed a near-miss way if its inputs tell the near misses from the
reference.  That is checked here, on the reference alone: the near-miss restatements
below are written out in numpy from oracle/nf4_oracle.py::ref_scales / _apply, each with
one step changed, and must differ from the oracle on the built weight.
"""
from fractions import Fraction

import numpy as np
import pytest

import _gemm_cases as G
import nf4_oracle as O

_F127 = np.float32(127.0)


# ---- check_close ----------------------------------------------------------------------------
def _twins():
    import torch

    def np_check(got, ref, tol):
        G.check_close(np.array(got), np.array(ref), np.array(tol), "np")

    def torch_check(got, ref, tol):
        G.check_close_t(torch.tensor(got, dtype=torch.float32), torch.tensor(ref, dtype=torch.float64),
                        torch.tensor(tol, dtype=torch.float64), "torch")

    return [np_check, torch_check]


@pytest.mark.parametrize("which", [0, 1])
def test_check_close_rejects_nan_inf_and_just_outside(which):
    check = _twins()[which]
    ref, tol = [1.0, 2.0, -3.0], [0.25, 0.25, 0.25]
    check([1.25, 1.75, -3.0], ref, tol)  # at tol (all exact in fp32): passes
    check([1.0, 2.0, -3.0], ref, [0.0, 0.0, 0.0])
    for bad in (float("nan"), float("inf"), float("-inf"), 2.0 + 0.25 + 2.0 ** -20, 2.0 - 0.25 - 2.0 ** -20):
        with pytest.raises(AssertionError, match="1 of 3 outside"):
            check([1.0, bad, -3.0], ref, tol)
    # the form the suites used to have lets the NaN through
    got = np.array([np.nan, 2.0])
    assert not (np.abs(got - np.array([1.0, 2.0])) > 0.25).any()
    with pytest.raises(AssertionError, match="1 NaN"):
        check([float("nan"), 2.0, -3.0], ref, tol)
    # a NaN tolerance (inf - inf in a bound) does not pass anything either
    with pytest.raises(AssertionError):
        check([1.0, 2.0, -3.0], ref, [0.25, float("nan"), 0.25])


# ---- the near-miss restatements, whole matrices ---------------------------------------------
def _scales(a1, a2, m, n, how):
    """oracle/nf4_oracle.py::ref_scales with the scale computed `how`."""
    bpr = (n + 63) // 64
    g = (bpr + 3) // 4
    r = np.arange(m, dtype=np.int64)[:, None]
    b = np.arange(bpr, dtype=np.int64)[None, :]
    q = a1[(r * bpr + b) % a1.size].astype(np.float32)
    s2 = a2.astype(np.float32)[(r * g + b // 4) % a2.size]
    if how == "reference":
        return ((q / _F127) * s2).astype(np.float32)
    if how == "reciprocal_scale":
        return ((q * (np.float32(1.0) / _F127)).astype(np.float32) * s2).astype(np.float32)
    if how == "reordered_scale":
        return ((q * s2).astype(np.float32) / _F127).astype(np.float32)
    raise ValueError(how)


def _round_once(exact, dt):
    """float64 -> 16-bit pattern, one RNE rounding; written apart from G.round_once_bits
    (integer arithmetic on the float64 pattern; normal 16-bit range or zero only)."""
    if dt == "f16":
        return exact.astype(np.float16).view(np.uint16)  # numpy rounds float64 -> float16 once
    u = exact.view(np.uint64)
    drop = np.uint64(52 - 7)
    r = (u + ((np.uint64(1) << (drop - np.uint64(1))) - np.uint64(1)) + ((u >> drop) & np.uint64(1))) >> drop
    back = (r << drop).view(np.float64).astype(np.float32)  # exact: 8 significant bits
    assert ((np.abs(back) >= 2.0 ** -126) | (back == 0)).all()
    return (back.view(np.uint32) >> 16).astype(np.uint16)


def _restated(packed, a1, a2, m, n, dt, kind):
    vals = O._decode(packed, m, n)
    how = kind if kind in ("reciprocal_scale", "reordered_scale") else "reference"
    s = np.repeat(_scales(a1, a2, m, n, how), 64, axis=1)[:, :n]
    if kind == "single_rounding":
        return _round_once(vals.astype(np.float64) * s.astype(np.float64), dt)
    return O.to_bits((vals * s).astype(np.float32), O.BF16 if dt == "bf16" else O.F16)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", [(64, 2048), (128, 1024), (128, 4096)])
def test_sensitive_weight_tells_every_near_miss_apart(coracle, dt, N, K):
    packed, a1, a2, kind_of_block = G.sensitive_weight(N, K, dt)
    assert a1.size == N * K // 64 and a2.size == N * (-(-(K // 64) // 4))
    code = O.BF16 if dt == "bf16" else O.F16
    want = coracle.dequant_ref(packed, a1, a2, N, K, code)
    assert np.array_equal(want, _restated(packed, a1, a2, N, K, dt, "reference"))
    assert np.isfinite(G.bits_to_f64(want, dt)).all()
    for k, kind in enumerate(G.KINDS):
        diff = _restated(packed, a1, a2, N, K, dt, kind) != want
        rows, cols = np.nonzero(diff)
        blocks = set(zip(rows.tolist(), (cols // 64).tolist()))
        print(f"sensitivity {dt} {N}x{K} {kind}: {int(diff.sum())} elements in {len(blocks)} blocks")
        assert diff.sum() >= 32 and len(blocks) >= 16, (kind, int(diff.sum()), len(blocks))
        assert (cols % 2 == 0).any() and (cols % 2 == 1).any(), kind  # high- and low-nibble columns
        # the blocks built for this near miss differ in all their 64 elements
        mine = kind_of_block == k
        assert mine.sum() >= 16 and diff.reshape(N, K // 64, 64)[mine].all(), kind


# ---- the double-rounding cases of test_gpu_parity.py ----------------------------------------
def _fraction_round(x: Fraction, p: int, emin: int) -> Fraction:
    """x rounded once, ties to even, to p significant bits (spacing never below 2^emin)."""
    if x == 0:
        return x
    e = 0
    while abs(x) >= Fraction(2) ** e:
        e += 1
    while abs(x) < Fraction(2) ** (e - 1):
        e -= 1
    q = Fraction(2) ** max(e - p, emin)
    return round(x / q) * q  # Python's round(): half to even


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_double_rounding_scales_are_genuine(dt):
    from test_gpu_parity import _double_rounding_scales

    s, c = _double_rounding_scales(dt)
    assert len(s) == 64 and s.dtype == np.float32 and len(set(zip(s.tolist(), c.tolist()))) == 64
    p, emin = (8, -133) if dt == "bf16" else (11, -24)
    for sv, cv in zip(s.tolist(), c.tolist()):
        exact = Fraction(float(O.NF4_LUT[cv])) * Fraction(sv)
        once = _fraction_round(exact, p, emin)
        twice = _fraction_round(_fraction_round(exact, 24, -149), p, emin)
        assert once != twice, (sv, cv)
        # and the oracle's arithmetic is the "twice" one
        bits = G.weight_bits(np.array([sv], np.float32), np.array([cv]), dt)
        assert Fraction(float(G.bits_to_f64(bits, dt)[0])) == twice


def test_round_once_matches_an_independent_rounding():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(200000) * np.exp2(rng.integers(-12, 3, 200000))
    for dt in ("bf16", "f16"):
        assert np.array_equal(G.round_once_bits(x, dt), _round_once(x, dt))
    # halfway cases go to even, subnormals keep their fixed grid, zeros keep their sign
    assert G.round_once_bits(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]), "bf16").tolist() == [0x3F80, 0x3F82]
    assert G.round_once_bits(np.array([2.0 ** -25, 3 * 2.0 ** -25, -0.0]), "f16").tolist() == [0, 2, 0x8000]
