"""The judge of the adapter suites (tests/_lora_cases.py) tested where no GPU is needed: torch's
own fp32-accumulated chain on the host lies inside the bound at every element, two broken chains
-- one that drops the last 32 of K, one that drops the last rank index -- are caught in most
elements, ``tol_t`` is ``_gemm_cases.tol``, and the exact probes keep their premise.

The rounding-chain probes (``rounding_case``): ``rn`` is torch's conversion; every probe builds --
the premise, the shares and the ties are the builder's own assertions -- and torch's fp32-accumulated
chain on the host gives the expected bits; each of five broken chains differs from them in at least
1 % of the outputs at every shape, dtype and scale.  The special rows (``special_case``,
``check_classes``): the honest chain is accepted and isolated, and a NaN leaked into a plain row, a
finite value where an infinity is due and the wrong infinity are each rejected; the overflow probe
has the classes it is built for."""
import numpy as np
import pytest
import torch

import _lora_cases as C
from _activation_cases import isolated, positions
from _lora_cases import TDT, check, drawn_case, exact_case, gemm_tol, lora_oracle, outside, tol_t, torch_chain, worst_ratio

SHAPES = [(1, 128, 8, 64), (5, 96, 24, 80), (17, 384, 32, 192), (33, 1024, 64, 64), (128, 4096, 16, 64)]  # M, K, r, N
SCALE = 2.0


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_tol_t_is_the_gemm_bound(dt):
    g = torch.Generator().manual_seed(1)
    ref, mag = torch.randn(7, 9, generator=g, dtype=torch.float64), torch.rand(7, 9, generator=g, dtype=torch.float64) * 50
    assert np.array_equal(tol_t(ref, mag, dt).numpy(), gemm_tol(ref.numpy(), mag.numpy(), dt))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_chain_inside_and_broken_chains_outside(shape, dt):
    M, K, r, N = shape
    x, A, B, base = drawn_case(M, K, r, N, dt)
    for b in (base, None):
        ref, bound = lora_oracle(x, A, B, SCALE, dt, b)
        good = torch_chain(x, A, B, SCALE, b)
        assert good.dtype == TDT[dt]
        check(good, ref, bound, f"{shape} {dt}")
        assert worst_ratio(good, ref, bound) < 1.0
        short_k = torch_chain(x[:, :K - 32].contiguous(), A[:, :K - 32].contiguous(), B, SCALE, b)
        short_r = torch_chain(x, A[:r - 1].contiguous(), B[:, :r - 1].contiguous(), SCALE, b)
        for name, broken in (("K - 32", short_k), ("r - 1", short_r)):
            frac = float(outside(broken, ref, bound).double().mean())
            assert frac > 0.5, (shape, dt, name, frac)
            with pytest.raises(AssertionError):
                check(broken, ref, bound, name)


def test_nan_inf_and_a_wrong_scale_are_caught():
    x, A, B, base = drawn_case(5, 96, 24, 80, "bf16")
    ref, bound = lora_oracle(x, A, B, SCALE, "bf16", base)
    good = torch_chain(x, A, B, SCALE, base)
    for bad_value in (float("nan"), float("inf")):
        y = good.clone()
        y[2, 3] = bad_value
        assert int(outside(y, ref, bound).sum()) == 1
    assert float(outside(torch_chain(x, A, B, -SCALE, base), ref, bound).double().mean()) > 0.5
    ref0, bound0 = lora_oracle(x, A, B, 0.0, "bf16", base)
    check(base, ref0, bound0, "scale 0 is the base")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_exact_probes_keep_their_premise(dt):
    for M, K, r, N in ((5, 96, 24, 80), (33, 384, 128, 192)):
        x, A, B, base, y, v = exact_case(M, K, r, N, dt)
        for a in (x, A, B):
            assert set(a.double().unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert int((A != 0).sum(1).max()) <= 8 and int((B != 0).sum(1).max()) <= 8
        assert float(base.double().abs().max()) <= 16
        assert torch.equal(torch_chain(x, A, B, 0.5, base), y) and torch.equal(torch_chain(x, A, B, 0.5), v)
        ref, bound = lora_oracle(x, A, B, 0.5, dt, base)
        assert torch.equal(ref, y.double())


# ---- the rounding-chain probes --------------------------------------------------------------------------
PROBES = [(1, 32, 8, 16), (5, 96, 24, 80), (33, 384, 128, 192), (128, 384, 64, 192),  # test_gpu_lora.py runs the same,
          (33, 384, 24, 80), (33, 384, 8, 16)]                                          # and the last three in one group
PROBE_SCALES = (1.5, 0.3)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rn_is_the_dtypes_conversion(dt):
    """``rn`` (mode "even") against torch's fp32 -> 16-bit conversion on draws of every size, on exact
    ties, on subnormals and at the overflow threshold; the two other modes where they must differ."""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(20000) * 2.0 ** rng.integers(-30, 17, 20000)).astype(np.float32).astype(np.float64)
    ulp = 2.0 ** (1 - C.SIG[dt])
    ties = (1.0 + ulp * (np.arange(64) + 0.5)) * 2.0 ** rng.integers(-10, 10, 64)      # halfway between neighbours
    edge = np.array([0.0, -0.0, 65504.0, 65519.0, 65520.0, -65520.0, 1e30, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26,
                     C.FMAX["bf16"], float(np.float32(3.4e38)), np.inf, -np.inf, np.nan])
    v = np.concatenate([v, ties, -ties, edge])
    want = C.widen(torch.from_numpy(v.astype(np.float32)).to(TDT[dt]))
    got = C.rn(v, dt)
    ok = ~np.isnan(want)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    t = np.abs(ties)
    assert (C.rn(t, dt, "zero") < t).all() and (C.rn(t, dt, "away") > t).all()
    assert ((C.rn(t, dt) == C.rn(t, dt, "zero")) != (C.rn(t, dt) == C.rn(t, dt, "away"))).all()
    assert (C.rn(t, dt) == C.rn(t, dt, "away")).sum() == 32                                # every other tie goes up


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("scale", PROBE_SCALES)
def test_rounding_probes_keep_their_premise_and_their_shares(scale, dt):
    ties = {"t": 0, "u": 0}
    for shape in PROBES:
        x, A, B, base, y, v = C.rounding_case(*shape, dt, scale)    # asserts the premise (2^24), the 5 % shares, no overflow
        for a in (x, A, B, base, y, v):
            assert a.dtype == TDT[dt]
        n = [C.widen(a) for a in (x, A, B, base)]
        worst = C.premise(n[0], n[1], 1.0), C.premise(C.rn(C._dot(n[0], n[1]), dt), n[2], float(np.abs(n[2][n[2] != 0]).min()))
        assert max(worst) < 2.0 ** 20, worst                         # in fact far below the cap: 2^11 .. 2^18
        st = C.rounding_stats(*n, scale, dt)
        for name in "tuvy":
            assert 20 * st[name + "_inexact"] >= st[name + "_numel"], (shape, name, st)
        ties["t"] += st["t_ties"]
        ties["u"] += st["u_ties"]
        # fp32 accumulation in any order gives these bits: torch's own chain on the host does
        assert torch.equal(torch_chain(x, A, B, scale, base).view(torch.int16), y.view(torch.int16)), shape
        assert torch.equal(torch_chain(x, A, B, scale).view(torch.int16), v.view(torch.int16)), shape
        if shape[0] * shape[2] >= 512:
            assert st["t_ties"] >= 16 and st["u_ties"] >= 16, (shape, st)
    assert ties["t"] >= 16 and ties["u"] >= 16


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("scale", PROBE_SCALES)
def test_every_broken_chain_is_told_apart_by_the_probes(scale, dt):
    for shape in PROBES:
        x, A, B, base, y, v = (C.widen(a) for a in C.rounding_case(*shape, dt, scale))
        good = C.chain16(x, A, B, base, scale, dt)
        assert np.array_equal(good[0], y) and np.array_equal(good[1], v)
        for broken in C.BREAKS:
            yb, vb = C.chain16(x, A, B, base, scale, dt, broken=broken)
            frac = float((yb != y).mean())
            assert frac >= 0.01, (shape, dt, scale, broken, frac)
            if broken != "v":                                        # with base = NULL the "v" chain is the right one
                assert float((vb != v).mean()) >= 0.01, (shape, dt, scale, broken)


def test_the_premise_stops_a_probe_that_is_too_large():
    x, A, B, base = C.rounding_inputs(5, 96, 24, 80, "bf16")
    with pytest.raises(AssertionError):
        C.chain16(x * 4096, A, B, base, 1.5, "bf16")                 # sum |x| |A| of 2^24 and more
    with pytest.raises(AssertionError):
        C.chain16(x + 0.5, A, B, base, 1.5, "bf16")                  # off the grid


def test_the_overflow_probe_has_its_classes():
    x, A, B, base, y, v = C.overflow_case()
    assert y.dtype == torch.float16 and bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(A.float()).all())
    t = C.rn(C._dot(C.widen(x), C.widen(A)), "f16")
    assert np.isinf(t).any() and np.abs(C._dot(C.widen(x), C.widen(A))).max() > 65520
    for z in (y, v):
        assert bool(torch.isnan(z).any()) and bool(torch.isposinf(z).any()) and bool(torch.isneginf(z).any())
        assert float(torch.isfinite(z).float().mean()) > 0.25
    assert bool(C.same_bits_or_nan(y, y.clone()).all())
    wrong = y.clone()
    wrong[torch.isnan(y)] = float("inf")
    assert not bool(C.same_bits_or_nan(wrong, y).all())
    wrong = y.clone()
    wrong[torch.isposinf(y)] = 65504.0
    assert not bool(C.same_bits_or_nan(wrong, y).all())


# ---- the special rows and their judge -----------------------------------------------------------------------
def _honest(x, A, B, base, scale, dt):
    """The header's chain on the host (float64 sums: within the bound of any fp32 order), as 16-bit tensors."""
    y, v = C.chain16(C.widen(x), C.widen(A), C.widen(B), C.widen(base), scale, dt, cap=None)
    return tuple(torch.from_numpy(z.astype(np.float32)).to(TDT[dt]) for z in (y, v))


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 5, 17, 33])
def test_class_judge_accepts_the_honest_chain_and_rejects_each_mutant(M, dt):
    K, N, scale = 96, 80, 1.5
    seen = set()
    for r in (8, 40):
        for a_col in ("nonzero", "mixed"):
            for kinds in C.special_kind_sets(M, dt):
                xs, x, A, B, base, rows = C.special_case(M, K, r, N, dt, kinds, a_col)
                assert sorted(rows.values()) == sorted(kinds) and sorted(rows) == sorted(positions(M, len(kinds)))
                assert set(np.flatnonzero((_bits(xs) != _bits(x)).any(1)).tolist()) == set(rows)
                seen |= set(kinds)
                ref, bound = C.lora_oracle_rows(xs, A, B, scale, dt, base)
                y, v = _honest(xs, A, B, base, scale, dt)
                yp, _ = _honest(x, A, B, base, scale, dt)
                what = f"M={M} r={r} {a_col} {kinds}"
                C.check_classes(y, ref, bound, what)
                C.check_classes(v, *C.lora_oracle_rows(xs, A, B, scale, dt), what)
                isolated(_bits(y), _bits(yp), rows, what)
                plain = [m for m in range(M) if m not in rows]
                for m in plain:                                       # a plain row's reference is the plain call's
                    assert bool(torch.isfinite(ref[m]).all()) and bool(torch.isfinite(bound[m]).all())
                for row, kind in rows.items():
                    if kind == "nan" or (kind in ("pinf", "ninf") and a_col == "mixed"):
                        assert bool(torch.isnan(ref[row]).all()) and bool(torch.isnan(y[row]).all())
                    elif kind in ("pinf", "ninf"):                    # a mix of the infinity and NaN, not all NaN
                        inf = torch.isposinf(ref[row]) if kind == "pinf" else torch.isneginf(ref[row])
                        assert int(inf.sum()) >= N // 2 and bool(torch.isnan(ref[row]).any()) and not bool(torch.isfinite(ref[row]).any())
                        bad = y.clone()
                        bad[row] = torch.where(torch.isinf(y[row]), -y[row], y[row])
                        with pytest.raises(AssertionError):
                            C.check_classes(bad, ref, bound, "the other infinity")
                        bad = y.clone()
                        bad[row] = torch.where(torch.isinf(y[row]), torch.full_like(y[row], C.FMAX["f16"]), y[row])
                        with pytest.raises(AssertionError):
                            C.check_classes(bad, ref, bound, "a finite value where the infinity is due")
                        bad = y.clone()
                        bad[row] = torch.where(torch.isnan(y[row]), torch.zeros_like(y[row]), y[row])
                        with pytest.raises(AssertionError):
                            C.check_classes(bad, ref, bound, "inf * 0 given as 0")
                    elif kind in ("zero", "negzero"):
                        assert torch.equal(y[row].float(), base[row].float()) and bool((v[row] == 0).all())
                    else:
                        assert float((v[row] != 0).float().mean()) > 0.9
                if plain and any(k in ("nan", "pinf", "ninf") for k in kinds):
                    bad = y.clone()
                    bad[plain[0], 3] = float("nan")
                    with pytest.raises(AssertionError):
                        C.check_classes(bad, ref, bound, "a NaN leaked into a plain row")
                    with pytest.raises(AssertionError):
                        isolated(_bits(bad), _bits(yp), rows, "a NaN leaked into a plain row")
                    bad = y.clone()
                    bad.view(torch.int16)[plain[0], 5] ^= 1           # one ulp in a plain row: not isolated
                    with pytest.raises(AssertionError):
                        isolated(_bits(bad), _bits(yp), rows)
    assert seen == {k for g in C.SPECIAL[dt] for k in g}
