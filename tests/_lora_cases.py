"""Inputs and the judge of the fused adapter launch (nf4_lora_add, nf4_linear_lora_bnb):
shared by test_gpu_lora.py and test_gpu_lora_api.py; test_lora_cases_cpu.py checks this module
itself on the host.

The reference is the float64 chain of the 16-bit inputs with NO intermediate rounding,

    t = x A^T      u = t B^T      v = u * scale      y = base + v,

and the bound is the suite's GEMM bound ``_gemm_cases.tol`` carried through the chain.  With
p = 8 (bf16) or 10 (fp16) and ``sub`` as in ``tol``:

    bt = tol(t, |x| |A|^T)
    bu = bt |B|^T (1 + 2^-p) + tol(u, (|t| + bt) |B|^T)
    bv = bu |scale| (1 + 2^-p) + 2^-p |v| + sub
    by = bv (1 + 2^-p) + 2^-p |y| + sub            (+ the base's own bound, when it has one)

bt covers the fp32 summation and the rounding of t; the first term of bu carries t's error through
the second product (and through the rounding of u, hence 1 + 2^-p), the second is the second
product's own GEMM bound over the perturbed |t|; bv and by add one rounding each.  Everything is
torch float64 so the same code judges on the host and on the device.

``rounding_case`` builds the rounding-chain probes: integers (over a power of two) so large that each
of the header's four roundings changes its value, yet with both fp32 sums exact in any order, so the
expected bits are unique and ``chain16`` computes them on the host; ``overflow_case`` is the same with
some t beyond the fp16 range.  ``lora_oracle_rows`` / ``check_classes`` judge calls whose x has NaN,
infinite, zero or tiny rows (test_gpu_lora_activations.py).

``exact_case`` builds the exact probes: x, A and B in {-1, 0, 1} with at most 8 non-zeros per row
of A and per row of B, scale 0.5 and an integer base in [-16, 16].  Every intermediate is then a
half-integer of at most 8 significant bits, every fp32 summation order and every rounding is
exact, and y must equal integer arithmetic bit for bit.  The builder asserts that premise.
"""
from __future__ import annotations

import numpy as np
import torch

from _gemm_cases import tol as gemm_tol

TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
P_SUB = {"bf16": (8, 2.0 ** -134), "f16": (10, 2.0 ** -25)}


def tol_t(ref, mag, dt):
    """``_gemm_cases.tol`` on torch float64 tensors (test_lora_cases_cpu.py holds the two equal)."""
    p, sub = P_SUB[dt]
    return 2.0 ** -p * ref.abs() + 2.0 ** -20 * mag + sub


def f32(scale) -> float:
    """The fp32 the C entry receives, as a Python float."""
    return float(np.float32(scale))


def lora_oracle(x, A, B, scale, dt, base=None, base_bound=None):
    """(y_ref, by) in float64 on the inputs' device.  x, A, B: 16-bit tensors; base: None, a 16-bit
    tensor, or a float64 reference with its own bound ``base_bound`` (added to by)."""
    p, sub = P_SUB[dt]
    e = 1.0 + 2.0 ** -p
    s = f32(scale)
    xf, Af, Bf = x.double(), A.double(), B.double()
    t = xf @ Af.T
    bt = tol_t(t, xf.abs() @ Af.abs().T, dt)
    u = t @ Bf.T
    bu = bt @ Bf.abs().T * e + tol_t(u, (t.abs() + bt) @ Bf.abs().T, dt)
    v = u * s
    bv = bu * abs(s) * e + 2.0 ** -p * v.abs() + sub
    if base is None:
        return v, bv
    y = base.double() + v
    by = bv * e + 2.0 ** -p * y.abs() + sub
    if base_bound is not None:
        by = by + base_bound
    return y, by


def outside(got, ref, bound):
    """Boolean mask of the elements where ``abs(got - ref) <= bound`` is NOT true (NaN, inf included)."""
    return ~((got.double() - ref).abs() <= bound)


def check(got, ref, bound, what=""):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = outside(got, ref, bound)
    if bool(bad.any()):
        g = got.double()
        ratio = (g - ref).abs() / bound
        fin = ratio[torch.isfinite(ratio)]
        worst = float(fin.max()) if fin.numel() else float("nan")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound "
                             f"({int(torch.isnan(g).sum())} NaN, {int(torch.isinf(g).sum())} inf); "
                             f"worst error {worst:.3g} of the bound")


def worst_ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


def drawn_case(M, K, r, N, dt, seed=0):
    """(x [M, K], A [r, K], B [N, r], base [M, N]) as 16-bit host tensors: x, t, u and base all of
    unit size, so that a wrong delta is not hidden behind the base's rounding."""
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * K))  # of (seed, M, K) alone
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * K + 17 * r + N + 1)
    A = torch.randn(r, K, generator=g) / K ** 0.5
    B = torch.randn(N, r, generator=g) / r ** 0.5
    base = torch.randn(M, N, generator=g)
    return tuple(a.to(TDT[dt]) for a in (x, A, B, base))


def torch_chain(x, A, B, scale, base=None):
    """PEFT's expression on 16-bit tensors as torch computes it (fp32 accumulation, four roundings)."""
    u = torch.nn.functional.linear(torch.nn.functional.linear(x, A), B)
    v = u * f32(scale)
    return v if base is None else base + v


def _sparse_signs(rows, cols, nnz, g):
    out = torch.zeros(rows, cols)
    for i in range(rows):
        idx = torch.randperm(cols, generator=g)[:min(nnz, cols)]
        out[i, idx] = torch.randint(0, 2, (idx.numel(),), generator=g).float() * 2 - 1
    return out


def exact_case(M, K, r, N, dt, seed=0):
    """(x, A, B, base, y_want, v_want) as 16-bit host tensors; scale is 0.5.  y_want = base + v_want
    and v_want = (x A^T B^T) / 2 in exact arithmetic."""
    g = torch.Generator().manual_seed(77 + seed + M + K + r + N)
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    A = _sparse_signs(r, K, 8, g)
    B = _sparse_signs(N, r, 8, g)
    base = torch.randint(-16, 17, (M, N), generator=g).float()
    t = x.double() @ A.double().T
    u = t @ B.double().T
    v = u * 0.5
    y = base.double() + v
    for name, z in (("t", t), ("u", u), ("v", v), ("y", y)):  # the premise: half-integers of <= 8 significant bits
        z2 = z * 2
        assert bool((z2 == z2.round()).all()) and float(z2.abs().max()) < 256, name
    assert float(u.abs().max()) > 2, "a probe that exercises nothing"
    cast = lambda a: a.to(TDT[dt])  # noqa: E731 -- exact: every value is representable
    out = tuple(cast(a) for a in (x, A, B, base, y, v))
    assert torch.equal(out[4].double(), y) and torch.equal(out[5].double(), v)
    return out


# ---- the header's rounding chain on the host, and the probes that make every rounding of it real ------
SIG = {"bf16": 8, "f16": 11}            # significant bits
EMIN = {"bf16": -126, "f16": -14}       # exponent of the smallest normal
FMAX = {"bf16": (2.0 - 2.0 ** -7) * 2.0 ** 127, "f16": 65504.0}
CAP = 2.0 ** 24                         # the premise's cap on sum |a| |b| in grid units: fp32's significand
BREAKS = ("t", "u", "v", "zero", "away")


def widen(a):
    """A 16-bit (or any) torch tensor as a float64 numpy array."""
    return a.detach().cpu().float().numpy().astype(np.float64)


def rn(v, dt, mode="even"):
    """float64 -> the values of ``dt``, as float64: round to nearest even (the header's rn), or, for the
    broken chains of test_lora_cases_cpu.py, "zero" (truncate) and "away" (halves away from zero).
    Subnormals are kept, an overflow is the infinity ("zero": the format's max), inf and NaN pass.
    Exact for any input of at most 53 - SIG significant bits more than its result, as every fp32 is."""
    v = np.asarray(v, np.float64)
    out = v.copy()
    fin = np.isfinite(v) & (v != 0)
    a = np.abs(v[fin])
    e = np.maximum(np.frexp(a)[1] - 1, EMIN[dt])
    ulp = np.ldexp(1.0, e - (SIG[dt] - 1))
    q = a / ulp
    q = np.rint(q) if mode == "even" else np.floor(q) if mode == "zero" else np.floor(q + 0.5)
    assert mode in ("even", "zero", "away")
    r = q * ulp
    r = np.where(r > FMAX[dt], FMAX[dt] if mode == "zero" else np.inf, r)
    out[fin] = np.copysign(r, v[fin])
    return out


def to16(v, dt):
    """float64 values of ``dt`` as a 16-bit host tensor; asserts that nothing is rounded (NaN stays NaN)."""
    t = torch.from_numpy(np.asarray(v, np.float64).astype(np.float32)).to(TDT[dt])
    back = widen(t)
    assert np.array_equal(back, np.asarray(v, np.float64), equal_nan=True), "not values of the dtype"
    return t


def _dot(a, b):
    """sum_j a[m][j] b[n][j] in float64 by elementwise product and sum (no BLAS: a routine that skips
    zero operands would lose inf * 0 = NaN); exact wherever the premise holds."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a[:, None, :] * b[None, :, :]).sum(-1)


def premise(a, b, grid, cap=CAP):
    """sum |a| |b| over the whole reduction, in units of the terms' common grid: every product a
    multiple of ``grid`` and the largest sum below ``cap``.  Then every partial sum, in any order and
    association, is an integer below 2^24 in those units, and fp32 holds it exactly.  ``a`` holds
    integers, ``b`` multiples of ``grid``; an infinite a (the overflow probe) is no term of a finite sum."""
    fa = np.where(np.isfinite(a), a, 0.0)
    for z, g in ((fa, 1.0), (b, grid)):
        assert np.array_equal(z / g, np.round(z / g)), "a value off its grid"
    worst = float((np.abs(fa) @ np.abs(b).T).max()) / grid
    assert worst < cap, (worst, cap)
    return worst


def chain16(x, A, B, base, scale, dt, broken=None, cap=CAP):
    """The header's chain on float64 numpy arrays holding values of ``dt``:

        t = rn(exact x A^T)    u = rn(exact t B^T)    v = rn(fp32(u) * fp32(scale))    y = rn(fp32(base) + fp32(v))

    the two sums exact in float64, the product and the add one fp32 operation each.  Returns (y, v)
    as float64 values of ``dt``; v is the output under base = NULL.  ``broken`` names one departure
    (BREAKS): "t" not rounded; "u" not rounded, the scale applied to the fp32 sum; "v" not rounded,
    the base added to the fp32 product and one rounding; "zero" / "away": every rounding in that mode.
    ``cap``: the premise is asserted for both sums (None: not at all, for inputs that are no probe)."""
    mode = broken if broken in ("zero", "away") else "even"
    s = np.float32(f32(scale))
    if cap is not None:
        premise(x, A, 1.0, cap)
    t = _dot(x, A)
    if broken != "t":
        t = rn(t, dt, mode)
    if cap is not None:
        grid = float(np.abs(B[B != 0]).min())
        premise(t, B, grid, cap)
    u = _dot(t, B)
    if broken != "u":
        u = rn(u, dt, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        u32 = u.astype(np.float32)
        assert np.array_equal(u32.astype(np.float64), u, equal_nan=True)  # exact in fp32, rounded or not
        p = u32 * s
        v = rn(p.astype(np.float64), dt, mode)
        if broken == "v":
            y = rn((base.astype(np.float32) + p).astype(np.float64), dt, mode)
        else:
            y = rn((base.astype(np.float32) + v.astype(np.float32)).astype(np.float64), dt, mode)
    return y, v


def _t_target(dt, K, overflow):
    """Half-width of the integers of x and A: t of about 2 * 2^SIG, so its rounding unit is 1 .. 8 and
    both inexact values and exact ties are frequent; for the overflow probe about 30000, fp16."""
    want = 30000.0 if overflow else 2.0 * 2.0 ** SIG[dt]
    return max(2, int(np.ceil((3.0 * want / K ** 0.5) ** 0.5)))


def rounding_inputs(M, K, r, N, dt, seed=0, overflow=False):
    """(x, A, B, base) as float64 numpy arrays of values of ``dt``.  x and A: integers in [-m, m], m
    chosen for K (``_t_target``).  B: min(8, r) non-zeros per row, k / 2 (bf16) or k / 8 (fp16: u stays
    far under 65504) with 1 <= |k| <= 3 -- a grid a few steps below u's rounding unit, so that u has
    exact ties.  base: k / 8 over +-8 rounding units of a typical v, so that the last add is rarely
    absorbed and rarely exact."""
    rng = np.random.default_rng([seed, M, K, r, N, SIG[dt], int(overflow)])
    m = _t_target(dt, K, overflow)
    x = np.random.default_rng([seed, M, K, SIG[dt], int(overflow)]).integers(-m, m + 1, (M, K)).astype(np.float64)  # of (seed, M, K) alone
    A = rng.integers(-m, m + 1, (r, K)).astype(np.float64)
    kmax, den = (3, 2.0) if dt == "bf16" else (3, 8.0)
    nnz = min(8, r)
    cols = np.argsort(rng.random((N, r)), axis=1, kind="stable")[:, :nnz]
    vals = rng.integers(1, kmax + 1, (N, nnz)) * (2 * rng.integers(0, 2, (N, nnz)) - 1) / den
    B = np.zeros((N, r))
    np.put_along_axis(B, cols, vals, axis=1)
    t_typ = m * (m + 1) / 3.0 * K ** 0.5
    v_typ = nnz ** 0.5 * t_typ * (kmax + 1) / 2.0 / den
    half = int(max(8, min(2.0 ** SIG[dt] - 1, 64.0 * v_typ / 2.0 ** SIG[dt])))  # in eighths: 8 units of v's rounding
    base = rng.integers(-half, half + 1, (M, N)) / 8.0
    return x, A, B, base


_ROUNDING = {}


def rounding_case(M, K, r, N, dt, scale, seed=0, cap=CAP):
    """(x, A, B, base, y_want, v_want) as 16-bit host tensors: a probe whose expected bits are unique
    -- both fp32 sums are exact in any order (``premise``, asserted) -- and in which every one of the
    four roundings of the header's chain matters: each changes at least 5 % of its elements (at
    least one where there are fewer than 20), nothing overflows, and where t has 512 elements or
    more, at least 16 of t and 16 of u are exact ties, which tell round-half-even from
    round-half-away.  (The smallest shape has 8 elements of t and 16 of u; test_lora_cases_cpu.py
    asserts the ties over the probe set and that every broken chain is told apart at every shape.)"""
    key = (M, K, r, N, dt, f32(scale), seed, cap)
    if key in _ROUNDING:
        return _ROUNDING[key]
    x, A, B, base = rounding_inputs(M, K, r, N, dt, seed)
    y, v = chain16(x, A, B, base, scale, dt, cap=cap)
    st = rounding_stats(x, A, B, base, scale, dt)
    for name in ("t", "u", "v", "y"):
        assert st[name + "_inexact"] >= max(1, int(np.ceil(0.05 * st[name + "_numel"]))), (name, st)
    if st["t_numel"] >= 512:
        assert st["t_ties"] >= 16 and st["u_ties"] >= 16, st
    assert np.isfinite(y).all() and np.isfinite(v).all() and st["max"] < FMAX[dt], "a probe must not overflow"
    out = tuple(to16(a, dt) for a in (x, A, B, base, y, v))
    _ROUNDING[key] = out
    return out


def rounding_stats(x, A, B, base, scale, dt):
    """How many elements each of the four roundings changes, and the exact ties of the first two."""
    s = np.float32(f32(scale))
    te = _dot(x, A)
    t = rn(te, dt)
    ue = _dot(t, B)
    u = rn(ue, dt)
    pe = (u.astype(np.float32) * s).astype(np.float64)
    v = rn(pe, dt)
    ye = (base.astype(np.float32) + v.astype(np.float32)).astype(np.float64)
    y = rn(ye, dt)
    st = {"max": float(max(np.abs(a).max() for a in (te, ue, pe, ye)))}
    assert np.isfinite(st["max"]), "a probe must not overflow"
    for name, exact, rounded in (("t", te, t), ("u", ue, u), ("v", pe, v), ("y", ye, y)):
        st[name + "_numel"] = int(exact.size)
        st[name + "_inexact"] = int((exact != rounded).sum())
        st[name + "_ties"] = int(((rn(exact, dt, "zero") != rn(exact, dt, "away")) &
                                  (np.abs(exact - rn(exact, dt, "zero")) == np.abs(rn(exact, dt, "away") - exact))).sum())
    return st


def overflow_case(M=33, K=384, r=24, N=80, scale=1.5, seed=0, cap=CAP):
    """The exact overflow probe (fp16), in place of a ``huge`` activation row, where a float64 chain
    cannot say at which element rn(t) overflows: ``rounding_inputs`` with x and A so large that some
    exact t exceed 65520 and must become infinity, while every finite sum stays exact.  u, v and y
    follow elementwise by the header's chain: inf * 0 = NaN where B is zero, the infinity where all
    infinite terms agree in sign, NaN where they do not.  Returns (x, A, B, base, y_want, v_want)."""
    dt = "f16"
    x, A, B, base = rounding_inputs(M, K, r, N, dt, seed, overflow=True)
    y, v = chain16(x, A, B, base, scale, dt, cap=cap)
    t = rn(_dot(x, A), dt)
    assert 8 <= int(np.isinf(t).sum()) < t.size // 2 and np.abs(_dot(x, A)).max() < 2.0 ** 20, "some t overflow, most do not"
    for z in (y, v):
        assert np.isnan(z).any() and np.isinf(z).any() and np.isfinite(z).mean() > 0.25, "NaN, infinities and finite outputs"
    assert (np.isposinf(y).any() and np.isneginf(y).any())
    return tuple(to16(a, dt) for a in (x, A, B, base, y, v))


def same_bits_or_nan(got, want):
    """Mask of the elements of two 16-bit tensors that agree: the same bits, or NaN where NaN is due."""
    g, w = got.view(torch.int16), want.view(torch.int16)
    return torch.where(torch.isnan(want), torch.isnan(got), g == w)


# ---- special rows of x: a float64 reference by elementwise product and sum, judged by class ------------
def _dot_t(a, b):
    return (a[:, None, :] * b[None, :, :]).sum(-1)


def lora_oracle_rows(x, A, B, scale, dt, base=None):
    """``lora_oracle`` with both products formed elementwise (``_dot``'s reason), for inputs with
    NaN, infinities and zero rows: (y_ref, by) in float64 on the inputs' device.  A row of x that
    holds a NaN or an infinity has a NaN or infinite reference and a meaningless bound."""
    p, sub = P_SUB[dt]
    e = 1.0 + 2.0 ** -p
    s = f32(scale)
    xf, Af, Bf = x.double(), A.double(), B.double()
    t = _dot_t(xf, Af)
    bt = tol_t(t, _dot_t(xf.abs(), Af.abs()), dt)
    u = _dot_t(t, Bf)
    bu = _dot_t(bt, Bf.abs()) * e + tol_t(u, _dot_t(t.abs() + bt, Bf.abs()), dt)
    v = u * s
    bv = bu * abs(s) * e + 2.0 ** -p * v.abs() + sub
    if base is None:
        return v, bv
    y = base.double() + v
    return y, bv * e + 2.0 ** -p * y.abs() + sub


SPECIAL = {"bf16": (("nan", "pinf", "ninf"), ("zero", "negzero", "small")),
           "f16": (("nan", "pinf", "ninf"), ("zero", "negzero", "tiny"))}
_NAN_BITS = {"bf16": 0x7FC0, "f16": 0x7E00}
_INF_BITS = {"bf16": 0x7F80, "f16": 0x7C00}


def special_kind_sets(M, dt):
    """The kinds of one call: each group of SPECIAL at once, or one kind at a time at M = 1."""
    return [(k,) for g in SPECIAL[dt] for k in g] if M == 1 else list(SPECIAL[dt])


def special_case(M, K, r, N, dt, kinds, a_col="nonzero", seed=0):
    """(x_special, x_plain, A, B, base, rows): ``drawn_case`` with the rows ``_activation_cases.positions``
    names replaced, kind by kind as _activation_cases.py describes them (``huge`` is ``overflow_case``'s).
    An infinity sits at one column k0.  A is drawn with a quarter of its entries zero;
    ``a_col`` = "mixed" leaves zeros and non-zeros in column k0, so that t has NaN beside infinities
    and, B being dense, every output of the row is NaN; "nonzero" makes the column non-zero, so that
    every t of the row is an infinity, and gives the first half of B's rows the signs of that column:
    their outputs are the infinity, the others -- sums of infinities of both signs -- mostly NaN."""
    from _activation_cases import positions

    assert a_col in ("nonzero", "mixed")
    x, A, B, base = drawn_case(M, K, r, N, dt, seed)
    g = torch.Generator().manual_seed(4099 * seed + 131 * M + 17 * K + 7 * r + N)
    A = torch.where(torch.rand(r, K, generator=g) < 0.25, torch.zeros((), dtype=A.dtype), A)
    k0 = int(torch.randint(0, K, (1,), generator=g))
    col = A[:, k0].float()
    if a_col == "mixed":
        col[0] = 0.0
        col[r - 1] = col[r - 1] if float(col[r - 1]) != 0 else 0.125
        assert bool((col == 0).any()) and bool((col != 0).any())
    else:
        col = torch.where(col == 0, torch.full_like(col, 0.125), col)
    A[:, k0] = col.to(A.dtype)
    B = torch.where(B == 0, torch.full_like(B, 0.25), B)                       # dense and non-zero
    if a_col == "nonzero":
        half = N // 2
        B[:half] = (B[:half].float().abs() * torch.sign(col)[None, :]).to(B.dtype)
    assert bool((B != 0).all()) and bool(torch.isfinite(A.float()).all())
    xs = x.clone()
    bits = xs.view(torch.int16)
    rows = dict(zip(positions(M, len(kinds)), kinds))
    for row, kind in rows.items():
        if kind == "nan":
            bits[row, int(torch.randint(0, K, (1,), generator=g))] = _NAN_BITS[dt]
        elif kind in ("pinf", "ninf"):
            bits[row, k0] = _INF_BITS[dt] if kind == "pinf" else (_INF_BITS[dt] | 0x8000) - 0x10000  # as int16
        elif kind == "zero":
            bits[row] = 0
        elif kind == "negzero":
            bits[row] = -0x8000
        elif kind == "tiny":
            assert dt == "f16"
            xs[row] = (x[row].double() * 2.0 ** -16).to(xs.dtype)
            assert float(((xs[row].float().abs() < 2.0 ** -14) & (xs[row] != 0)).float().mean()) > 0.5  # mostly subnormal
        elif kind == "small":
            assert dt == "bf16"
            xs[row] = (x[row].double() * 2.0 ** -100).to(xs.dtype)
            assert torch.equal(xs[row].double(), x[row].double() * 2.0 ** -100)  # exact
        else:
            raise ValueError(kind)
    return xs, x, A, B, base, rows


def class_ok(got, ref, bound):
    """Mask: a NaN reference needs NaN, an infinite one the same infinity, a finite one a value
    within the bound (so a NaN or an infinity where a finite value is due fails too)."""
    g = got.double()
    same_inf = torch.isinf(g) & (torch.sign(g) == torch.sign(ref))
    close = (g - ref).abs() <= bound
    return torch.where(torch.isnan(ref), torch.isnan(g), torch.where(torch.isinf(ref), same_inf, close))


def check_classes(got, ref, bound, what=""):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    ok = class_ok(got, ref, bound)
    if not bool(ok.all()):
        g = got.double()
        bad = (~ok).nonzero()
        m, n = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} outputs of the wrong class or outside the bound "
                             f"({int(torch.isnan(g).sum())} NaN, {int(torch.isinf(g).sum())} inf; reference "
                             f"{int(torch.isnan(ref).sum())} NaN, {int(torch.isinf(ref).sum())} inf), rows "
                             f"{sorted(set(bad[:, 0].tolist()))[:8]}; first at ({m}, {n}): got {float(g[m, n])!r} "
                             f"reference {float(ref[m, n])!r}")


__all__ = ["BREAKS", "CAP", "TDT", "chain16", "check", "check_classes", "class_ok", "drawn_case", "exact_case", "f32",
           "gemm_tol", "lora_oracle", "lora_oracle_rows", "outside", "overflow_case", "premise", "rn", "rounding_case",
           "rounding_inputs", "rounding_stats", "same_bits_or_nan", "to16", "tol_t", "torch_chain", "widen", "worst_ratio"]
