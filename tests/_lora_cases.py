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


__all__ = ["TDT", "check", "drawn_case", "exact_case", "f32", "gemm_tol", "lora_oracle", "outside", "tol_t",
           "torch_chain", "worst_ratio"]
