"""The judge of the adapter suites (tests/_lora_cases.py) tested where no GPU is needed: torch's
own fp32-accumulated chain on the host lies inside the bound at every element, two broken chains
-- one that drops the last 32 of K, one that drops the last rank index -- are caught in most
elements, ``tol_t`` is ``_gemm_cases.tol``, and the exact probes keep their premise."""
import numpy as np
import pytest
import torch

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
