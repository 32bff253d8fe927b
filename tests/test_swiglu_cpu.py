"""``nf4_swiglu_bnb`` and ``nf4_mlp_bnb`` with CPU tensors (no GPU): the fallback route.

On CPU tensors ``nf4_swiglu_bnb`` is ``F.silu(g) * u`` with
``g, u = nf4_linear_bnb_grouped(x, [gate_proj, up_proj], biases)`` and must equal that expression
bit for bit; ``nf4_mlp_bnb`` is ``nf4_linear_bnb(nf4_swiglu_bnb(...), down_proj)`` and nothing
else.  ``dequantize_nf4_bnb`` has no host form, so -- as test_moe_cpu.py does -- the tests put the
C oracle's dequantization in its place, for the function under test and for the expected value
alike."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nf4_oracle as O
from nf4_triton_dequantization_amd import (Linear4bit, kernel, nf4_linear_bnb, nf4_linear_bnb_grouped, nf4_mlp_bnb,
                                           nf4_swiglu_bnb)

I, K, H = 192, 256, 128  # gate / up are [I, K], down is [H, I]


@pytest.fixture(autouse=True)
def cpu_backend(monkeypatch):
    monkeypatch.setenv("NF4_BACKEND", "cpu")


@pytest.fixture(autouse=True)
def oracle_dequant(monkeypatch, coracle):
    """kernel.dequantize_nf4_bnb := the C oracle on the module's host tensors."""
    def dequant(module):
        qs = module.weight.quant_state
        n, k = int(module.out_features), int(module.in_features)
        code = O.BF16 if qs.dtype == torch.bfloat16 else O.F16
        q = module.weight.data.reshape(-1).numpy()
        if qs.state2 is not None:
            bits = coracle.dequant_bnb(q, qs.absmax.numpy(), qs.state2.code.numpy(), qs.state2.absmax.numpy(),
                                       float(qs.offset), n * k, code, 64, int(qs.state2.blocksize))
        else:
            bits = coracle.dequant_bnb_single(q, qs.absmax.numpy(), n * k, code, 64)
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(qs.dtype).reshape(n, k)

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", dequant)


def _mlp(dtype, nested, seed=0, bias=False):
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i, (n, k) in enumerate(((I, K), (I, K), (H, I))):
        w = torch.randn(n, k, generator=g) * (0.05 * (i + 1))
        b = torch.randn(n, generator=g) if bias else None
        mods.append(Linear4bit.from_float(w, compute_dtype=dtype, bias=b, compress_statistics=nested))
    return mods


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [True, False])
def test_cpu_tensors_equal_the_fallback_expression_bit_for_bit(dtype, nested):
    gate, up, down = _mlp(dtype, nested)
    x = (torch.randn(2, 5, K, generator=torch.Generator().manual_seed(1)) * 2).to(dtype)
    with torch.no_grad():
        g, u = nf4_linear_bnb_grouped(x, [gate, up], [None, None])
        want = F.silu(g) * u
        h = nf4_swiglu_bnb(x, gate, up)
        assert h.shape == (2, 5, I) and h.dtype == dtype
        assert torch.equal(h.view(torch.int16), want.view(torch.int16))
        # the weights are not interchangeable
        assert not torch.equal(nf4_swiglu_bnb(x, up, gate), h)
        y = nf4_mlp_bnb(x, gate, up, down)
        assert y.shape == (2, 5, H)
        assert torch.equal(y.view(torch.int16), nf4_linear_bnb(want, down).view(torch.int16))
        out = torch.full((2, 5, I), float("nan"), dtype=dtype)
        assert nf4_swiglu_bnb(x, gate, up, out=out) is out
        assert torch.equal(out.view(torch.int16), want.view(torch.int16))


def test_biases_ride_the_fallback():
    gate, up, _ = _mlp(torch.bfloat16, True, seed=3, bias=True)
    x = torch.randn(7, K, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    with torch.no_grad():
        g, u = nf4_linear_bnb_grouped(x, [gate, up], [gate.bias, up.bias])
        assert not torch.equal(g, nf4_linear_bnb(x, gate))  # the bias is in
        assert torch.equal(nf4_swiglu_bnb(x, gate, up), F.silu(g) * u)


def test_mismatched_shapes_raise():
    gate, up, down = _mlp(torch.bfloat16, True)
    x = torch.zeros(3, K, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        nf4_swiglu_bnb(torch.zeros(3, K + 1, dtype=torch.bfloat16), gate, up)
    with pytest.raises(RuntimeError):
        nf4_swiglu_bnb(torch.zeros(3, I, dtype=torch.bfloat16), gate, down)   # up_proj of another shape
    with pytest.raises(RuntimeError):
        nf4_swiglu_bnb(x, down, up)
    with pytest.raises(ValueError):
        nf4_swiglu_bnb(x, gate, up, out=torch.zeros(3, I + 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        nf4_swiglu_bnb(x, gate, up, out=torch.zeros(3, I))                    # fp32 out, bf16 modules
    with pytest.raises(RuntimeError):
        nf4_mlp_bnb(x, gate, up, gate)                                        # down_proj must take I features


@pytest.mark.parametrize("dt,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_the_acceptance_set_holds_torchs_cpu_chain_and_little_else(dt, dtype):
    """_swiglu_cases.accept, which judges the GPU results: torch's CPU chain on 2^16 N(0, 2) draws
    (and on every 16-bit g in [-40, 40] against one u) lies in the set with few near-tie elements;
    an h one 16-bit step off, a chain with g and u swapped, and a silu rounded only once (the
    product taken from the unrounded silu) do not."""
    from _swiglu_cases import accept, rn16, silu64, to_bits
    from _gemm_cases import bits_to_f64

    gen = torch.Generator().manual_seed(7)
    g = (torch.randn(1 << 16, generator=gen) * 2).to(dtype)
    u = (torch.randn(1 << 16, generator=gen) * 2).to(dtype)
    bits = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)
    h = F.silu(g) * u
    frac = accept(bits(h), bits(g), bits(u), dt, "torch cpu chain")
    assert frac < 0.004
    allg = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(dtype)
    allg = allg[torch.isfinite(allg.float()) & (allg.float().abs() <= 40)]
    for uv in (1.0, -0.3330078125, 3.0):
        uu = torch.full_like(allg, uv)
        accept(bits(F.silu(allg) * uu), bits(allg), bits(uu), dt, f"every g, u = {uv}")
    with pytest.raises(AssertionError):
        accept(bits(h) ^ np.uint16(1), bits(g), bits(u), dt)
    with pytest.raises(AssertionError):
        accept(bits(F.silu(u) * g), bits(g), bits(u), dt)
    once = to_bits(rn16(silu64(bits_to_f64(bits(g), dt)) * bits_to_f64(bits(u), dt), dt), dt)
    assert (once != bits(h)).mean() > 0.05
    with pytest.raises(AssertionError):
        accept(once, bits(g), bits(u), dt)


@pytest.mark.parametrize("dt,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_the_acceptance_set_follows_the_fp32_chain_over_the_whole_16_bit_domain(dt, dtype):
    """Past -g = ln(FLT_MAX) = 88.72 the chain's fp32 ``expf`` is +inf and s = g / inf = -0; a
    float64 silu is still a 16-bit subnormal there in bf16.  torch's CPU chain ``F.silu(g) * u`` on
    every bf16 g in [-110, -80] and [80, 110], every fp16 g in [-20, -15] (s leaves the fp16 grid),
    +-65504 (the fp16 max; bf16's nearest), +-inf and NaN, each with u from {0, -0, 1, -3, max,
    inf, NaN}: all in the acceptance set, non-finite ones by class.  Without the flag a non-finite
    g or u is refused as before, and a -0 past the overflow is required, not merely allowed."""
    from _swiglu_cases import accept, allowed_s
    from _gemm_cases import bits_to_f64

    bits = lambda t: t.contiguous().view(torch.int16).numpy().view(np.uint16)
    allg = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(dtype)
    gf = allg.float()
    if dt == "bf16":
        grid = allg[((gf >= -110) & (gf <= -80)) | ((gf >= 80) & (gf <= 110))]
        assert grid.numel() == 2 * 61              # spacing 0.5 over [80, 110], both signs
    else:
        grid = allg[(gf >= -20) & (gf <= -15)]
        assert grid.numel() == 128 + 257           # spacing 2^-7 over [15, 16), 2^-6 over [16, 20]
    edge = torch.tensor([65504.0, -65504.0, float("inf"), float("-inf"), float("nan")]).to(dtype)
    gs = torch.cat([grid, edge])
    fmax = torch.finfo(dtype).max
    for uv in (0.0, -0.0, 1.0, -3.0, fmax, float("inf"), float("nan")):
        uu = torch.full_like(gs, uv)
        h = F.silu(gs) * uu
        frac = accept(bits(h), bits(gs), bits(uu), dt, f"{dt} u = {uv}", nonfinite=True)
        assert frac <= 0.01
        if np.isfinite(uv):
            accept(bits(F.silu(grid) * uu[:grid.numel()]), bits(grid), bits(uu[:grid.numel()]), dt, f"{dt} finite, u = {uv}")
            with pytest.raises(AssertionError, match="non-finite g or u"):
                accept(bits(h), bits(gs), bits(uu), dt, "no flag")
    if dt == "bf16":  # the overflow itself: -88.5 keeps a nonzero s, -89.0 and everything below is -0
        probe = torch.tensor([-88.5, -89.0, -90.0, -95.0, -104.0, -110.0]).to(dtype)
        sa, sb, near = allowed_s(bits(probe), dt)
        assert not near.any() and sa[0] < 0 and (sa[1:] == 0).all() and np.signbit(sa[1:]).all()
        assert (bits(F.silu(probe))[1:] == 0x8000).all() and bits(F.silu(probe))[0] != 0x8000
        one = torch.ones_like(probe)
        with pytest.raises(AssertionError):  # the float64 silu's subnormal where the chain gives -0
            accept(np.array([0x8287], np.uint16), bits(probe[1:2]), bits(one[1:2]), dt)
    # classes: silu(+inf) = +inf, silu(-inf) = NaN, inf * 0 = NaN; a wrong class is refused
    g3 = torch.tensor([float("inf"), float("-inf"), float("inf")]).to(dtype)
    u3 = torch.tensor([2.0, 2.0, 0.0]).to(dtype)
    want = F.silu(g3) * u3
    assert bool(torch.isinf(want[0])) and bool(torch.isnan(want[1])) and bool(torch.isnan(want[2]))
    accept(bits(want), bits(g3), bits(u3), dt, "classes", nonfinite=True)
    for wrong in ([0.0, float("nan"), float("nan")], [float("inf"), float("-inf"), float("nan")],
                  [float("inf"), float("nan"), 0.0], [float("-inf"), float("nan"), float("nan")]):
        with pytest.raises(AssertionError):
            accept(bits(torch.tensor(wrong).to(dtype)), bits(g3), bits(u3), dt, "wrong class", nonfinite=True)
    assert np.isfinite(bits_to_f64(bits(grid), dt)).all()


def test_backward_reaches_x():
    gate, up, down = _mlp(torch.bfloat16, True)
    x = torch.randn(4, K, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).requires_grad_()
    h = nf4_swiglu_bnb(x, gate, up)
    assert h.requires_grad and h.grad_fn is not None
    h.float().sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool(x.grad.float().abs().sum() > 0)
    x.grad = None
    nf4_mlp_bnb(x, gate, up, down).float().sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all()) and bool(x.grad.float().abs().sum() > 0)
