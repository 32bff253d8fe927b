"""``nf4_linear_lora_bnb``, ``nf4_linear_lora_bnb_grouped`` and ``LoraLinear4bit`` with CPU tensors
(no GPU): the composite route, which is also the functions' definition,

    y = nf4_linear_bnb(x, module, bias); t = F.linear(x.to(A.dtype), A); u = F.linear(t, B)
    y + (u * scaling).to(y.dtype)

and must be met bit for bit.  ``dequantize_nf4_bnb`` has no host form, so -- as test_swiglu_cpu.py
does -- the tests put the C oracle's dequantization in its place, for the function under test and
for the expected value alike."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nf4_oracle as O
import nf4_triton_dequantization_amd as P
from nf4_triton_dequantization_amd import Linear4bit, LoraLinear4bit, kernel, nf4_linear_bnb, nf4_linear_bnb_grouped

N, K = 192, 256


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


def _module(dtype, n=N, seed=0, bias=False):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, K, generator=g) * 0.05
    b = torch.randn(n, generator=g) if bias else None
    return Linear4bit.from_float(w, compute_dtype=dtype, bias=b)


def _adapter(dtype, n=N, r=16, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return (torch.randn(r, K, generator=g) / K ** 0.5).to(dtype), (torch.randn(n, r, generator=g) / r ** 0.5).to(dtype)


def _composite(x, module, A, B, scaling, bias=None):
    y = nf4_linear_bnb(x, module, bias)
    t = F.linear(x.to(A.dtype), A)
    u = F.linear(t, B)
    return y + (u * scaling).to(y.dtype)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_package_exports():
    for name in ("nf4_linear_lora_bnb", "nf4_linear_lora_bnb_grouped", "LoraLinear4bit"):
        assert name in P.__all__ and hasattr(P, name), name
    assert isinstance(kernel.LORA_ROUTED_MIN_M, int) and isinstance(kernel.LORA_ROUTED_MAX_M, int)
    assert kernel.LORA_ROUTED_MAX_M <= 128


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bias", [False, True])
def test_cpu_tensors_equal_the_composite_bit_for_bit(dtype, bias):
    mod = _module(dtype, bias=bias)
    A, B = _adapter(dtype)
    x = torch.randn(2, 5, K, generator=torch.Generator().manual_seed(1)).to(dtype)
    with torch.no_grad():
        want = _composite(x, mod, A, B, 0.75, mod.bias)
        y = P.nf4_linear_lora_bnb(x, mod, A, B, 0.75, mod.bias)
        assert y.shape == (2, 5, N) and _same_bits(y, want)
        assert not torch.equal(y, nf4_linear_bnb(x, mod, mod.bias))  # the adapter is in
        assert _same_bits(P.nf4_linear_lora_bnb(x, mod, A, B, 0.0, mod.bias), _composite(x, mod, A, B, 0.0, mod.bias))


def test_grouped_equals_the_composite_per_module():
    dtype = torch.bfloat16
    mods = [_module(dtype, n, seed=s, bias=(s == 1)) for s, n in enumerate((192, 64, 128))]
    ads = [(*_adapter(dtype, 192, 16, 0), 0.5), None, (*_adapter(dtype, 128, 64, 2), -2.0)]
    biases = [m.bias for m in mods]
    x = torch.randn(7, K, generator=torch.Generator().manual_seed(2)).to(dtype)
    with torch.no_grad():
        ys = P.nf4_linear_lora_bnb_grouped(x, mods, ads, biases)
        base = nf4_linear_bnb_grouped(x, mods, biases)
        assert len(ys) == 3
        for y, b, mod, ad in zip(ys, base, mods, ads):
            want = b if ad is None else _composite(x, mod, ad[0], ad[1], ad[2], mod.bias)
            assert _same_bits(y, want)
        assert P.nf4_linear_lora_bnb_grouped(x, [], []) == []
    with pytest.raises(ValueError):
        P.nf4_linear_lora_bnb_grouped(x, mods, ads[:2])


def test_module_names_initialisation_and_forward():
    dtype = torch.bfloat16
    base = _module(dtype, bias=True)
    m = LoraLinear4bit.from_linear4bit(base, r=16, lora_alpha=32)
    assert m.base_layer is base and m.scaling == 2.0 and m.r == 16
    names = dict(m.named_parameters())
    assert {"lora_A.weight", "lora_B.weight"} <= set(names) and "lora_A.bias" not in names and "lora_B.bias" not in names
    assert tuple(m.lora_A.weight.shape) == (16, K) and tuple(m.lora_B.weight.shape) == (N, 16)
    assert m.lora_A.weight.dtype == dtype and m.lora_B.weight.dtype == dtype
    assert bool((m.lora_A.weight != 0).any()) and not bool((m.lora_B.weight != 0).any())
    bound = 1.0 / K ** 0.5                                   # kaiming-uniform with a = sqrt(5)
    assert float(m.lora_A.weight.detach().float().abs().max()) <= bound * (1 + 2.0 ** -8)
    assert "dropout" in LoraLinear4bit.__doc__.lower()
    x = torch.randn(3, K, generator=torch.Generator().manual_seed(3)).to(dtype)
    with torch.no_grad():
        assert _same_bits(m(x), base(x))                     # zero delta at initialisation
        A, B = _adapter(dtype, seed=5)
        # an adapter state dict in PEFT's names loads once its prefix is stripped
        m.load_state_dict({"lora_A.weight": A, "lora_B.weight": B}, strict=False)
        assert _same_bits(m(x), _composite(x, base, A, B, 2.0, base.bias))
    assert LoraLinear4bit.from_linear4bit(base, 8, 16, dtype=torch.float32).lora_A.weight.dtype == torch.float32


def test_fp32_adapter_and_requires_grad_take_the_composite_with_gradients(monkeypatch):
    monkeypatch.setattr(kernel, "LORA_ROUTED_MIN_M", 1)      # even a routed range does not change this
    monkeypatch.setattr(kernel, "LORA_ROUTED_MAX_M", 128)
    monkeypatch.setattr(kernel, "_lora_add", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fused")))
    dtype = torch.bfloat16
    mod = _module(dtype)
    x = torch.randn(4, K, generator=torch.Generator().manual_seed(4)).to(dtype)
    A, B = (t.float().requires_grad_() for t in _adapter(dtype))
    y = P.nf4_linear_lora_bnb(x, mod, A, B, 0.5)
    assert y.dtype == dtype and y.grad_fn is not None
    assert _same_bits(y.detach(), _composite(x, mod, A.detach(), B.detach(), 0.5))
    y.float().sum().backward()
    for t in (A, B):
        assert t.grad is not None and t.grad.shape == t.shape and bool(t.grad.abs().sum() > 0)
    m = LoraLinear4bit.from_linear4bit(mod, 8, 16)
    torch.nn.init.normal_(m.lora_B.weight, std=0.1)
    m(x).float().sum().backward()
    assert m.lora_A.weight.grad is not None and m.lora_B.weight.grad is not None
