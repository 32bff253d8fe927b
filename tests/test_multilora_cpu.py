"""``nf4_linear_multilora_bnb``, ``nf4_linear_multilora_bnb_grouped`` and ``MultiLoraLinear4bit`` with
CPU tensors (no GPU): the composite route, which is also the functions' definition.  Row by row it
must agree with ``nf4_linear_lora_bnb``'s composite for that row's adapter within ``lora_oracle``'s
bound (the two sum in different orders: bmm against linear), a row without an adapter is the base
bit for bit, and autograd reaches the stacks.  ``dequantize_nf4_bnb`` has no host form, so -- as
test_lora_cpu.py does -- the tests put the C oracle's dequantization in its place."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
import nf4_triton_dequantization_amd as P
from _lora_cases import check, lora_oracle
from nf4_triton_dequantization_amd import Linear4bit, LoraLinear4bit, MultiLoraLinear4bit, kernel, nf4_linear_bnb

N, K = 192, 256
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


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


def _stack(dtype, S, n=N, r=16, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    A = (torch.randn(S, r, K, generator=g) / K ** 0.5).to(dtype)
    B = (torch.randn(S, n, r, generator=g) / r ** 0.5).to(dtype)
    scaling = torch.tensor([0.5 + 0.25 * s for s in range(S)], dtype=torch.float32)
    return A, B, scaling


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def _judge(y, x, mod, A, B, scaling, ids, dt, bias=None):
    """Every row against the oracle of its own adapter over the base the function itself computes."""
    base = nf4_linear_bnb(x, mod, bias).reshape(-1, y.shape[-1])
    y2, x2 = y.reshape(-1, y.shape[-1]), x.reshape(-1, K)
    S = A.shape[0]
    for m, a in enumerate(ids.reshape(-1).tolist()):
        if 0 <= a < S:
            ref, bound = lora_oracle(x2[m:m + 1], A[a], B[a], float(scaling[a]), dt, base[m:m + 1])
            check(y2[m:m + 1], ref, bound, f"row {m} adapter {a}")
            single = P.nf4_linear_lora_bnb(x2[m:m + 1], mod, A[a], B[a], float(scaling[a]), bias)
            check(single, ref, bound, f"row {m} adapter {a}, nf4_linear_lora_bnb")       # the same judge holds both
        else:
            assert _same_bits(y2[m:m + 1], base[m:m + 1]), (m, a)


def test_package_exports():
    for name in ("nf4_linear_multilora_bnb", "nf4_linear_multilora_bnb_grouped", "MultiLoraLinear4bit"):
        assert name in P.__all__ and hasattr(P, name), name
    assert isinstance(kernel.MULTILORA_ROUTED_MIN_M, int) and isinstance(kernel.MULTILORA_ROUTED_MAX_M, int)
    assert kernel.MULTILORA_ROUTED_MAX_M <= 128
    assert P._lib.LORA_MAX_ADAPTERS == 64


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_rows_agree_with_the_single_adapter_composite(dt, idt):
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    mod = _module(dtype, bias=True)
    A, B, scaling = _stack(dtype, 5)
    x = torch.randn(3, 13, K, generator=torch.Generator().manual_seed(1)).to(dtype)      # 39 rows: two chunks
    ids = torch.randint(-1, 6, (3, 13), generator=torch.Generator().manual_seed(2)).to(idt)
    ids[0, 0], ids[0, 1] = INT32_MIN, INT32_MAX
    assert {-1, 0, 4, 5} <= set(ids.reshape(-1).tolist())
    with torch.no_grad():
        y = P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, ids, mod.bias)
        assert y.shape == (3, 13, N) and y.dtype == dtype
        _judge(y, x, mod, A, B, scaling, ids, dt, mod.bias)
        # a sequence of floats is the same scaling; flat ids are the same ids
        assert _same_bits(y, P.nf4_linear_multilora_bnb(x, mod, A, B, scaling.tolist(), ids.reshape(-1), mod.bias))


def test_no_adapter_rows_are_the_base_bit_for_bit_including_negative_zero(monkeypatch):
    dtype = torch.bfloat16
    mod = _module(dtype)
    A, B, scaling = _stack(dtype, 3)
    x = torch.randn(6, K, generator=torch.Generator().manual_seed(3)).to(dtype)
    base = nf4_linear_bnb(x, mod).clone()
    base[:, ::3] = -0.0
    base[:, 1::3] = 0.0
    assert bool((base.view(torch.int16) == -0x8000).any())
    monkeypatch.setattr(kernel, "nf4_linear_bnb", lambda x, module, bias=None: base.clone())
    for ids in ([-1] * 6, [3] * 6, [INT32_MIN, INT32_MAX, -1, 3, 64, -7]):
        for idt in (torch.int32, torch.int64):
            with torch.no_grad():
                y = P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, torch.tensor(ids, dtype=idt))
            assert _same_bits(y, base), ids
    with torch.no_grad():
        y = P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, torch.tensor([1, -1, 1, -1, 1, -1]))
    assert _same_bits(y[1::2], base[1::2]) and not torch.equal(y[0::2], base[0::2])
    big = torch.tensor([2 ** 32, 2 ** 32 + 1, -2 ** 32, 2 ** 40, 2 ** 33 + 2, -2 ** 63], dtype=torch.int64)
    with torch.no_grad():                                   # beyond 32 bits: still no adapter, never wrapped into range
        assert _same_bits(P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, big), base)
    assert kernel._multilora_ids32(big, 3).tolist() == [3, 3, -1, 3, 3, -1]


def test_grouped_equals_the_single_calls():
    dtype = torch.bfloat16
    mods = [_module(dtype, n, seed=s, bias=(s == 1)) for s, n in enumerate((192, 64, 128))]
    stacks = [_stack(dtype, 4, 192, 16, 0), None, _stack(dtype, 4, 128, 64, 2)]
    biases = [m.bias for m in mods]
    x = torch.randn(7, K, generator=torch.Generator().manual_seed(4)).to(dtype)
    ids = torch.tensor([0, 3, -1, 2, 2, 4, 1])
    with torch.no_grad():
        ys = P.nf4_linear_multilora_bnb_grouped(x, mods, stacks, ids, biases)
        assert len(ys) == 3
        for y, mod, st in zip(ys, mods, stacks):
            want = nf4_linear_bnb(x, mod, mod.bias) if st is None else P.nf4_linear_multilora_bnb(x, mod, *st, ids, mod.bias)
            assert _same_bits(y, want)
        assert P.nf4_linear_multilora_bnb_grouped(x, [], [], ids) == []
    with pytest.raises(ValueError, match="one stack"):
        P.nf4_linear_multilora_bnb_grouped(x, mods, stacks[:2], ids)


def test_module_stacking_padding_and_adapter_views():
    dtype = torch.bfloat16
    base = _module(dtype, bias=True)
    g = torch.Generator().manual_seed(5)
    ads = [((torch.randn(r, K, generator=g) / K ** 0.5).to(dtype), (torch.randn(N, r, generator=g) / r ** 0.5).to(dtype), sc)
           for r, sc in ((4, 2.0), (20, 0.5), (8, -1.0))]
    m = MultiLoraLinear4bit.from_linear4bit(base, ads)
    assert m.base_layer is base and m.num_adapters == 3 and m.r == 24 and m.ranks == [4, 20, 8]
    assert tuple(m.lora_A.shape) == (3, 24, K) and tuple(m.lora_B.shape) == (3, N, 24)
    assert m.lora_A.dtype == dtype and m.lora_B.dtype == dtype and not m.lora_A.requires_grad
    assert m.scaling.dtype == torch.float32 and m.scaling.tolist() == [2.0, 0.5, -1.0] and "scaling" in dict(m.named_buffers())
    assert {"lora_A", "lora_B"} <= set(dict(m.named_parameters()))
    for s, (A, B, _) in enumerate(ads):
        r = A.shape[0]
        assert torch.equal(m.lora_A[s, :r], A) and torch.equal(m.lora_B[s, :, :r], B)
        assert not bool(m.lora_A[s, r:].any()) and not bool(m.lora_B[s, :, r:].any())          # the padding is zeros
    x = torch.randn(2, 4, K, generator=torch.Generator().manual_seed(6)).to(dtype)
    ids = torch.tensor([[0, 1, 2, -1], [2, 2, 0, 3]])
    with torch.no_grad():
        y = m(x, ids)
        _judge(y, x, base, m.lora_A.detach(), m.lora_B.detach(), m.scaling, ids, "bf16", base.bias)
        for s in range(3):
            one = m.adapter(s)
            assert isinstance(one, LoraLinear4bit) and one.base_layer is base and one.r == ads[s][0].shape[0]
            assert one.scaling == ads[s][2] and torch.equal(one.lora_A.weight, ads[s][0]) and torch.equal(one.lora_B.weight, ads[s][1])
            assert one.lora_A.weight.data_ptr() == m.lora_A[s].data_ptr()                         # a view, not a copy
            rows = (ids.reshape(-1) == s).nonzero().reshape(-1)
            got, single = y.reshape(-1, N)[rows], one(x.reshape(-1, K)[rows])
            ref, bound = lora_oracle(x.reshape(-1, K)[rows], ads[s][0], ads[s][1], ads[s][2], "bf16",
                                     nf4_linear_bnb(x.reshape(-1, K)[rows], base, base.bias))
            check(got, ref, bound, f"adapter {s}")
            check(single, ref, bound, f"adapter({s})")
    with pytest.raises(IndexError):
        m.adapter(3)
    assert MultiLoraLinear4bit.from_linear4bit(base, ads, dtype=torch.float32).lora_A.dtype == torch.float32


def test_error_messages():
    dtype = torch.bfloat16
    mod = _module(dtype)
    A, B, scaling = _stack(dtype, 3)
    x = torch.randn(4, K).to(dtype)
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"lora_A must be \[S, r, K\]"):
        P.nf4_linear_multilora_bnb(x, mod, A[0], B[0], scaling, ids)
    with pytest.raises(ValueError, match="do not fit"):
        P.nf4_linear_multilora_bnb(x, mod, A, B[:, :64], scaling, ids)
    with pytest.raises(ValueError, match="do not fit"):
        P.nf4_linear_multilora_bnb(x, mod, A[:, :8], B, scaling, ids)
    with pytest.raises(ValueError, match="one value per adapter"):
        P.nf4_linear_multilora_bnb(x, mod, A, B, [1.0, 2.0], ids)
    with pytest.raises(ValueError, match="5 adapter ids for 4 rows"):
        P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(TypeError, match="int32 or int64"):
        P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, torch.zeros(4))
    with pytest.raises(ValueError, match="features"):
        P.nf4_linear_multilora_bnb(x[:, :128], mod, A, B, scaling, ids)
    with pytest.raises(ValueError, match="at least one adapter"):
        MultiLoraLinear4bit.from_linear4bit(mod, [])
    with pytest.raises(ValueError, match="adapter 1 must be"):
        MultiLoraLinear4bit.from_linear4bit(mod, [(A[0], B[0], 1.0), (A[1], B[1][:, :8], 1.0)])
    with pytest.raises(ValueError, match="MultiLoraLinear4bit: lora_A must be"):
        MultiLoraLinear4bit(mod, A, B[:2], scaling)
    with pytest.raises(ValueError, match="2 scalings for 3 adapters"):
        MultiLoraLinear4bit(mod, A, B, scaling[:2])


def test_autograd_reaches_the_stacks_through_the_composite(monkeypatch):
    monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MIN_M", 1)      # even a routed range does not change this
    monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MAX_M", 128)
    monkeypatch.setattr(kernel, "_multilora_add", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fused")))
    dtype = torch.bfloat16
    mod = _module(dtype)
    x = torch.randn(6, K, generator=torch.Generator().manual_seed(7)).to(dtype)
    A, B, scaling = _stack(dtype, 4)
    A, B = A.float().requires_grad_(), B.float().requires_grad_()
    ids = torch.tensor([0, 2, 2, -1, 0, 7])
    y = P.nf4_linear_multilora_bnb(x, mod, A, B, scaling, ids)
    assert y.dtype == dtype and y.grad_fn is not None
    y.float().sum().backward()
    for t in (A, B):
        assert t.grad is not None and t.grad.shape == t.shape
        assert bool(t.grad[0].abs().sum() > 0) and bool(t.grad[2].abs().sum() > 0)
        assert not bool(t.grad[1].any()) and not bool(t.grad[3].any())       # adapters no row names get no gradient
