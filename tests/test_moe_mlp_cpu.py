"""``nf4_moe_swiglu_bnb`` and ``nf4_moe_mlp_bnb`` with CPU tensors (no GPU): the composite route.

On CPU tensors ``nf4_moe_swiglu_bnb`` is ``F.silu(nf4_moe_linear_bnb(x, w1, ids)) *
nf4_moe_linear_bnb(x, w3, ids)``, and that is the per-expert loop over ``nf4_linear_bnb``.
``dequantize_nf4_bnb`` has no host form, so -- as in test_moe_cpu.py, whose fixtures these are --
the C oracle's dequantization stands in its place, for the function and for the expected rows
alike: what is checked is the definition, pair by pair and bit for bit, with no tolerance."""
import pytest
import torch
import torch.nn.functional as F

import nf4_triton_dequantization_amd as P
from nf4_triton_dequantization_amd import (Experts4bit, kernel, nf4_linear_bnb, nf4_moe_linear_bnb, nf4_moe_mlp_bnb,
                                           nf4_moe_swiglu_bnb)
from test_moe_cpu import cpu_backend, oracle_dequant  # noqa: F401  (fixtures)

E, I, K = 4, 64, 256


def _weights(seed, n=I, k=K, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    # every expert on its own scale, so that absmax2 groups and offsets differ between experts
    return torch.stack([torch.randn(n, k, generator=g) * (0.02 * (e + 1)) for e in range(E)]).to(dtype)


def _stacks(nested=True):
    return (Experts4bit.from_float(_weights(11), compress_statistics=nested),
            Experts4bit.from_float(_weights(12), compress_statistics=nested))


def test_both_functions_are_exported():
    for name in ("nf4_moe_swiglu_bnb", "nf4_moe_mlp_bnb"):
        assert name in P.__all__ and getattr(P, name) is getattr(kernel, name)
    assert isinstance(kernel.MOE_SWIGLU_ROUTED_MIN_P, int) and isinstance(kernel.MOE_SWIGLU_ROUTED_MAX_P, int)
    assert kernel.MOE_SWIGLU_ROUTED_MAX_P <= 128  # NF4DQ_MOE_MAX_PAIRS: one launch holds no more


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("per_pair", [False, True])
def test_swiglu_is_the_per_pair_loop_bit_for_bit(cpu_backend, oracle_dequant, nested, ids_dtype, per_pair):  # noqa: F811
    """x [T, K] (shared by the token's choices) and [T, k, K]; ids outside 0..E-1 (-1 and E) give
    rows of zeros; one token names the same expert twice; expert 3 stays idle; ``out=``."""
    T, k = 5, 2
    w1, w3 = _stacks(nested)
    ids = torch.tensor([[0, 1], [2, 2], [-1, 0], [1, E], [2, 0]], dtype=ids_dtype)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((T, k, K) if per_pair else (T, K), generator=g).to(torch.bfloat16)
    h = nf4_moe_swiglu_bnb(x, w1, w3, ids)
    assert tuple(h.shape) == (T, k, I) and h.dtype == torch.bfloat16
    for t in range(T):
        for j in range(k):
            e = int(ids[t, j])
            row = (x[t, j] if per_pair else x[t])[None]
            if 0 <= e < E:
                want = (F.silu(nf4_linear_bnb(row, w1.expert(e))) * nf4_linear_bnb(row, w3.expert(e)))[0]
                assert bool(want.abs().sum() > 0)
            else:
                want = torch.zeros(I, dtype=torch.bfloat16)
            assert torch.equal(h[t, j], want), (t, j, e)
    assert torch.equal(h, F.silu(nf4_moe_linear_bnb(x, w1, ids)) * nf4_moe_linear_bnb(x, w3, ids))
    assert not torch.equal(h, nf4_moe_swiglu_bnb(x, w3, w1, ids))     # gate and up are not interchangeable
    out = torch.full((T, k, I), float("nan"), dtype=torch.bfloat16)
    assert nf4_moe_swiglu_bnb(x, w1, w3, ids, out=out) is out and torch.equal(out, h)


def test_mismatched_stacks_and_bad_arguments_raise(cpu_backend):  # noqa: F811
    w1, w3 = _stacks()
    ids = torch.zeros((3, 2), dtype=torch.int64)
    x = torch.zeros(3, K, dtype=torch.bfloat16)
    others = (Experts4bit.from_float(_weights(13, n=128)),                       # another I
              Experts4bit.from_float(_weights(13, k=128)),                       # another K
              Experts4bit.from_float(_weights(13)[:2]),                          # another expert count
              Experts4bit.from_float(_weights(13, dtype=torch.float16)),         # another dtype
              Experts4bit.from_float(_weights(13), compress_statistics=False))   # fp32 statistics beside nested
    for other in others:
        with pytest.raises(ValueError):
            nf4_moe_swiglu_bnb(x, w1, other, ids)
        with pytest.raises(ValueError):
            nf4_moe_swiglu_bnb(torch.zeros(3, other.in_features, dtype=torch.bfloat16), other, w3, ids)
    # nf4_moe_linear_bnb's own checks, with its errors
    with pytest.raises(RuntimeError):
        nf4_moe_swiglu_bnb(torch.zeros(3, K + 1), w1, w3, ids)
    with pytest.raises(RuntimeError):
        nf4_moe_swiglu_bnb(torch.zeros(3, 3, K), w1, w3, ids)
    with pytest.raises(ValueError):
        nf4_moe_swiglu_bnb(x, w1, w3, ids.float())
    with pytest.raises(ValueError):
        nf4_moe_swiglu_bnb(x, w1, w3, ids.reshape(-1))
    with pytest.raises(ValueError):
        nf4_moe_swiglu_bnb(x, w1, w3, ids, out=torch.zeros(3, 2, I))  # fp32 out, bf16 experts
    with pytest.raises(ValueError):
        nf4_moe_swiglu_bnb(x, w1, w3, ids, out=torch.zeros(3, 2, I + 64, dtype=torch.bfloat16))
    empty = nf4_moe_swiglu_bnb(torch.zeros(0, K), w1, w3, ids[:0])
    assert tuple(empty.shape) == (0, 2, I)


@pytest.mark.parametrize("nested", [True, False])
def test_mlp_is_its_three_line_expression(cpu_backend, oracle_dequant, nested):  # noqa: F811
    H, T, k = K, 6, 2
    w1, w3 = _stacks(nested)
    w2 = Experts4bit.from_float(_weights(14, n=H, k=I), compress_statistics=nested)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    ids = torch.tensor([[0, 1], [2, 2], [-1, 0], [1, E], [3, 0], [1, 2]])
    for rw_dtype in (torch.float32, torch.bfloat16, torch.float64):
        rw = torch.rand(T, k, generator=g).to(rw_dtype)
        y = nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw)
        h = nf4_moe_swiglu_bnb(x, w1, w3, ids)
        d = nf4_moe_linear_bnb(h, w2, ids)
        want = (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1)
        assert tuple(y.shape) == (T, H) and y.dtype == torch.bfloat16 and torch.equal(y, want)
        assert bool(y.abs().sum() > 0)
    # a token whose two ids are both invalid gets a row of zeros
    ids2 = ids.clone()
    ids2[0] = torch.tensor([-1, E])
    assert bool((nf4_moe_mlp_bnb(x, w1, w3, w2, ids2, rw)[0] == 0).all())


def test_backward_reaches_x(cpu_backend, oracle_dequant):  # noqa: F811
    w1, w3 = _stacks()
    w2 = Experts4bit.from_float(_weights(14, n=K, k=I))
    ids = torch.tensor([[0, 3], [1, 1]])
    x = torch.randn(2, K, requires_grad=True)
    h = nf4_moe_swiglu_bnb(x, w1, w3, ids)
    assert h.requires_grad
    h.float().sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and bool((x.grad.abs().sum(1) > 0).all())
    # the gradient is the composite's own
    x2 = x.detach().clone().requires_grad_(True)
    (F.silu(nf4_moe_linear_bnb(x2, w1, ids)) * nf4_moe_linear_bnb(x2, w3, ids)).float().sum().backward()
    assert torch.equal(x.grad, x2.grad)
    x3 = x.detach().clone().requires_grad_(True)
    y = nf4_moe_mlp_bnb(x3, w1, w3, w2, ids, torch.tensor([[0.7, 0.3], [0.5, 0.5]]))
    assert y.requires_grad
    y.float().sum().backward()
    assert x3.grad is not None and bool((x3.grad.abs().sum(1) > 0).all())
