"""``nf4_moe_down_bnb`` with CPU tensors (no GPU): the composite route -- ``nf4_moe_linear_bnb``'s
per-expert loop, the products in the 16-bit dtype, the ascending fp32 sum from +0 -- against the
documented chain on the host (_moe_down_cases.chain), bit for bit, at k = 1 .. 4; the chain against
torch's own three-line expression at k <= 2; -0, invalid ids, argument errors, empty input and the
export.  ``dequantize_nf4_bnb`` is the C oracle here, as in test_moe_cpu.py."""
import numpy as np
import pytest
import torch

import nf4_triton_dequantization_amd as pkg
from _moe_down_cases import chain
from nf4_triton_dequantization_amd import Experts4bit, kernel, nf4_moe_down_bnb, nf4_moe_linear_bnb, nf4_moe_mlp_bnb
from test_moe_cpu import E, K, N, _weights, cpu_backend, oracle_dequant  # noqa: F401  (fixtures)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _rw_np(rw, dtype):
    return rw.numpy() if rw.dtype == torch.float32 else _bits(rw.to(dtype))


@pytest.mark.parametrize("dtype,dt", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_composite_is_the_chain(cpu_backend, oracle_dequant, dtype, dt, k):  # noqa: F811
    T = 6
    ex = Experts4bit.from_float(_weights(6, dtype))
    g = torch.Generator().manual_seed(k)
    ids = torch.randint(0, E, (T, k), generator=g)
    ids[1, 0], ids[2, -1] = -1, E                       # invalid ids: rows of zeros in d
    h = torch.randn((T, k, K), generator=g).to(dtype)
    for rw_dtype in (torch.float32, dtype, torch.float64):
        rw = torch.rand((T, k), generator=g, dtype=torch.float64).to(rw_dtype)
        y = nf4_moe_down_bnb(h, ex, ids, rw)
        assert tuple(y.shape) == (T, N) and y.dtype == dtype
        d = nf4_moe_linear_bnb(h, ex, ids)
        want = chain(_bits(d).reshape(T * k, N), ids.numpy(), E, _rw_np(rw, dtype), k, dt)
        assert (_bits(y) == want).all(), (k, rw_dtype)
        if k <= 2:  # a sum of two fp32 terms is order-free: torch's expression, bit for bit
            assert torch.equal(y, (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1))
        out = torch.full((T, N), float("nan"), dtype=dtype)
        assert nf4_moe_down_bnb(h, ex, ids, rw, out=out) is out and torch.equal(out, y)
    if k == 2:  # x [T, K], shared by the token's choices
        y = nf4_moe_down_bnb(h[:, 0], ex, ids, rw)
        d = nf4_moe_linear_bnb(h[:, 0], ex, ids)
        assert (_bits(y) == chain(_bits(d).reshape(T * k, N), ids.numpy(), E, _rw_np(rw, dtype), k, dt)).all()


def test_minus_zero_invalid_ids_and_nan_weights(cpu_backend, oracle_dequant):  # noqa: F811
    """A token of invalid ids with weights -0.0: both products are -0, the sum from +0 is +0 bits --
    in the function, in the host chain and in torch's expression; a NaN weight on an invalid id gives
    NaN; a token of invalid ids with finite weights is a row of +0 bits."""
    ex = Experts4bit.from_float(_weights(7))
    ids = torch.tensor([[-1, E], [0, 1], [E, 2], [-5, E + 1]])
    rw = torch.tensor([[-0.0, -0.0], [-0.0, -0.0], [float("nan"), 0.5], [0.25, 0.75]])
    h = torch.randn((4, 2, K), generator=torch.Generator().manual_seed(8)).to(torch.bfloat16)
    y = nf4_moe_down_bnb(h, ex, ids, rw)
    d = nf4_moe_linear_bnb(h, ex, ids)
    assert (_bits(d[0]) == 0).all() and (_bits(d * rw.to(d.dtype).unsqueeze(-1))[0] == 0x8000).all()
    yb = _bits(y)
    assert (yb[0] == 0).all() and (yb[3] == 0).all() and ((yb[1] & 0x7FFF) == 0).all()
    assert bool(torch.isnan(y[2].float()).all()) and bool(torch.isfinite(y[[0, 1, 3]].float()).all())
    # (NaN as NaN: torch's host conversions to bf16 do not keep one NaN pattern)
    want = chain(_bits(d).reshape(8, N), ids.numpy(), E, rw.numpy(), 2, "bf16")
    assert (yb[[0, 1, 3]] == want[[0, 1, 3]]).all() and ((want[2] & 0x7FFF) > 0x7F80).all()
    assert torch.equal(y[[0, 1, 3]], (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1)[[0, 1, 3]])


def test_backward_reaches_h_and_the_weights(cpu_backend, oracle_dequant):  # noqa: F811
    ex = Experts4bit.from_float(_weights(9))
    ids = torch.tensor([[0, 3], [1, 1]])
    h = torch.randn(2, 2, K, requires_grad=True)
    rw = torch.rand(2, 2, requires_grad=True)
    y = nf4_moe_down_bnb(h, ex, ids, rw)
    assert y.requires_grad
    y.float().sum().backward()
    assert h.grad is not None and bool((h.grad.abs().sum(-1) > 0).all())
    assert rw.grad is not None and bool((rw.grad != 0).all())


def test_mlp_block_is_unchanged_at_k2_and_keeps_its_lines_beyond(cpu_backend, oracle_dequant):  # noqa: F811
    from nf4_triton_dequantization_amd import nf4_moe_swiglu_bnb

    assert kernel.MOE_DOWN_MLP_MAX_K == 2
    w1, w3 = (Experts4bit.from_float(_weights(s)[:, :, :N].contiguous().repeat(1, 4, 1)) for s in (10, 11))  # [E] x [256, 64]
    w2 = Experts4bit.from_float(_weights(12))                                                               # [E] x [64, 256]
    g = torch.Generator().manual_seed(13)
    for k in (1, 2, 3):
        ids = torch.randint(0, E, (5, k), generator=g)
        x = torch.randn((5, N), generator=g).to(torch.bfloat16)
        rw = torch.rand((5, k), generator=g)
        hh = nf4_moe_swiglu_bnb(x, w1, w3, ids)
        d = nf4_moe_linear_bnb(hh, w2, ids)
        assert torch.equal(nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw), (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1)), k


def test_argument_errors_empty_input_and_export(cpu_backend):  # noqa: F811
    assert "nf4_moe_down_bnb" in pkg.__all__ and pkg.nf4_moe_down_bnb is kernel.nf4_moe_down_bnb
    assert kernel.MOE_DOWN_ROUTED_MIN_P >= 1 and kernel.MOE_DOWN_ROUTED_MAX_P <= 128
    ex = Experts4bit.from_float(_weights(5))
    ids = torch.zeros((3, 2), dtype=torch.int64)
    rw = torch.ones(3, 2)
    h = torch.zeros(3, 2, K)
    with pytest.raises(RuntimeError):
        nf4_moe_down_bnb(torch.zeros(3, 2, K + 1), ex, ids, rw)
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, ex, ids.float(), rw)
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, ex, ids, torch.ones(3, 3))
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, ex, ids, torch.ones(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, ex, ids, rw, out=torch.zeros(3, N))            # fp32 out, bf16 experts
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, ex, ids, rw, out=torch.zeros(3, 2, N, dtype=torch.bfloat16))
    empty = nf4_moe_down_bnb(torch.zeros(0, 2, K), ex, ids[:0], rw[:0])
    assert tuple(empty.shape) == (0, N) and empty.dtype == torch.bfloat16
    none = nf4_moe_down_bnb(torch.zeros(3, 0, K), ex, ids[:, :0], rw[:, :0])
    assert tuple(none.shape) == (3, N) and (_bits(none) == 0).all()
