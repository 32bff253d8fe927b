"""``Experts4bit`` and the per-expert route of ``nf4_moe_linear_bnb`` with CPU tensors (no GPU).

Storage: ``from_float`` goes through the library's host quantizer (``NF4_BACKEND=cpu``) and must
stack exactly the bytes of E separate ``Linear4bit.from_float`` calls; ``expert(e)`` is a view.
Routing: on CPU tensors ``nf4_moe_linear_bnb`` takes the per-expert loop over ``nf4_linear_bnb``.
``dequantize_nf4_bnb`` has no host form, so the tests put the C oracle's dequantization in its
place (for the loop and for the expected rows alike): what is checked is which rows go to which
expert, the zero rows, and both layouts of x -- with no tolerance."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from nf4_triton_dequantization_amd import Experts4bit, Linear4bit, kernel, nf4_linear_bnb, nf4_moe_linear_bnb

E, N, K = 4, 64, 256


@pytest.fixture()
def cpu_backend(monkeypatch):
    monkeypatch.setenv("NF4_BACKEND", "cpu")


@pytest.fixture()
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
    return dequant


def _weights(seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    # every expert on its own scale, so that absmax2 groups and offsets differ between experts
    return torch.stack([torch.randn(N, K, generator=g) * (0.02 * (e + 1)) for e in range(E)]).to(dtype)


@pytest.mark.parametrize("nested", [True, False])
def test_from_float_stacks_the_bytes_of_separate_quantizations(cpu_backend, nested):
    w = _weights()
    ex = Experts4bit.from_float(w, compress_statistics=nested)
    assert (ex.num_experts, ex.out_features, ex.in_features, ex.dtype) == (E, N, K, torch.bfloat16)
    assert ex.weight.dtype == torch.uint8 and tuple(ex.weight.shape) == (E, N * K // 2) and not ex.weight.requires_grad
    assert tuple(ex.absmax.shape) == (E, N * K // 64) and ex.nested == nested
    for e in range(E):
        lin = Linear4bit.from_float(w[e], compress_statistics=nested)
        qs = lin.weight.quant_state
        assert torch.equal(ex.weight.data[e], lin.weight.data.reshape(-1))
        assert ex.absmax.dtype == qs.absmax.dtype and torch.equal(ex.absmax[e], qs.absmax)
        if nested:
            assert torch.equal(ex.absmax2[e], qs.state2.absmax) and torch.equal(ex.code2, qs.state2.code)
            assert ex.offset[e].item() == qs.offset.item()
        else:
            assert ex.absmax2 is None and ex.code2 is None and ex.offset is None
    if nested:  # own statistics: the experts' offsets are not one number
        assert len({float(v) for v in ex.offset}) == E
    # a list of nn.Linear / bare weights and a compute dtype
    mods = [torch.nn.Linear(K, N, bias=False) for _ in range(2)]
    ex2 = Experts4bit.from_float([mods[0], mods[1].weight.detach()], compute_dtype=torch.float16, compress_statistics=nested)
    assert ex2.dtype == torch.float16 and ex2.num_experts == 2
    assert torch.equal(ex2.weight.data[1], Linear4bit.from_float(mods[1]).weight.data.reshape(-1))
    with pytest.raises(ValueError):
        Experts4bit.from_float(w[0])  # [N, K]: not a stack


@pytest.mark.parametrize("nested", [True, False])
def test_expert_is_a_view_of_the_stack(cpu_backend, nested):
    ex = Experts4bit.from_float(_weights(1), compress_statistics=nested)
    for e in range(E):
        lin = ex.expert(e)
        qs = lin.weight.quant_state
        assert isinstance(lin, Linear4bit) and lin.bias is None and (lin.out_features, lin.in_features) == (N, K)
        assert lin.weight.data.data_ptr() == ex.weight.data[e].data_ptr() and tuple(lin.weight.data.shape) == (N * K // 2, 1)
        assert qs.absmax.data_ptr() == ex.absmax[e].data_ptr() and qs.blocksize == 64 and qs.quant_type == "nf4"
        assert qs.dtype == ex.dtype and tuple(qs.shape) == (N, K)
        if nested:
            assert qs.state2.absmax.data_ptr() == ex.absmax2[e].data_ptr() and qs.state2.blocksize == 256
            assert qs.state2.code.data_ptr() == ex.code2.data_ptr() and qs.offset.data_ptr() == ex.offset[e].data_ptr()
        else:
            assert qs.state2 is None and qs.offset is None
    with pytest.raises(IndexError):
        ex.expert(E)


def test_from_modules_round_trips_and_rejects_mixed_groups(cpu_backend):
    w = _weights(2)
    mods = [Linear4bit.from_float(w[e]) for e in range(E)]
    ex = Experts4bit.from_modules(mods)
    for e, m in enumerate(mods):
        got, want = ex.expert(e).weight, m.weight
        assert torch.equal(got.data, want.data) and got.data.data_ptr() != want.data.data_ptr()  # a copy
        assert torch.equal(got.quant_state.absmax, want.quant_state.absmax)
        assert torch.equal(got.quant_state.state2.absmax, want.quant_state.state2.absmax)
        assert got.quant_state.offset.item() == want.quant_state.offset.item()
    single = Linear4bit.from_float(w[0], compress_statistics=False)
    other_shape = Linear4bit.from_float(w[0][:, :128])
    other_dtype = Linear4bit.from_float(w[0], compute_dtype=torch.float16)
    other_block = Linear4bit.from_float(w[0], blocksize=128)
    for bad in (single, other_shape, other_dtype, other_block):
        with pytest.raises(ValueError):
            Experts4bit.from_modules([mods[0], bad])
    with pytest.raises(ValueError):
        Experts4bit.from_modules([])
    singles = Experts4bit.from_modules([Linear4bit.from_float(w[e], compress_statistics=False) for e in range(2)])
    assert not singles.nested and singles.absmax.dtype == torch.float32


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("per_pair", [False, True])
def test_fallback_route_is_the_per_expert_loop(cpu_backend, oracle_dequant, nested, ids_dtype, per_pair):
    """x [T, K] (shared by the token's choices) and [T, k, K]; an id outside 0..E-1 (-1 and E)
    gives a row of zeros; one token names the same expert twice; expert 3 stays idle."""
    T, k = 5, 2
    ex = Experts4bit.from_float(_weights(3), compress_statistics=nested)
    ids = torch.tensor([[0, 1], [2, 2], [-1, 0], [1, E], [2, 0]], dtype=ids_dtype)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((T, k, K) if per_pair else (T, K), generator=g).to(torch.bfloat16)
    y = nf4_moe_linear_bnb(x, ex, ids)
    assert tuple(y.shape) == (T, k, N) and y.dtype == torch.bfloat16
    for t in range(T):
        for j in range(k):
            e = int(ids[t, j])
            row = x[t, j] if per_pair else x[t]
            want = nf4_linear_bnb(row[None], ex.expert(e))[0] if 0 <= e < E else torch.zeros(N, dtype=torch.bfloat16)
            assert torch.equal(y[t, j], want), (t, j, e)
    assert torch.equal(ex(x, ids), y)                       # Experts4bit.forward is the same call
    out = torch.full((T, k, N), float("nan"), dtype=torch.bfloat16)
    assert nf4_moe_linear_bnb(x, ex, ids, out=out) is out and torch.equal(out, y)


def test_fallback_route_reaches_x_with_a_gradient(cpu_backend, oracle_dequant):
    ex = Experts4bit.from_float(_weights(4))
    ids = torch.tensor([[0, 3], [1, 1]])
    x = torch.randn(2, K, requires_grad=True)
    y = nf4_moe_linear_bnb(x, ex, ids)
    assert y.requires_grad
    y.float().sum().backward()
    # d(sum y) / dx[t] = the column sums of the token's experts' weights (each a bf16 sum of 64 rows)
    want = torch.stack([sum(oracle_dequant(ex.expert(int(e))).double().sum(0) for e in row) for row in ids])
    # three bf16 roundings at most (each expert's product, their sum), each 2^-9 of a value no larger
    # than the sum of the two experts' magnitudes
    mag = torch.stack([sum(oracle_dequant(ex.expert(int(e))).double().sum(0).abs() for e in row) for row in ids])
    assert x.grad is not None and bool(((x.grad.double() - want).abs() <= 3 * 2.0 ** -9 * mag + 1e-30).all())


def test_argument_checks(cpu_backend):
    ex = Experts4bit.from_float(_weights(5))
    ids = torch.zeros((3, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        nf4_moe_linear_bnb(torch.zeros(3, K + 1), ex, ids)
    with pytest.raises(RuntimeError):
        nf4_moe_linear_bnb(torch.zeros(3, 3, K), ex, ids)
    with pytest.raises(ValueError):
        nf4_moe_linear_bnb(torch.zeros(3, K), ex, ids.float())
    with pytest.raises(ValueError):
        nf4_moe_linear_bnb(torch.zeros(3, K), ex, ids.reshape(-1))
    with pytest.raises(ValueError):
        nf4_moe_linear_bnb(torch.zeros(3, K), ex, ids, out=torch.zeros(3, 2, N))  # fp32 out, bf16 experts
    empty = nf4_moe_linear_bnb(torch.zeros(0, K), ex, ids[:0])
    assert tuple(empty.shape) == (0, 2, N)
