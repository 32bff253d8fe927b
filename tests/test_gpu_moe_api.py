"""``nf4_moe_linear_bnb`` / ``Experts4bit.forward`` on the GPU (``-m gpu``): the fused route
against the float64 oracle of each pair's expert's exact weights (``dequantize_nf4_bnb`` made to
raise, so nothing composite can answer), routing read on the device under graph replay, and the
per-expert fallback beyond 128 pairs and under autograd."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits

pytestmark = pytest.mark.gpu

E, N, K = 4, 128, 256


def _dt(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f16"


_CACHE = {}


def _experts(coracle, gpu, dtype, nested=True):
    """(Experts4bit on the GPU, the oracle's 16-bit matrix of every expert); one per (dtype, mode)."""
    from nf4_triton_dequantization_amd import Experts4bit

    key = (dtype, nested)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(17)
        w = torch.stack([torch.randn(N, K, generator=g) * (0.02 * (e + 1)) for e in range(E)]).to(dtype).to(gpu)
        ex = Experts4bit.from_float(w, compress_statistics=nested)
        code = O.BF16 if dtype == torch.bfloat16 else O.F16
        bits = []
        for e in range(E):
            q = ex.weight.data[e].cpu().numpy()
            if nested:
                bits.append(coracle.dequant_bnb(q, ex.absmax[e].cpu().numpy(), ex.code2.cpu().numpy(),
                                                ex.absmax2[e].cpu().numpy(), float(ex.offset[e]), N * K, code, 64,
                                                256).reshape(N, K))
            else:
                bits.append(coracle.dequant_bnb_single(q, ex.absmax[e].cpu().numpy(), N * K, code, 64).reshape(N, K))
        _CACHE[key] = (ex, bits)
    return _CACHE[key]


def _check(y, xb, ids, bits, dt, what):
    """y [T, k, N] against the oracle: pair (t, j) uses row t of xb [T, K] or row (t, j) of xb [T, k, K]."""
    T, k = ids.shape
    yb = y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(T * k, N)
    xrows = (np.repeat(xb, k, axis=0) if xb.ndim == 2 else xb.reshape(T * k, -1))
    flat = ids.reshape(-1)
    valid = (flat >= 0) & (flat < E)
    assert (yb[~valid] == 0).all(), f"{what}: rows of ids outside 0..E-1 are not zero"
    for e in range(E):
        sel = np.nonzero(flat == e)[0]
        if sel.size:
            ref, bound = gemm_oracle(xrows[sel], bits[e], dt)
            check_close(bits_to_f64(yb[sel], dt), ref, bound, f"{what} expert {e}")


def _ids(T, k, seed, with_invalid=False):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, E, (T, k))
    if with_invalid and T * k >= 4:
        ids.reshape(-1)[[1, -1]] = (-1, E)
    return ids


@pytest.fixture()
def no_composite(monkeypatch):
    """The fused route must not dequantize: the composite's first step raises."""
    from nf4_triton_dequantization_amd import kernel

    def boom(module):
        raise AssertionError("dequantize_nf4_bnb called: the fused route was not taken")

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", boom)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("T,k", [(1, 2), (8, 2), (64, 2)])
def test_fused_route_matches_the_oracle(coracle, gpu, no_composite, dtype, nested, T, k):
    """T * k = 2, 16 and 128 pairs; x [T, K] (shared by the token's choices) and [T, k, K]; int32 and
    int64 ids; ids outside 0..E-1 give zero rows; the function and the module's forward."""
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb

    ex, bits = _experts(coracle, gpu, dtype, nested)
    dt = _dt(dtype)
    ids = _ids(T, k, seed=T, with_invalid=True)
    xt, xb = x_bits(T * k, K, dt, seed=3)
    for shared in (True, False):
        x = xt[:T] if shared else xt.view(T, k, K)
        xbits = xb[:T] if shared else xb.reshape(T, k, K)
        for ids_dtype in (torch.int32, torch.int64):
            idt = torch.from_numpy(ids).to(ids_dtype).to(gpu)
            what = f"T={T} k={k} shared={shared} {ids_dtype} {dt} nested={nested}"
            y = nf4_moe_linear_bnb(x.to(gpu), ex, idt)
            assert tuple(y.shape) == (T, k, N) and y.dtype == dtype
            _check(y, xbits, ids, bits, dt, what)
        out = torch.full((T, k, N), float("nan"), dtype=dtype, device=gpu)
        assert ex(x.to(gpu), idt).equal(y) and nf4_moe_linear_bnb(x.to(gpu), ex, idt, out=out) is out and out.equal(y)


def test_graph_replay_follows_the_ids_on_the_device(coracle, gpu, no_composite):
    """One capture at T = 4, k = 2 with int64 ids (the cast to int32 is captured too).  Replay,
    overwrite the ids tensor in place with another routing, replay again: each replay must match
    the oracle and the eager result for its own ids -- the routing is read on the device."""
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb

    dtype, T, k = torch.bfloat16, 4, 2
    ex, bits = _experts(coracle, gpu, dtype)
    xt, xb = x_bits(T, K, "bf16", seed=5)
    x = xt.to(gpu)
    first = np.array([[0, 1], [2, 3], [1, 1], [3, 0]])
    second = np.array([[2, 2], [0, -1], [3, 1], [E, 2]])   # other experts, one twice, two invalid ids
    ids = torch.from_numpy(first).to(gpu)
    eager = {}
    for name, routing in (("first", first), ("second", second)):
        ids.copy_(torch.from_numpy(routing))
        eager[name] = nf4_moe_linear_bnb(x, ex, ids).clone()   # (also the warm-up: workspace, kernel attributes)
    ids.copy_(torch.from_numpy(first))
    torch.cuda.synchronize()
    out = torch.full((T, k, N), float("nan"), dtype=dtype, device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nf4_moe_linear_bnb(x, ex, ids, out=out)
    for name, routing in (("first", first), ("second", second), ("first", first)):
        ids.copy_(torch.from_numpy(routing))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _check(out, xb, routing, bits, "bf16", f"replay with the {name} routing")
        assert out.equal(eager[name]), f"replay with the {name} routing differs from the eager call"
    assert not eager["first"].equal(eager["second"])


@pytest.mark.parametrize("shared", [True, False])
def test_more_than_128_pairs_take_the_per_expert_loop(coracle, gpu, shared):
    """T * k = 130: the fallback over nf4_linear_bnb(x[idx], experts.expert(e)); same oracle."""
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb

    dtype, T, k = torch.bfloat16, 65, 2
    ex, bits = _experts(coracle, gpu, dtype)
    ids = _ids(T, k, seed=9, with_invalid=True)
    xt, xb = x_bits(T * k, K, "bf16", seed=7)
    x, xbits = (xt[:T], xb[:T]) if shared else (xt.view(T, k, K), xb.reshape(T, k, K))
    y = nf4_moe_linear_bnb(x.to(gpu), ex, torch.from_numpy(ids).to(gpu))
    _check(y, xbits, ids, bits, "bf16", f"130 pairs shared={shared}")


def test_a_gradient_for_x_takes_the_loop_and_backward_reaches_x(coracle, gpu):
    from nf4_triton_dequantization_amd import dequantize_nf4_bnb, nf4_moe_linear_bnb

    dtype, T, k = torch.bfloat16, 4, 2
    ex, bits = _experts(coracle, gpu, dtype)
    ids = np.array([[0, 1], [2, 2], [3, -1], [1, 0]])
    xt, xb = x_bits(T, K, "bf16", seed=8)
    x = xt.to(gpu).requires_grad_(True)
    y = nf4_moe_linear_bnb(x, ex, torch.from_numpy(ids).to(gpu))
    assert y.requires_grad
    _check(y.detach(), xb, ids, bits, "bf16", "with a gradient")
    y.float().sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == (T, K)
    # d(sum y) / dx[t] = the column sums of the token's valid experts' weights; three bf16 roundings
    # at most (each expert's product, their sum), each 2^-9 of at most the summed magnitudes
    w = [dequantize_nf4_bnb(ex.expert(e)).double() for e in range(E)]
    want = torch.stack([sum((w[e].sum(0) for e in row if 0 <= e < E), torch.zeros(K, dtype=torch.float64, device=gpu))
                        for row in ids.tolist()])
    # (and the fp32 accumulation of 128 terms: 2^-17 of the summed |w|)
    mag, mabs = (torch.stack([sum((f(w[e]) for e in row if 0 <= e < E), torch.zeros(K, dtype=torch.float64, device=gpu))
                              for row in ids.tolist()]) for f in (lambda m: m.sum(0).abs(), lambda m: m.abs().sum(0)))
    assert bool(((x.grad.double() - want).abs() <= 3 * 2.0 ** -9 * mag + 2.0 ** -17 * mabs + 1e-30).all())
