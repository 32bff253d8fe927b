"""``nf4_moe_linear_bnb`` and what is built on it beyond 128 (token, choice) pairs on the GPU
(``-m gpu``): 129 .. 1024 pairs take the row-block launch (``nf4_gemm_bnb_moe_rb``), never the
per-expert loop -- which synchronises with the host and cannot be captured -- so the whole block
(``nf4_moe_mlp_bnb``) is capturable at 160 pairs and a replay follows the ids on the device.
More than 1024 pairs and a gradient for ``x`` keep the loop."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_moe_api as API
import test_gpu_moe_mlp_api as MLP
from _gemm_cases import x_bits
from test_gpu_moe_api import no_composite  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def routes(monkeypatch):
    """What nf4_moe_linear_bnb does while the test runs: ``rb`` the pair counts of its
    nf4_gemm_bnb_moe_rb calls, ``moe`` those of nf4_gemm_bnb_moe, ``loop`` the per-expert loops.
    With ``forbid_loop()`` the loop raises instead."""
    from types import SimpleNamespace

    from nf4_triton_dequantization_amd import _lib, kernel

    L = _lib.lib()
    seen = SimpleNamespace(rb=[], moe=[], loop=[])

    def counted(real, into):
        def call(*a):
            into.append(a[2])
            return real(*a)
        return call

    monkeypatch.setattr(L, "nf4_gemm_bnb_moe_rb", counted(L.nf4_gemm_bnb_moe_rb, seen.rb))
    monkeypatch.setattr(L, "nf4_gemm_bnb_moe", counted(L.nf4_gemm_bnb_moe, seen.moe))
    real_loop = kernel._moe_fallback

    def loop(x3, experts, ids, out):
        seen.loop.append(ids.numel())
        return real_loop(x3, experts, ids, out)

    def boom(x3, experts, ids, out):
        raise AssertionError(f"_moe_fallback called at {ids.numel()} pairs: the fused route was not taken")

    monkeypatch.setattr(kernel, "_moe_fallback", loop)
    seen.forbid_loop = lambda: monkeypatch.setattr(kernel, "_moe_fallback", boom)
    return seen


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T,k", [(65, 2), (64, 8)])
def test_129_to_1024_pairs_take_the_row_block_launch(coracle, gpu, no_composite, routes, dtype, T, k):  # noqa: F811
    """T * k = 130 and 512: one nf4_gemm_bnb_moe_rb call each, no per-expert loop (made to raise), no
    dequantize; x [T, K] and [T, k, K], int32 and int64 ids, ids outside 0..E-1 among them; ``out=``
    is honoured and ``Experts4bit.__call__`` agrees with the function."""
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb

    routes.forbid_loop()
    ex, bits = API._experts(coracle, gpu, dtype)
    dt = API._dt(dtype)
    ids = API._ids(T, k, seed=T, with_invalid=True)
    xt, xb = x_bits(T * k, API.K, dt, seed=3)
    calls = 0
    for shared in (True, False):
        x = (xt[:T] if shared else xt.view(T, k, API.K)).to(gpu)
        xbits = xb[:T] if shared else xb.reshape(T, k, API.K)
        for ids_dtype in (torch.int32, torch.int64):
            idt = torch.from_numpy(ids).to(ids_dtype).to(gpu)
            y = nf4_moe_linear_bnb(x, ex, idt)
            assert tuple(y.shape) == (T, k, API.N) and y.dtype == dtype
            API._check(y, xbits, ids, bits, dt, f"T={T} k={k} shared={shared} {ids_dtype} {dt}")
            calls += 1
        out = torch.full((T, k, API.N), float("nan"), dtype=dtype, device=gpu)
        assert nf4_moe_linear_bnb(x, ex, idt, out=out) is out and out.equal(y)
        assert ex(x, idt).equal(y)
        calls += 2
    assert routes.rb == [T * k] * calls and routes.moe == [] and routes.loop == []


def test_the_bounds_of_the_routes(coracle, gpu, routes):
    """128 pairs keep nf4_gemm_bnb_moe, 129 and 1024 take the row blocks, 1026 and 2000 pairs and a
    gradient for x take the per-expert loop; every result passes the oracle."""
    from nf4_triton_dequantization_amd import kernel, nf4_moe_linear_bnb

    assert (kernel.MOE_RB_ROUTED_MIN_P, kernel.MOE_RB_ROUTED_MAX_P) == (129, 1024)
    dtype = torch.bfloat16
    ex, bits = API._experts(coracle, gpu, dtype)
    want = {128: "moe", 129: "rb", 1024: "rb", 1026: "loop", 2000: "loop"}
    for P, route in want.items():
        T, k = (P, 1) if P % 2 else (P // 2, 2)
        ids = API._ids(T, k, seed=P, with_invalid=True)
        xt, xb = x_bits(T, API.K, "bf16", seed=6)
        y = nf4_moe_linear_bnb(xt.to(gpu), ex, torch.from_numpy(ids).to(gpu))
        API._check(y, xb, ids, bits, "bf16", f"{P} pairs")
        got = {"moe": routes.moe, "rb": routes.rb, "loop": routes.loop}
        assert got.pop(route) == [P] and all(v == [] for v in got.values()), (P, route, routes)
        for v in (routes.moe, routes.rb, routes.loop):
            del v[:]
    T, k = 80, 2
    ids = API._ids(T, k, seed=4, with_invalid=True)
    xt, xb = x_bits(T, API.K, "bf16", seed=8)
    x = xt.to(gpu).requires_grad_(True)
    y = nf4_moe_linear_bnb(x, ex, torch.from_numpy(ids).to(gpu))
    assert y.requires_grad and routes.loop == [T * k] and routes.rb == [] and routes.moe == []
    API._check(y.detach(), xb, ids, bits, "bf16", "160 pairs with a gradient")
    y.float().sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == (T, API.K)


def test_the_block_is_captured_at_160_pairs_and_replays_follow_the_ids(coracle, gpu, no_composite, routes):  # noqa: F811
    """``nf4_moe_mlp_bnb`` at T = 80, k = 2 (E = 4, H = 128, I = 384) under ``torch.cuda.graph``: three
    row-block launches and torch's elementwise steps, nothing read by the host (the per-expert
    loop is made to raise; before this entry the capture itself failed in its ``nonzero``).  Replay,
    overwrite ``expert_ids`` in place, replay again: each replay equals the eager block for its
    own ids bit for bit.  The eager block is judged by the oracle stage by stage: h against the
    float64 SwiGLU chain of x, the down products against the float64 GEMM of h's own bits, and y
    equal to the block's three-line expression."""
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb, nf4_moe_mlp_bnb, nf4_moe_swiglu_bnb

    routes.forbid_loop()
    dtype, T, k, inter = torch.bfloat16, 80, 2, 384
    (w1, gbits), (w3, ubits) = MLP._w13(coracle, gpu, dtype, n=inter)
    w2, dbits = MLP._experts(coracle, gpu, dtype, True, 23, MLP.H, inter)
    xt, xb = x_bits(T, MLP.H, "bf16", seed=44)
    x = xt.to(gpu)
    rw = torch.rand(T, k, generator=torch.Generator().manual_seed(12)).to(gpu)
    routings = [MLP._ids(T, k, seed=60), MLP._ids(T, k, seed=61, with_invalid=True)]
    routings.append(np.full((T, k), 3))                      # every pair on one expert: two row blocks
    ids = torch.from_numpy(routings[0]).to(gpu)              # int64: the cast to int32 is captured too
    eager = []
    for r in routings:                                       # (also the warm-up: workspaces, kernel attributes)
        ids.copy_(torch.from_numpy(r))
        h = nf4_moe_swiglu_bnb(x, w1, w3, ids)
        MLP._check(h, xb, r, gbits, ubits, "bf16", "h of the eager block")
        d = nf4_moe_linear_bnb(h, w2, ids)
        API._check(d, MLP._bits(h).reshape(T, k, inter), r, dbits, "bf16", "down products of the eager block")
        y = nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw)
        assert torch.equal(y, MLP._expression(x, w1, w3, w2, ids, rw)) and bool(torch.isfinite(y.float()).all())
        assert torch.equal(h, F.silu(nf4_moe_linear_bnb(x, w1, ids)) * nf4_moe_linear_bnb(x, w3, ids))
        eager.append(y.clone())
    assert not eager[0].equal(eager[1]) and not eager[1].equal(eager[2])
    assert routes.rb and set(routes.rb) == {T * k} and routes.moe == []
    ids.copy_(torch.from_numpy(routings[0]))
    torch.cuda.synchronize()
    del routes.rb[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw)
    assert routes.rb == [T * k] * 3 and routes.moe == []     # w1, w3, w2
    for i in (0, 1, 2, 0):
        ids.copy_(torch.from_numpy(routings[i]))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert y.equal(eager[i]), f"replay {i} differs from the eager block"
