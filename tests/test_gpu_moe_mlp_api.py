"""``nf4_moe_swiglu_bnb`` and ``nf4_moe_mlp_bnb`` on the GPU (``-m gpu``): the fused route against
the float64 chain of the float64 GEMMs of each pair's expert's exact weights (``dequantize_nf4_bnb``
made to raise, so nothing composite can answer), the routing constants, the composite beyond 128
pairs and under autograd, and the whole block against its three-line expression and under graph
replay."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nf4_oracle as O
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits
from _swiglu_cases import accept, swiglu_oracle
from test_gpu_moe_api import _dt, no_composite  # noqa: F401  (no_composite: a fixture)

pytestmark = pytest.mark.gpu

E, H, I = 4, 128, 192


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


_CACHE = {}


def _experts(coracle, gpu, dtype, nested, seed, n, k):
    """(Experts4bit [E] x [n, k] on the GPU, the oracle's 16-bit matrix of every expert), cached."""
    from nf4_triton_dequantization_amd import Experts4bit

    key = (dtype, nested, seed, n, k)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        w = torch.stack([torch.randn(n, k, generator=g) * (0.05 * (e + 1)) for e in range(E)]).to(dtype).to(gpu)
        ex = Experts4bit.from_float(w, compress_statistics=nested)
        code = O.BF16 if dtype == torch.bfloat16 else O.F16
        bits = []
        for e in range(E):
            q = ex.weight.data[e].cpu().numpy()
            if nested:
                bits.append(coracle.dequant_bnb(q, ex.absmax[e].cpu().numpy(), ex.code2.cpu().numpy(),
                                                ex.absmax2[e].cpu().numpy(), float(ex.offset[e]), n * k, code, 64,
                                                256).reshape(n, k))
            else:
                bits.append(coracle.dequant_bnb_single(q, ex.absmax[e].cpu().numpy(), n * k, code, 64).reshape(n, k))
        _CACHE[key] = (ex, bits)
    return _CACHE[key]


def _w13(coracle, gpu, dtype, nested=True, n=I):
    return _experts(coracle, gpu, dtype, nested, 21, n, H), _experts(coracle, gpu, dtype, nested, 22, n, H)


def _check(h, xb, ids, gbits, ubits, dt, what):
    """h [T, k, I] against the oracle chain: pair (t, j) uses row t of xb [T, K] or row (t, j) of xb [T, k, K]."""
    T, k = ids.shape
    hb = _bits(h).reshape(T * k, -1)
    xrows = (np.repeat(xb, k, axis=0) if xb.ndim == 2 else xb.reshape(T * k, -1))
    flat = ids.reshape(-1)
    valid = (flat >= 0) & (flat < E)
    assert (hb[~valid] == 0).all(), f"{what}: rows of ids outside 0..E-1 are not zero"
    for e in range(E):
        sel = np.nonzero(flat == e)[0]
        if sel.size:
            (gr, gt), (ur, ut) = gemm_oracle(xrows[sel], gbits[e], dt), gemm_oracle(xrows[sel], ubits[e], dt)
            ref, bound = swiglu_oracle(gr, gt, ur, ut, dt)
            check_close(bits_to_f64(hb[sel], dt), ref, bound, f"{what} expert {e}")


def _ids(T, k, seed, with_invalid=False):
    ids = np.random.default_rng(seed).integers(0, E, (T, k))
    if with_invalid and T * k >= 4:
        ids.reshape(-1)[[1, -1]] = (-1, E)
    return ids


@pytest.fixture()
def fused_calls(monkeypatch):
    """The pair counts of the nf4_gemm_bnb_moe_swiglu calls made while the test runs."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    real, calls = L.nf4_gemm_bnb_moe_swiglu, []

    def counted(*a):
        calls.append(a[2])
        return real(*a)

    monkeypatch.setattr(L, "nf4_gemm_bnb_moe_swiglu", counted)
    return calls


@pytest.fixture()
def routed_everywhere(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    monkeypatch.setattr(kernel, "MOE_SWIGLU_ROUTED_MIN_P", 1)
    monkeypatch.setattr(kernel, "MOE_SWIGLU_ROUTED_MAX_P", 128)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("T,k", [(1, 2), (8, 2), (64, 2)])
def test_fused_route_matches_the_oracle_chain(coracle, gpu, no_composite, routed_everywhere, fused_calls,  # noqa: F811
                                              dtype, nested, T, k):
    """T * k = 2, 16 and 128 pairs with the routing constants opened to 1..128; x [T, K] (shared by
    the token's choices) and [T, k, K]; int32 and int64 ids; ids outside 0..E-1 give zero rows;
    ``out=``."""
    from nf4_triton_dequantization_amd import nf4_moe_swiglu_bnb

    (w1, gbits), (w3, ubits) = _w13(coracle, gpu, dtype, nested)
    dt = _dt(dtype)
    ids = _ids(T, k, seed=T, with_invalid=True)
    xt, xb = x_bits(T * k, H, dt, seed=3)
    for shared in (True, False):
        x = (xt[:T] if shared else xt.view(T, k, H)).to(gpu)
        xbits = xb[:T] if shared else xb.reshape(T, k, H)
        for ids_dtype in (torch.int32, torch.int64):
            idt = torch.from_numpy(ids).to(ids_dtype).to(gpu)
            h = nf4_moe_swiglu_bnb(x, w1, w3, idt)
            assert tuple(h.shape) == (T, k, I) and h.dtype == dtype
            _check(h, xbits, ids, gbits, ubits, dt, f"T={T} k={k} shared={shared} {ids_dtype} {dt} nested={nested}")
        out = torch.full((T, k, I), float("nan"), dtype=dtype, device=gpu)
        assert nf4_moe_swiglu_bnb(x, w1, w3, idt, out=out) is out and out.equal(h)
    assert fused_calls == [T * k] * 6, "a call did not take the fused launch"


def test_the_routing_constants_decide_between_the_fused_launch_and_the_composite(coracle, gpu, fused_calls):
    """Unpatched constants.  At a routed pair count the function must lie in the acceptance set of
    the composite's own g and u (K = 128 is one chunk and one K slice in both routes, so the sums
    run in the same order) without dequantizing; at a count that is not routed it IS the composite."""
    from nf4_triton_dequantization_amd import kernel, nf4_moe_linear_bnb, nf4_moe_swiglu_bnb

    lo, hi = kernel.MOE_SWIGLU_ROUTED_MIN_P, kernel.MOE_SWIGLU_ROUTED_MAX_P
    dtype, k = torch.bfloat16, 2
    (w1, gbits), (w3, ubits) = _w13(coracle, gpu, dtype)
    routed = [P for P in (16, 2, 128, 8, 32) if lo <= P <= hi and P % k == 0]
    if routed:
        T = routed[0] // k
        ids = _ids(T, k, seed=31, with_invalid=True)
        idt = torch.from_numpy(ids).to(gpu)
        x = x_bits(T, H, "bf16", seed=4)[0].to(gpu)
        h = nf4_moe_swiglu_bnb(x, w1, w3, idt)
        assert fused_calls == [T * k], "a routed pair count did not take the fused launch"
        g, u = nf4_moe_linear_bnb(x, w1, idt), nf4_moe_linear_bnb(x, w3, idt)
        accept(_bits(h).reshape(T * k, I), _bits(g).reshape(T * k, I), _bits(u).reshape(T * k, I), "bf16", f"{T * k} pairs")
    del fused_calls[:]
    off = [P for P in (1, 4, 64, 128) if not lo <= P <= hi]
    for P in off[:1] + [130]:   # (130: beyond one launch, never routed)
        T, kk = (P, 1) if P % 2 else (P // 2, 2)
        ids = _ids(T, kk, seed=32, with_invalid=True)
        idt = torch.from_numpy(ids).to(gpu)
        x = x_bits(T, H, "bf16", seed=5)[0].to(gpu)
        h = nf4_moe_swiglu_bnb(x, w1, w3, idt)
        assert fused_calls == [], f"{P} pairs are not routed and took the fused launch"
        assert h.equal(F.silu(nf4_moe_linear_bnb(x, w1, idt)) * nf4_moe_linear_bnb(x, w3, idt))
        _check(h, x_bits(T, H, "bf16", seed=5)[1], ids, gbits, ubits, "bf16", f"{P} pairs, composite")


def test_a_gradient_for_x_takes_the_composite_and_backward_reaches_x(coracle, gpu, routed_everywhere, fused_calls):
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb, nf4_moe_swiglu_bnb

    dtype, T, k = torch.bfloat16, 4, 2
    (w1, gbits), (w3, ubits) = _w13(coracle, gpu, dtype)
    ids = np.array([[0, 1], [2, 2], [3, -1], [1, 0]])
    idt = torch.from_numpy(ids).to(gpu)
    xt, xb = x_bits(T, H, "bf16", seed=8)
    x = xt.to(gpu).requires_grad_(True)
    h = nf4_moe_swiglu_bnb(x, w1, w3, idt)
    assert h.requires_grad and fused_calls == []
    _check(h.detach(), xb, ids, gbits, ubits, "bf16", "with a gradient")
    h.float().sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == (T, H) and bool(torch.isfinite(x.grad).all())
    x2 = xt.to(gpu).requires_grad_(True)
    (F.silu(nf4_moe_linear_bnb(x2, w1, idt)) * nf4_moe_linear_bnb(x2, w3, idt)).float().sum().backward()
    assert torch.equal(x.grad, x2.grad) and bool((x.grad.abs().sum(1) > 0).all())


def _block(coracle, gpu, dtype, inter):
    (w1, _), (w3, _) = _w13(coracle, gpu, dtype, n=inter)
    w2, _ = _experts(coracle, gpu, dtype, True, 23, H, inter)
    return w1, w3, w2


def _expression(x, w1, w3, w2, ids, rw):
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb, nf4_moe_swiglu_bnb

    h = nf4_moe_swiglu_bnb(x, w1, w3, ids)
    d = nf4_moe_linear_bnb(h, w2, ids)
    return (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mlp_is_its_three_line_expression(coracle, gpu, dtype):
    """E = 4, H = 128, I = 192, T = 8, k = 2; routing weights in fp32 and in the experts' dtype; ids
    with invalid ones."""
    from nf4_triton_dequantization_amd import nf4_moe_mlp_bnb

    T, k = 8, 2
    w1, w3, w2 = _block(coracle, gpu, dtype, I)
    x = x_bits(T, H, _dt(dtype), seed=6)[0].to(gpu)
    ids = torch.from_numpy(_ids(T, k, seed=33, with_invalid=True)).to(gpu)
    g = torch.Generator().manual_seed(9)
    for rw_dtype in (torch.float32, dtype):
        rw = torch.rand(T, k, generator=g).to(rw_dtype).to(gpu)
        y = nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw)
        assert tuple(y.shape) == (T, H) and y.dtype == dtype and bool(torch.isfinite(y.float()).all())
        assert torch.equal(y, _expression(x, w1, w3, w2, ids, rw)) and bool((y.float().abs().sum(1) > 0).all())


def test_mlp_graph_replay_follows_ids_weights_and_x(coracle, gpu, no_composite):  # noqa: F811
    """One capture of the whole block at E = 4, H = 128, T = 8, k = 2; replays after the ids, the
    routing weights and x were overwritten in place match the eager block for their own inputs.
    I = 384 here, not 192: w2's K is I, and the expert GEMM's fused route needs K % 128 == 0 -- at
    I = 192 the w2 projection takes the per-expert loop, which reads the routing back on the host
    and cannot be captured at all (nf4_moe_linear_bnb's docstring)."""
    from nf4_triton_dequantization_amd import nf4_moe_mlp_bnb

    dtype, T, k, inter = torch.bfloat16, 8, 2, 384
    w1, w3, w2 = _block(coracle, gpu, dtype, inter)
    g = torch.Generator().manual_seed(10)
    cases = []
    for i in range(3):
        cases.append((x_bits(T, H, "bf16", seed=40 + i)[0].to(gpu),
                      torch.from_numpy(_ids(T, k, seed=50 + i, with_invalid=i == 1)).to(gpu),
                      torch.rand(T, k, generator=g).to(gpu)))
    eager = [nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw).clone() for x, ids, rw in cases]  # (also the warm-up: workspaces)
    assert not eager[0].equal(eager[1]) and not eager[1].equal(eager[2])
    for (x, ids, rw), y in zip(cases, eager):
        assert torch.equal(y, _expression(x, w1, w3, w2, ids, rw))
    x, ids, rw = (t.clone() for t in cases[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = nf4_moe_mlp_bnb(x, w1, w3, w2, ids, rw)
    for i in (0, 1, 2, 0):
        for dst, src in zip((x, ids, rw), cases[i]):
            dst.copy_(src)
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert y.equal(eager[i]), f"replay {i} differs from the eager block"
