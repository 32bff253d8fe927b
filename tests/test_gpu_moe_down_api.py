"""``nf4_moe_down_bnb`` on the GPU (``-m gpu``): the fused route bit for bit against the documented
chain over ``nf4_moe_linear_bnb``'s products (``dequantize_nf4_bnb`` made to raise, so nothing
composite can answer), for k = 2 also against the three-line torch expression; which route a call
takes (a counting wrapper on the C entry); the composite under autograd; ``nf4_moe_mlp_bnb`` at
k = 2 and k = 4; one graph capture replayed over changed ids, weights and activations."""
import numpy as np
import pytest
import torch

from _gemm_cases import x_bits
from _moe_down_cases import chain
from test_gpu_moe_api import _dt, no_composite  # noqa: F401  (no_composite: a fixture)
from test_gpu_moe_mlp_api import E, H, _bits, _block, _experts, _ids

pytestmark = pytest.mark.gpu

I = 384  # w2's K: the expert GEMM's fused route needs K % 128 == 0


@pytest.fixture()
def down_calls(monkeypatch):
    """The pair counts of the nf4_gemm_bnb_moe_down calls made while the test runs."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    real, calls = L.nf4_gemm_bnb_moe_down, []

    def counted(*a):
        calls.append(a[2])
        return real(*a)

    monkeypatch.setattr(L, "nf4_gemm_bnb_moe_down", counted)
    return calls


@pytest.fixture()
def routed_everywhere(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    monkeypatch.setattr(kernel, "MOE_DOWN_ROUTED_MIN_P", 1)
    monkeypatch.setattr(kernel, "MOE_DOWN_ROUTED_MAX_P", 128)


def _rw_np(rw, dt):
    """What the kernel is handed: fp32 values, or the experts' dtype's patterns (fp64 is cast first)."""
    if rw.dtype == torch.float32:
        return rw.cpu().numpy()
    return _bits(rw.to(torch.bfloat16 if dt == "bf16" else torch.float16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("T,k", [(1, 2), (8, 2), (8, 4)])
def test_fused_route_is_the_chain_of_the_expert_gemm(coracle, gpu, no_composite, routed_everywhere, down_calls,  # noqa: F811
                                                     dtype, nested, T, k):
    from nf4_triton_dequantization_amd import nf4_moe_down_bnb, nf4_moe_linear_bnb

    w2, _ = _experts(coracle, gpu, dtype, nested, 23, H, I)
    dt = _dt(dtype)
    ids = _ids(T, k, seed=60 + T + k, with_invalid=True)
    h = x_bits(T * k, I, dt, seed=12)[0].view(T, k, I).to(gpu)
    g = torch.Generator().manual_seed(13)
    n = 0
    for rw_dtype in (torch.float32, dtype, torch.float64):
        rw = torch.rand(T, k, generator=g, dtype=torch.float64).to(rw_dtype).to(gpu)
        for ids_dtype in (torch.int32, torch.int64):
            idt = torch.from_numpy(ids).to(ids_dtype).to(gpu)
            y = nf4_moe_down_bnb(h, w2, idt, rw)
            n += 1
            assert tuple(y.shape) == (T, H) and y.dtype == dtype
            d = nf4_moe_linear_bnb(h, w2, idt)
            want = chain(_bits(d).reshape(T * k, H), ids, E, _rw_np(rw, dt), k, dt)
            assert (_bits(y) == want).all(), f"T={T} k={k} rw {rw_dtype} {ids_dtype} {dt} nested={nested}"
            if k == 2:
                assert torch.equal(y, (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1))
        out = torch.full((T, H), float("nan"), dtype=dtype, device=gpu)
        assert nf4_moe_down_bnb(h, w2, idt, rw, out=out) is out and out.equal(y)
        n += 1
    assert down_calls == [T * k] * n, "a call did not take the fused launch"
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, w2, idt, rw[:, :1])
    with pytest.raises(ValueError):
        nf4_moe_down_bnb(h, w2, idt, rw, out=torch.empty((T, k, H), dtype=dtype, device=gpu))


def test_the_routing_constants_decide_the_route(coracle, gpu, down_calls):
    """Unpatched constants: inside MOE_DOWN_ROUTED_MIN_P .. MAX_P the call goes to the C entry, outside
    (and at 130 pairs, beyond one launch) it is the composite; both are the chain."""
    from nf4_triton_dequantization_amd import kernel, nf4_moe_down_bnb, nf4_moe_linear_bnb

    lo, hi = kernel.MOE_DOWN_ROUTED_MIN_P, kernel.MOE_DOWN_ROUTED_MAX_P
    dtype, k = torch.bfloat16, 2
    w2, _ = _experts(coracle, gpu, dtype, True, 23, H, I)
    routed = [P for P in (16, 2, 8, 32, 128) if lo <= P <= hi]
    off = [P for P in (2, 8, 32, 128) if not lo <= P <= hi]
    for P, fused in [(P, True) for P in routed[:1]] + [(P, False) for P in off[:1] + [130]]:
        T = P // k
        ids = _ids(T, k, seed=70 + P, with_invalid=True)
        idt = torch.from_numpy(ids).to(gpu)
        h = x_bits(P, I, "bf16", seed=14)[0].view(T, k, I).to(gpu)
        rw = torch.rand(T, k, generator=torch.Generator().manual_seed(P)).to(gpu)
        del down_calls[:]
        y = nf4_moe_down_bnb(h, w2, idt, rw)
        assert down_calls == ([P] if fused else []), f"{P} pairs took the wrong route"
        d = nf4_moe_linear_bnb(h, w2, idt)
        assert (_bits(y) == chain(_bits(d).reshape(P, H), ids, E, rw.cpu().numpy(), k, "bf16")).all(), P


def test_a_gradient_takes_the_composite_and_backward_reaches_h_and_the_weights(coracle, gpu, routed_everywhere, down_calls):
    from nf4_triton_dequantization_amd import nf4_moe_down_bnb

    dtype, T, k = torch.bfloat16, 4, 2
    w2, _ = _experts(coracle, gpu, dtype, True, 23, H, I)
    idt = torch.from_numpy(np.array([[0, 1], [2, 2], [3, -1], [1, 0]])).to(gpu)
    ht = x_bits(T * k, I, "bf16", seed=15)[0].view(T, k, I).to(gpu)
    rwt = torch.rand(T, k, generator=torch.Generator().manual_seed(16)).to(gpu)
    plain = nf4_moe_down_bnb(ht, w2, idt, rwt)
    assert down_calls == [T * k]
    for grad_h, grad_rw in ((True, False), (False, True), (True, True)):
        del down_calls[:]
        h, rw = ht.clone().requires_grad_(grad_h), rwt.clone().requires_grad_(grad_rw)
        y = nf4_moe_down_bnb(h, w2, idt, rw)
        assert down_calls == [] and y.requires_grad
        y.float().sum().backward()
        for t, on in ((h, grad_h), (rw, grad_rw)):
            assert (t.grad is not None) == on
            if on:
                assert t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any())
        if not grad_h:  # h without a gradient: the composite's expert GEMM is the fused one, so the bits agree
            assert torch.equal(y.detach(), plain)


def test_mlp_takes_the_fused_down_launch_at_k2_and_not_at_k4(coracle, gpu, down_calls):
    """Unpatched constants: at k = 2 the block calls the C entry when the routing constants admit its
    pair count; at k = 4 it keeps its three lines whatever they say."""
    from nf4_triton_dequantization_amd import kernel, nf4_moe_mlp_bnb

    dtype, T = torch.bfloat16, 8
    w1, w3, w2 = _block(coracle, gpu, dtype, I)
    x = x_bits(T, H, "bf16", seed=17)[0].to(gpu)
    for k in (2, 4):
        idt = torch.from_numpy(_ids(T, k, seed=80 + k)).to(gpu)
        rw = torch.rand(T, k, generator=torch.Generator().manual_seed(k)).to(gpu)
        del down_calls[:]
        y = nf4_moe_mlp_bnb(x, w1, w3, w2, idt, rw)
        admitted = k <= kernel.MOE_DOWN_MLP_MAX_K and kernel.MOE_DOWN_ROUTED_MIN_P <= T * k <= kernel.MOE_DOWN_ROUTED_MAX_P
        assert down_calls == ([T * k] if admitted else []), k
        assert tuple(y.shape) == (T, H) and bool(torch.isfinite(y.float()).all())
    assert kernel.MOE_DOWN_MLP_MAX_K == 2


def test_mlp_at_k4_never_takes_it(coracle, gpu, routed_everywhere, down_calls):
    from nf4_triton_dequantization_amd import nf4_moe_mlp_bnb

    dtype, T = torch.bfloat16, 8
    w1, w3, w2 = _block(coracle, gpu, dtype, I)
    x = x_bits(T, H, "bf16", seed=17)[0].to(gpu)
    for k, want in ((4, []), (2, [T * 2])):
        idt = torch.from_numpy(_ids(T, k, seed=80 + k)).to(gpu)
        rw = torch.rand(T, k, generator=torch.Generator().manual_seed(k)).to(gpu)
        del down_calls[:]
        nf4_moe_mlp_bnb(x, w1, w3, w2, idt, rw)
        assert down_calls == want, k


def test_graph_replay_follows_ids_weights_and_h(coracle, gpu, no_composite, routed_everywhere, down_calls):  # noqa: F811
    """One capture at E = 4, T = 8, k = 2, I = 384; replays after the ids, the routing weights and h
    were overwritten in place match the eager results for their own inputs."""
    from nf4_triton_dequantization_amd import nf4_moe_down_bnb

    dtype, T, k = torch.bfloat16, 8, 2
    w2, _ = _experts(coracle, gpu, dtype, True, 23, H, I)
    g = torch.Generator().manual_seed(18)
    cases = []
    for i in range(3):
        cases.append((x_bits(T * k, I, "bf16", seed=90 + i)[0].view(T, k, I).to(gpu),
                      torch.from_numpy(_ids(T, k, seed=95 + i, with_invalid=i == 1)).to(gpu),
                      torch.rand(T, k, generator=g).to(gpu)))
    eager = [nf4_moe_down_bnb(h, w2, ids, rw).clone() for h, ids, rw in cases]  # (also the warm-up: the workspace)
    assert not eager[0].equal(eager[1]) and not eager[1].equal(eager[2])
    h, ids, rw = (t.clone() for t in cases[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = nf4_moe_down_bnb(h, w2, ids, rw)
    assert down_calls == [T * k] * 4
    for i in (0, 1, 2, 0):
        for dst, src in zip((h, ids, rw), cases[i]):
            dst.copy_(src)
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert y.equal(eager[i]), f"replay {i} differs from the eager call"
