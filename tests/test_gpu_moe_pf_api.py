"""``nf4_moe_linear_bnb_prefill`` on the GPU (``-m gpu``): a prompt's pairs in one call of
``nf4_gemm_bnb_moe_pf``, never the per-expert loop; captured in a graph a replay follows the ids;
``nf4_moe_linear_bnb`` takes the entry only inside the routed range, which ships empty."""
import numpy as np
import pytest
import torch

import test_gpu_moe_api as API
from _gemm_cases import x_bits
from test_gpu_moe_api import no_composite  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def calls(monkeypatch):
    """The pair counts of the nf4_gemm_bnb_moe_pf calls made while the test runs; the per-expert loop raises."""
    from nf4_triton_dequantization_amd import _lib, kernel

    L, seen = _lib.lib(), []
    real = L.nf4_gemm_bnb_moe_pf
    monkeypatch.setattr(L, "nf4_gemm_bnb_moe_pf", lambda *a: (seen.append(a[2]), real(*a))[1])

    def boom(x3, experts, ids, out):
        raise AssertionError(f"_moe_fallback called at {ids.numel()} pairs")

    monkeypatch.setattr(kernel, "_moe_fallback", boom)
    return seen


def _case(gpu, T, k, seed):
    ids = API._ids(T, k, seed=seed, with_invalid=True)
    xt, xb = x_bits(T, API.K, "bf16", seed=seed + 1)
    return xt.to(gpu), xb, ids, torch.from_numpy(ids).to(gpu)


@pytest.mark.parametrize("routed", [False, True])
def test_2000_pairs_make_one_call_of_the_entry(coracle, gpu, no_composite, calls, monkeypatch, routed):  # noqa: F811
    """Through the prefill function, and through nf4_moe_linear_bnb once the routed range is opened."""
    from nf4_triton_dequantization_amd import kernel, nf4_moe_linear_bnb, nf4_moe_linear_bnb_prefill

    ex, bits = API._experts(coracle, gpu, torch.bfloat16)
    x, xb, ids, idt = _case(gpu, 1000, 2, seed=20)
    if routed:
        monkeypatch.setattr(kernel, "MOE_PF_ROUTED_MAX_P", 16384)
    y = (nf4_moe_linear_bnb if routed else nf4_moe_linear_bnb_prefill)(x, ex, idt)
    assert calls == [2000] and tuple(y.shape) == (1000, 2, API.N)
    API._check(y, xb, ids, bits, "bf16", "2000 pairs")
    kernel.check_gemm_workspaces()
    assert all(int(ws.count_nonzero()) == 0 for ws, _ in kernel._GEMM_WS.values())


def test_a_replay_follows_the_ids_rewritten_in_place(coracle, gpu, no_composite, calls):  # noqa: F811
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb_prefill

    ex, bits = API._experts(coracle, gpu, torch.bfloat16)
    x, xb, ids0, idt = _case(gpu, 700, 2, seed=30)
    routings = [ids0, API._ids(700, 2, seed=31), np.full((700, 2), 3)]
    eager = []
    for r in routings:  # (also the warm-up: workspace, kernel attributes)
        idt.copy_(torch.from_numpy(r))
        eager.append(nf4_moe_linear_bnb_prefill(x, ex, idt).clone())
        API._check(eager[-1], xb, r, bits, "bf16", "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = nf4_moe_linear_bnb_prefill(x, ex, idt)
    for i in (0, 1, 2, 0, 0):
        idt.copy_(torch.from_numpy(routings[i]))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert y.equal(eager[i]), f"replay of routing {i} differs from the eager call"


def test_n_192_falls_through_to_nf4_moe_linear_bnb(coracle, gpu, calls, monkeypatch):
    """Not a multiple of 128: the prefill function hands the call on (here: 100 pairs, nf4_gemm_bnb_moe)."""
    from nf4_triton_dequantization_amd import Experts4bit, kernel, nf4_moe_linear_bnb, nf4_moe_linear_bnb_prefill

    w = (torch.randn(4, 192, API.K, generator=torch.Generator().manual_seed(3)) * 0.05).to(torch.bfloat16).to(gpu)
    ex = Experts4bit.from_float(w)
    x, _, _, idt = _case(gpu, 50, 2, seed=40)
    handed = []
    monkeypatch.setattr(kernel, "nf4_moe_linear_bnb", lambda *a: (handed.append(1), nf4_moe_linear_bnb(*a))[1])
    y = nf4_moe_linear_bnb_prefill(x, ex, idt)
    assert handed == [1] and calls == [] and y.equal(nf4_moe_linear_bnb(x, ex, idt))
