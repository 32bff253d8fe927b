"""``nf4_moe_linear_bnb_decode`` on the GPU (``-m gpu``): a decode step's pairs in one launch of
``nf4_gemm_bnb_moe_dec``; captured in a graph a replay follows the ids; ``nf4_moe_linear_bnb`` takes
the entry only inside the routed range, which ships empty."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_moe_api as API
from test_gpu_moe_api import no_composite  # noqa: F401  (a fixture)
from test_gpu_moe_pf_api import _case

pytestmark = pytest.mark.gpu


@pytest.fixture()
def calls(monkeypatch):
    """The (entry, pair count) of the expert launches made while the test runs."""
    from nf4_triton_dequantization_amd import _lib

    L, seen = _lib.lib(), []
    for name in ("nf4_gemm_bnb_moe_dec", "nf4_gemm_bnb_moe"):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, name=name, real=real: (seen.append((name[13:], a[2])), real(*a))[1])
    return seen


def test_the_function_is_the_c_entrys_bits(coracle, gpu, no_composite, calls):  # noqa: F811
    from nf4_triton_dequantization_amd import _lib, kernel, nf4_moe_linear_bnb_decode

    ex, bits = API._experts(coracle, gpu, torch.bfloat16)
    x, xb, ids, idt = _case(gpu, 50, 2, seed=20)
    y = nf4_moe_linear_bnb_decode(x, ex, idt)
    assert calls == [("moe_dec", 100)] and tuple(y.shape) == (50, 2, API.N)
    API._check(y, xb, ids, bits, "bf16", "100 pairs")
    kernel.check_gemm_workspaces()
    assert all(int(ws.count_nonzero()) == 0 for ws, _ in kernel._GEMM_WS.values())
    L, d = _lib.lib(), kernel._moe_desc(ex)
    dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    ws = torch.zeros(max(L.nf4_gemm_bnb_moe_dec_workspace_bytes(100, dp, None), 16), dtype=torch.uint8, device=gpu)
    direct, id32 = torch.full_like(y, float("nan")), idt.to(torch.int32)
    rc = L.nf4_gemm_bnb_moe_dec(x.data_ptr(), id32.data_ptr(), 100, 2, dp, direct.data_ptr(), _lib.BF16,
                                ws.data_ptr(), ws.numel(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(direct.view(torch.int16), y.view(torch.int16))


def test_129_pairs_and_a_gradient_go_to_nf4_moe_linear_bnb(coracle, gpu, calls):
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb, nf4_moe_linear_bnb_decode

    ex, _ = API._experts(coracle, gpu, torch.bfloat16)
    x, _, _, idt = _case(gpu, 43, 3, seed=40)
    assert nf4_moe_linear_bnb_decode(x, ex, idt).equal(nf4_moe_linear_bnb(x, ex, idt))
    x, _, _, idt = _case(gpu, 4, 2, seed=41)
    xg = x.clone().requires_grad_(True)
    y = nf4_moe_linear_bnb_decode(xg, ex, idt)
    assert y.requires_grad and not [c for c in calls if c[0] == "moe_dec"]


def test_a_replay_follows_the_ids_rewritten_in_place(coracle, gpu, no_composite, calls):  # noqa: F811
    from nf4_triton_dequantization_amd import nf4_moe_linear_bnb_decode

    ex, bits = API._experts(coracle, gpu, torch.bfloat16)
    x, xb, ids0, idt = _case(gpu, 40, 2, seed=30)
    routings = [ids0, API._ids(40, 2, seed=31), np.full((40, 2), 3)]
    eager = []
    for r in routings:  # (also the warm-up: workspace, kernel attributes)
        idt.copy_(torch.from_numpy(r))
        eager.append(nf4_moe_linear_bnb_decode(x, ex, idt).clone())
        API._check(eager[-1], xb, r, bits, "bf16", "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = nf4_moe_linear_bnb_decode(x, ex, idt)
    for i in (0, 1, 2, 0, 0):
        idt.copy_(torch.from_numpy(routings[i]))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert y.equal(eager[i]), f"replay of routing {i} differs from the eager call"


@pytest.mark.parametrize("opened", [False, True])
def test_nf4_moe_linear_bnb_takes_the_entry_only_inside_the_routed_range(coracle, gpu, calls, monkeypatch, opened):
    from nf4_triton_dequantization_amd import kernel, nf4_moe_linear_bnb, nf4_moe_linear_bnb_decode

    ex, _ = API._experts(coracle, gpu, torch.bfloat16)
    x, _, _, idt = _case(gpu, 64, 2, seed=50)
    if opened:
        monkeypatch.setattr(kernel, "MOE_DEC_ROUTED_MAX_P", 128)
    y = nf4_moe_linear_bnb(x, ex, idt)
    assert calls == [("moe_dec" if opened else "moe", 128)]
    if opened:
        assert y.equal(nf4_moe_linear_bnb_decode(x, ex, idt))
