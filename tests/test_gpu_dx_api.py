"""The input gradient through the Python layer (``-m gpu``): nf4_linear_bnb_dx is the C entry's
launch bit for bit, capturable, and the composite outside its rules; nf4_linear_bnb_autograd is
nf4_linear_bnb forward and nf4_linear_bnb_dx backward; the shipped routing leaves Linear4bit.forward
as it was.  N = 448, K = 384 as in test_gpu_gemm_pf_dx.py; gradients are judged against the float64
oracle of the C oracle's exact weights with the suite's GEMM bound."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_cases import check_gemm, x_bits

pytestmark = pytest.mark.gpu

DT, TDT = "bf16", torch.bfloat16
N, K = 448, 384


def _module(gpu, seed, nested=True, bias=False, K=K):
    from nf4_triton_dequantization_amd import Linear4bit

    wf = torch.from_numpy(O.normal_f32(seed, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    b = torch.from_numpy(O.normal_f32(seed + 1, N, stream=9)).to(gpu) if bias else None
    return Linear4bit.from_float(wf, compute_dtype=TDT, bias=b, compress_statistics=nested)


def _oracle_bits_of(coracle, mod):
    qs, q = mod.weight.quant_state, mod.weight.data.view(-1).cpu().numpy()
    return coracle.dequant_bnb(q, qs.absmax.cpu().numpy(), qs.state2.code.cpu().numpy(), qs.state2.absmax.cpu().numpy(),
                               float(qs.offset), N * K, O.BF16, int(qs.blocksize), int(qs.state2.blocksize)).reshape(N, K)


def _c_entry(mod, g2d):
    """nf4_gemm_bnb_pf_dx* on [M, N] rows under the library's cfg, on its own zeroed workspace."""
    from nf4_triton_dequantization_amd import _lib, kernel

    L, qs, keep, M = _lib.lib(), mod.weight.quant_state, [], g2d.shape[0]
    dx = torch.full((M, K), float("nan"), dtype=TDT, device=g2d.device)
    stats = kernel._bnb_stats("test", qs, g2d.device, keep)
    nested = kernel._bnb_nested(qs)
    wsz = L.nf4_gemm_bnb_pf_dx_workspace_bytes(M, N, K, None)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=g2d.device)
    args = (g2d.data_ptr(), M, mod.weight.data.data_ptr(), N * K // 2, *(stats if nested else (stats[3], stats[4], stats[6])),
            dx.data_ptr(), _lib.BF16, N, K, ws.data_ptr() if wsz else None, wsz, None, torch.cuda.current_stream().cuda_stream)
    assert (L.nf4_gemm_bnb_pf_dx if nested else L.nf4_gemm_bnb_pf_dx_single)(*args) == 0
    return dx


@pytest.mark.parametrize("nested", [True, False])
def test_dx_is_the_c_entry_bit_for_bit(gpu, nested):
    from nf4_triton_dequantization_amd import nf4_linear_bnb_dx

    mod = _module(gpu, 71, nested=nested)
    g = x_bits(3 * 43, N, DT, seed=7)[0].to(gpu).reshape(3, 43, N)
    want = _c_entry(mod, g.reshape(-1, N)).view(torch.int16).reshape(3, 43, K)
    got = nf4_linear_bnb_dx(g, mod)
    out = torch.full((3, 43, K), float("nan"), dtype=TDT, device=gpu)
    assert nf4_linear_bnb_dx(g, mod, out=out) is out
    assert got.shape == (3, 43, K) and torch.equal(got.view(torch.int16), want) and torch.equal(out.view(torch.int16), want)


@pytest.mark.parametrize("M", [8, 64, 200])
def test_autograd_forward_is_nf4_linear_bnb_and_backward_is_g_times_w(coracle, gpu, M):
    from nf4_triton_dequantization_amd import nf4_linear_bnb, nf4_linear_bnb_autograd

    mod = _module(gpu, 73, bias=True)
    wb_t = np.ascontiguousarray(_oracle_bits_of(coracle, mod).T)
    xt = x_bits(M, K, DT, seed=8)[0].to(gpu)
    with torch.no_grad():
        want = nf4_linear_bnb(xt, mod, mod.bias)
    gt, gb = x_bits(M, N, DT, seed=9)
    ones = np.full((M, N), 0x3F80, np.uint16)  # bf16 1.0: what .sum() sends back
    for upstream, bits in ((None, ones), (gt.to(gpu), gb)):
        x = xt.clone().requires_grad_()
        bias = mod.bias.detach().clone().requires_grad_()
        y = nf4_linear_bnb_autograd(x, mod, bias)
        assert y.grad_fn is not None and torch.equal(y.detach().view(torch.int16), want.view(torch.int16))
        y.sum().backward() if upstream is None else y.backward(upstream)
        check_gemm(x.grad, bits, wb_t, DT, f"x.grad M={M}")
        ref_bias = bias.detach().clone().requires_grad_()
        (want + ref_bias.to(want.dtype)).backward(torch.ones_like(want) if upstream is None else upstream)
        assert torch.equal(bias.grad, ref_bias.grad)


def test_outside_the_rules_gives_the_composites_bits(gpu):
    from nf4_triton_dequantization_amd import dequantize_nf4_bnb, nf4_linear_bnb_dx

    mod = _module(gpu, 75, K=192)
    g = x_bits(129, N, DT, seed=10)[0].to(gpu)
    assert torch.equal(nf4_linear_bnb_dx(g, mod), g @ dequantize_nf4_bnb(mod))


def test_dx_is_capturable(gpu):
    """One capture; each replay follows the new contents of the gradient buffer."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_dx

    mod = _module(gpu, 77)
    gs = [x_bits(257, N, DT, seed=s)[0].to(gpu) for s in (11, 12)]
    eager = [nf4_linear_bnb_dx(g, mod) for g in gs]
    buf = gs[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dx = nf4_linear_bnb_dx(buf, mod)
    for i in (1, 0, 1):
        buf.copy_(gs[i])
        dx.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dx, eager[i])


def test_shipped_routing_keeps_the_composite(gpu):
    from nf4_triton_dequantization_amd import dequantize_nf4_bnb, kernel

    assert (kernel.GEMM_DX_ROUTED_MIN_M, kernel.GEMM_DX_ROUTED_MAX_M) == (1, 0)
    mod = _module(gpu, 79)
    x = x_bits(64, K, DT, seed=13)[0].to(gpu).requires_grad_()
    y = mod(x)
    assert y.grad_fn is not None and torch.equal(y.detach(), x.detach() @ dequantize_nf4_bnb(mod).t())
