"""More than 128 rows through the Python layer (``-m gpu``): nf4_linear_bnb_prefill is one fused
launch (nf4_gemm_bnb_pf*) with no dequantized weight and no host read, capturable; nf4_linear_bnb
takes it once GEMM_PF_ROUTED_MAX_M is opened; everything outside its rules takes the composite.
Results are judged against the float64 oracle of the C oracle's exact weights with the suite's
GEMM bound."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_cases import bits_to_f64, check_close, check_gemm, gemm_oracle, x_bits

pytestmark = pytest.mark.gpu

DT, TDT = "bf16", torch.bfloat16
K = 1024


def _module(gpu, N, seed, nested=True, bias=False, blocksize=64, K=K):
    from nf4_triton_dequantization_amd import Linear4bit

    wf = torch.from_numpy(O.normal_f32(seed, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    b = torch.from_numpy(O.normal_f32(seed + 1, N, stream=9)).to(gpu) if bias else None
    kw = {} if blocksize == 64 else {"blocksize": blocksize}
    return Linear4bit.from_float(wf, compute_dtype=TDT, bias=b, compress_statistics=nested, **kw)


def _oracle_bits_of(coracle, mod, N, K=K):
    qs, q = mod.weight.quant_state, mod.weight.data.view(-1).cpu().numpy()
    if getattr(qs, "state2", None) is None:
        return coracle.dequant_bnb_single(q, qs.absmax.cpu().numpy(), N * K, O.BF16, int(qs.blocksize)).reshape(N, K)
    return coracle.dequant_bnb(q, qs.absmax.cpu().numpy(), qs.state2.code.cpu().numpy(), qs.state2.absmax.cpu().numpy(),
                               float(qs.offset), N * K, O.BF16, int(qs.blocksize), int(qs.state2.blocksize)).reshape(N, K)


def _patch_composite(monkeypatch, calls=None):
    """dequantize_nf4_bnb raises, or (calls given) counts."""
    from nf4_triton_dequantization_amd import kernel

    real = kernel.dequantize_nf4_bnb

    def wrapped(m):
        if calls is None:
            raise AssertionError("dequantized inside the prefill entry's domain")
        calls.append(1)
        return real(m)

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", wrapped)


def _check_with_bias(y, mod, xb, wb, M, what):
    ref, bound = gemm_oracle(xb, wb, DT)
    b16 = mod.bias.detach().to(TDT).view(torch.int16).cpu().numpy().view(np.uint16)
    exp = ref + bits_to_f64(b16, DT)[None, :]
    bound = bound + 2.0 ** -8 * np.abs(exp)  # the 16-bit add: half an ulp of the result
    yb = y.reshape(M, -1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    check_close(bits_to_f64(yb, DT), exp, bound, what)


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("lead", [(3, 43), (3, 100)])
def test_prefill_never_dequantizes(coracle, gpu, monkeypatch, nested, lead):
    """M = 129 and 300 as [3, rows, K] with a bias, the composite made to raise: the oracle's
    result plus the bias's one more rounding, in the lead shape."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_prefill

    N, M = 256, lead[0] * lead[1]
    mod = _module(gpu, N, 41, nested=nested, bias=True)
    wb = _oracle_bits_of(coracle, mod, N)
    xt, xb = x_bits(M, K, DT, seed=3)
    _patch_composite(monkeypatch)
    with torch.no_grad():
        y = nf4_linear_bnb_prefill(xt.to(gpu).reshape(*lead, K), mod, mod.bias)
    assert y.shape == (*lead, N) and y.dtype == TDT
    _check_with_bias(y, mod, xb, wb, M, f"prefill M={M} nested={nested}")


def test_prefill_is_capturable(gpu, monkeypatch):
    """M = 257: one capture, two replays; the replay after refilling y with NaN gives the eager bits."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_prefill

    mod = _module(gpu, 256, 43)
    x = x_bits(257, K, DT, seed=4)[0].to(gpu)
    _patch_composite(monkeypatch)
    with torch.no_grad():
        y0 = nf4_linear_bnb_prefill(x, mod)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = nf4_linear_bnb_prefill(x, mod)
        for _ in range(2):
            y.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, y0)


def test_opened_route_never_dequantizes(coracle, gpu, monkeypatch):
    """GEMM_PF_ROUTED_MAX_M = 8192: Linear4bit.forward at 129 rows is the fused launch."""
    from nf4_triton_dequantization_amd import kernel

    N = 128
    mod = _module(gpu, N, 60)
    xt, xb = x_bits(129, K, DT, seed=5)
    monkeypatch.setattr(kernel, "GEMM_PF_ROUTED_MAX_M", 8192)
    _patch_composite(monkeypatch)
    with torch.no_grad():
        y = mod(xt.to(gpu))
    check_gemm(y, xb, _oracle_bits_of(coracle, mod, N), DT, "opened route M=129")


@pytest.mark.parametrize("case", ["N192", "blocksize128", "requires_grad", "y_of_2GiB"])
def test_outside_the_rules_takes_the_composite_once(coracle, gpu, monkeypatch, case):
    """y_of_2GiB: 8192 rows of a 131072-row table (a tied vocabulary), K = 128: M * N * 2 reaches
    2^31, which the entry answers with NF4DQ_ERR_TOO_LARGE; judged on the first and last two rows."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_prefill

    N, K, M = (131072, 128, 8192) if case == "y_of_2GiB" else (192 if case == "N192" else 128, 1024, 129)
    mod = _module(gpu, N, 61, blocksize=128 if case == "blocksize128" else 64, K=K)
    xt, xb = x_bits(M, K, DT, seed=6)
    calls = []
    _patch_composite(monkeypatch, calls)
    if case == "requires_grad":
        y = nf4_linear_bnb_prefill(xt.to(gpu).requires_grad_(), mod)
        assert y.grad_fn is not None
        y = y.detach()
    else:
        with torch.no_grad():
            y = nf4_linear_bnb_prefill(xt.to(gpu), mod)
    assert len(calls) == 1, f"{case}: the composite ran {len(calls)} times"
    assert y.shape == (M, N)
    rows = [0, 1, M - 2, M - 1] if case == "y_of_2GiB" else list(range(M))
    check_gemm(y[rows], xb[rows], _oracle_bits_of(coracle, mod, N, K), DT, case)
