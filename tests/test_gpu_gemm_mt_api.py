"""33..128 rows through the Python layer (``-m gpu``): nf4_linear_bnb, Linear4bit.forward and
nf4_linear_bnb_grouped take the row-tiled entry (nf4_gemm_bnb_mt*) -- one launch, no host read
of the offset, capturable -- and everything outside its rules still takes dequantize + matmul.
Results are judged against the float64 oracle of the C oracle's exact weights with the suite's
GEMM bound."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_cases import bits_to_f64, check_close, check_gemm, gemm_oracle, x_bits

pytestmark = pytest.mark.gpu

DT = "bf16"
TDT = torch.bfloat16


def _oracle_bits_of(coracle, mod, N, K):
    qs = mod.weight.quant_state
    return coracle.dequant_bnb(mod.weight.data.view(-1).cpu().numpy(), qs.absmax.cpu().numpy(),
                               qs.state2.code.cpu().numpy(), qs.state2.absmax.cpu().numpy(), float(qs.offset),
                               N * K, O.BF16, int(qs.blocksize), int(qs.state2.blocksize)).reshape(N, K)


def _module(gpu, N, K, seed, bias=False, blocksize=64):
    from nf4_triton_dequantization_amd import Linear4bit

    wf = torch.from_numpy(O.normal_f32(seed, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    b = torch.from_numpy(O.normal_f32(seed + 1, N, stream=9)).to(gpu) if bias else None
    kw = {} if blocksize == 64 else {"blocksize": blocksize}
    return Linear4bit.from_float(wf, compute_dtype=TDT, bias=b, **kw)


def _raise_on_composite(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    def unfused(*a, **k):
        raise AssertionError("fell back to dequantize + matmul inside the row-tiled entry's domain")

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", unfused)


def test_forward_at_48_rows_never_dequantizes(coracle, gpu, monkeypatch):
    """Linear4bit.from_float(w)(x) for x [2, 24, K] (M = 48) with a bias, the unfused path made
    to raise: the oracle's result, plus the bias's one more rounding."""
    N, K = 256, 1024
    mod = _module(gpu, N, K, 41, bias=True)
    wb = _oracle_bits_of(coracle, mod, N, K)
    xt, xb = x_bits(48, K, DT, seed=3)
    _raise_on_composite(monkeypatch)
    with torch.no_grad():
        y = mod(xt.to(gpu).reshape(2, 24, K))
    assert y.shape == (2, 24, N) and y.dtype == TDT
    ref, bound = gemm_oracle(xb, wb, DT)
    b16 = mod.bias.detach().to(TDT).view(torch.int16).cpu().numpy().view(np.uint16)
    exp = ref + bits_to_f64(b16, DT)[None, :]
    bound = bound + 2.0 ** -8 * np.abs(exp)  # the 16-bit add: half an ulp of the result
    yb = y.reshape(48, N).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    check_close(bits_to_f64(yb, DT), exp, bound, "module(x) M=48")


def test_grouped_at_48_rows_never_dequantizes(coracle, gpu, monkeypatch):
    """nf4_linear_bnb_grouped(x, [q, k, v]) at M = 48: three correct outputs, no composite."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_grouped

    K = 1024
    mods = [_module(gpu, N, K, 50 + i) for i, N in enumerate((256, 128, 128))]
    xt, xb = x_bits(48, K, DT, seed=4)
    _raise_on_composite(monkeypatch)
    with torch.no_grad():
        ys = nf4_linear_bnb_grouped(xt.to(gpu), mods)
    assert len(ys) == 3
    for mod, y in zip(mods, ys):
        N = mod.out_features
        assert y.shape == (48, N)
        check_gemm(y, xb, _oracle_bits_of(coracle, mod, N, K), DT, f"grouped N={N}")


@pytest.mark.parametrize("M", [48, 64])
def test_forward_is_capturable(gpu, monkeypatch, M):
    """One capture and two replays (a host read of the offset would synchronise, which a capture
    refuses) at M = 64, and at M = 48; the replays give the eager result."""
    from nf4_triton_dequantization_amd import Linear4bit

    N, K = 256, 2048
    lin = torch.nn.Linear(K, N, bias=True, device=gpu, dtype=torch.bfloat16)
    mod = Linear4bit.from_float(lin)
    x = torch.randn((M, K), device=gpu, dtype=torch.bfloat16)
    _raise_on_composite(monkeypatch)
    with torch.no_grad():
        y0 = mod(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = mod(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, y0)
        y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
    assert y.shape == (M, N) and bool(torch.isfinite(y.float()).all())
    assert torch.equal(y, y0)


@pytest.mark.parametrize("case", ["M129", "blocksize128", "requires_grad"])
def test_outside_the_rules_takes_the_composite(coracle, gpu, monkeypatch, case):
    """129 rows, blocksize 128 and a gradient being recorded for x: dequantize + matmul (seen
    through a counting wrapper), still the oracle's result."""
    from nf4_triton_dequantization_amd import kernel

    N, K = 128, 1024
    M = 129 if case == "M129" else 48
    mod = _module(gpu, N, K, 60, blocksize=128 if case == "blocksize128" else 64)
    assert int(mod.weight.quant_state.blocksize) == (128 if case == "blocksize128" else 64)
    wb = _oracle_bits_of(coracle, mod, N, K)
    xt, xb = x_bits(M, K, DT, seed=5)
    calls = []
    real = kernel.dequantize_nf4_bnb

    def counting(m):
        calls.append(1)
        return real(m)

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", counting)
    x = xt.to(gpu)
    if case == "requires_grad":
        y = mod(x.requires_grad_())
        assert y.requires_grad and y.grad_fn is not None
        y = y.detach()
    else:
        with torch.no_grad():
            y = mod(x)
    assert len(calls) == 1, f"{case}: the composite ran {len(calls)} times"
    check_gemm(y, xb, wb, DT, case)
