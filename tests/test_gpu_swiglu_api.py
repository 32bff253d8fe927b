"""``nf4_swiglu_bnb`` / ``nf4_mlp_bnb`` on the GPU (``-m gpu``): inside its rules the fused launch
(nf4_gemm_bnb_mt_swiglu) answers alone -- the tests open the routed range to 1..128 rows and make
every composite route raise -- and everything outside them takes the fallback,
``F.silu(g) * u`` over ``nf4_linear_bnb_grouped``, seen through a counting wrapper.  Results are
judged with the acceptance set of _swiglu_cases.py against the modules' own ``nf4_linear_bnb``
outputs where the K slices agree, and against the float64 chain of the C oracle's exact weights
(``swiglu_oracle``) otherwise."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits
from _swiglu_cases import accept, swiglu_oracle

pytestmark = pytest.mark.gpu

DT = "bf16"
TDT = torch.bfloat16
I, K = 1024, 256  # two chunks: the row-tiled entry's and the fused launch's choice are both one K slice


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _oracle_bits_of(coracle, mod):
    qs = mod.weight.quant_state
    n, k = int(mod.out_features), int(mod.in_features)
    q = mod.weight.data.view(-1).cpu().numpy()
    if getattr(qs, "state2", None) is not None:
        return coracle.dequant_bnb(q, qs.absmax.cpu().numpy(), qs.state2.code.cpu().numpy(), qs.state2.absmax.cpu().numpy(),
                                   float(qs.offset), n * k, O.BF16, int(qs.blocksize), int(qs.state2.blocksize)).reshape(n, k)
    return coracle.dequant_bnb_single(q, qs.absmax.cpu().numpy(), n * k, O.BF16, int(qs.blocksize)).reshape(n, k)


def _module(gpu, n, k, seed, bias=False, blocksize=64, nested=True):
    from nf4_triton_dequantization_amd import Linear4bit

    wf = torch.from_numpy(O.normal_f32(seed, n * k, stream=9).reshape(n, k)).to(gpu) * 0.1
    b = torch.from_numpy(O.normal_f32(seed + 1, n, stream=9)).to(gpu) if bias else None
    kw = {} if blocksize == 64 else {"blocksize": blocksize}
    return Linear4bit.from_float(wf, compute_dtype=TDT, bias=b, compress_statistics=nested, **kw)


_MODS = {}


def _mods(gpu, nested=True):
    """(gate, up, down) for the whole module, never changed."""
    if nested not in _MODS:
        _MODS[nested] = (_module(gpu, I, K, 71, nested=nested), _module(gpu, I, K, 73, nested=nested),
                         _module(gpu, 256, I, 75, nested=nested))
    return _MODS[nested]


def _check_chain(coracle, h, xb, gate, up, what):
    """h against the float64 chain of the float64 GEMMs; a bias is one more 16-bit add on g / u."""
    refs = []
    for mod in (gate, up):
        ref, bound = gemm_oracle(xb, _oracle_bits_of(coracle, mod), DT)
        if getattr(mod, "bias", None) is not None:
            ref = ref + bits_to_f64(_bits(mod.bias.detach().to(TDT)), DT)[None, :]
            bound = bound + 2.0 ** -8 * np.abs(ref)  # the 16-bit add: half an ulp of the result
        refs.append((ref, bound))
    ref, bound = swiglu_oracle(*refs[0], *refs[1], DT)
    check_close(bits_to_f64(_bits(h), DT).reshape(ref.shape), ref, bound, what)


def _open_range_and_forbid_composites(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    def unfused(*a, **k):
        raise AssertionError("a composite route answered inside the fused launch's domain")

    monkeypatch.setattr(kernel, "SWIGLU_ROUTED_MIN_M", 1)
    monkeypatch.setattr(kernel, "SWIGLU_ROUTED_MAX_M", 128)
    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", unfused)
    monkeypatch.setattr(kernel, "nf4_linear_bnb_grouped", unfused)


def _count_fallbacks(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    calls, real = [], kernel.nf4_linear_bnb_grouped

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(kernel, "SWIGLU_ROUTED_MIN_M", 1)
    monkeypatch.setattr(kernel, "SWIGLU_ROUTED_MAX_M", 128)
    monkeypatch.setattr(kernel, "nf4_linear_bnb_grouped", counting)
    return calls


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("M", [1, 48, 128])
def test_inside_the_rules_the_fused_launch_answers_alone(coracle, gpu, monkeypatch, M, nested):
    from nf4_triton_dequantization_amd import nf4_linear_bnb, nf4_swiglu_bnb

    gate, up, _ = _mods(gpu, nested)
    xt, xb = x_bits(M, K, DT, seed=21)
    x = xt.to(gpu)
    with torch.no_grad():
        g, u = nf4_linear_bnb(x, gate), nf4_linear_bnb(x, up)
        _open_range_and_forbid_composites(monkeypatch)
        h = nf4_swiglu_bnb(x.reshape(1, M, K), gate, up)
    assert h.shape == (1, M, I) and h.dtype == TDT
    h = h.reshape(M, I)
    _check_chain(coracle, h, xb, gate, up, f"M={M}")
    if M > 32:  # the row-tiled entry with one K slice, as here: the same sums, so the same g and u
        accept(_bits(h), _bits(g), _bits(u), DT, f"M={M} nested={nested}")


@pytest.mark.parametrize("case", ["blocksize128", "bias", "M129", "requires_grad", "mixed"])
def test_outside_the_rules_takes_the_fallback(coracle, gpu, monkeypatch, case):
    from nf4_triton_dequantization_amd import nf4_swiglu_bnb

    M = 129 if case == "M129" else 48
    gate, up, _ = _mods(gpu)
    if case == "blocksize128":
        gate = _module(gpu, I, K, 81, blocksize=128)
        assert int(gate.weight.quant_state.blocksize) == 128
    elif case == "bias":
        up = _module(gpu, I, K, 83, bias=True)
    elif case == "mixed":
        up = _mods(gpu, nested=False)[1]
    xt, xb = x_bits(M, K, DT, seed=22)
    x = xt.to(gpu)
    calls = _count_fallbacks(monkeypatch)
    if case == "requires_grad":
        x.requires_grad_()
        h = nf4_swiglu_bnb(x, gate, up)
        assert h.requires_grad and h.grad_fn is not None
        h.float().sum().backward()
        assert x.grad is not None and x.grad.shape == x.shape and bool(x.grad.float().abs().sum() > 0)
        h = h.detach()
    else:
        with torch.no_grad():
            h = nf4_swiglu_bnb(x, gate, up)
    assert len(calls) == 1, f"{case}: the fallback ran {len(calls)} times"
    _check_chain(coracle, h, xb, gate, up, case)


def test_the_committed_range_routes_as_it_says(gpu, monkeypatch):
    """Without any patch of the range: M inside [SWIGLU_ROUTED_MIN_M, SWIGLU_ROUTED_MAX_M] never
    reaches the fallback, M outside it always does."""
    from nf4_triton_dequantization_amd import kernel, nf4_swiglu_bnb

    lo, hi = kernel.SWIGLU_ROUTED_MIN_M, kernel.SWIGLU_ROUTED_MAX_M
    gate, up, _ = _mods(gpu)
    calls, real = [], kernel.nf4_linear_bnb_grouped
    monkeypatch.setattr(kernel, "nf4_linear_bnb_grouped", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for M in (1, 32, 33, 64, 128, 129):
        x = x_bits(M, K, DT, seed=23)[0].to(gpu)
        before = len(calls)
        with torch.no_grad():
            h = nf4_swiglu_bnb(x, gate, up)
        assert bool(torch.isfinite(h.float()).all())
        assert (len(calls) == before) == (lo <= M <= hi), (M, lo, hi)


def test_mlp_out_and_shapes(gpu, monkeypatch):
    from nf4_triton_dequantization_amd import nf4_linear_bnb, nf4_mlp_bnb, nf4_swiglu_bnb

    gate, up, down = _mods(gpu)
    x = x_bits(48, K, DT, seed=24)[0].to(gpu).reshape(2, 24, K)
    with torch.no_grad():
        g, u = nf4_linear_bnb(x, gate), nf4_linear_bnb(x, up)
        committed = nf4_swiglu_bnb(x, gate, up)
        _open_range_and_forbid_composites(monkeypatch)
        h = nf4_swiglu_bnb(x, gate, up)
        y = nf4_mlp_bnb(x, gate, up, down)
        assert y.shape == (2, 24, 256) and torch.equal(y, nf4_linear_bnb(h, down))
        out = torch.full((2, 24, I), float("nan"), dtype=TDT, device=gpu)
        assert nf4_swiglu_bnb(x, gate, up, out=out) is out and torch.equal(out, h)
        with pytest.raises(RuntimeError):
            nf4_swiglu_bnb(x[..., :K - 128], gate, up)
        with pytest.raises(RuntimeError):
            nf4_swiglu_bnb(x, gate, down)
        with pytest.raises(ValueError):
            nf4_swiglu_bnb(x, gate, up, out=torch.empty((2, 24, I), dtype=torch.float16, device=gpu))
        with pytest.raises(ValueError):
            nf4_swiglu_bnb(x, gate, up, out=torch.empty((48, I + 64), dtype=TDT, device=gpu))
    # whichever route the committed range takes at 48 rows, it has the same definition: both lie in
    # the acceptance set of the modules' own outputs (one K slice on every route at K = 256)
    accept(_bits(h), _bits(g), _bits(u), DT, "fused")
    accept(_bits(committed), _bits(g), _bits(u), DT, "the committed range's route")
