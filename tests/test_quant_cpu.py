"""The quantizer's host path (``NF4_BACKEND=cpu`` -> nf4_quant_bnb_cpu / nf4_quant_bnb_nested_cpu)
against the Python quantizer, bit for bit: the size and value cases of the device suite
(tests/_quant_cases.py), no GPU needed."""
import numpy as np
import pytest
import torch

from nf4_triton_dequantization_amd import Linear4bit, _lib, nf4_quantize, quantize_nf4
from nf4_triton_dequantization_amd.bnb_layout import dynamic_map

import _quant_cases as Q


@pytest.fixture(autouse=True)
def _cpu_backend(monkeypatch):
    monkeypatch.setenv("NF4_BACKEND", "cpu")


def _both(w, bs):
    want = Q.expect_single(w, bs)
    packed, qs = nf4_quantize(w, blocksize=bs, compress_statistics=False)
    assert packed.shape == ((w.numel() + 1) // 2, 1) and packed.dtype == torch.uint8
    Q.check_state(qs, w, bs, nested=False)
    Q.check_single(packed, qs.absmax, want)
    packed, qs = nf4_quantize(w, blocksize=bs, compress_statistics=True)
    Q.check_state(qs, w, bs, nested=True)
    o = Q.check_nested(packed, qs.absmax, qs.state2.absmax, qs.offset, want)
    _, qs2 = nf4_quantize(w, blocksize=bs, compress_statistics=True)
    assert np.float32(qs2.offset.item()).tobytes() == o.tobytes()   # two calls: the same bits


@pytest.mark.parametrize("dt", list(Q.DTYPES))
@pytest.mark.parametrize("numel,bs", Q.SIZE_CASES)
def test_sizes(numel, bs, dt):
    _both(Q.normal_weight(numel, dt), bs)


@pytest.mark.parametrize("name,dt", Q.VALUE_CASES)
def test_values(name, dt):
    _both(Q.value_weight(name, dt), 64)


@pytest.mark.parametrize("dt", list(Q.DTYPES))
def test_boundary_at_larger_blocks(dt):
    # the same threshold-straddling inputs with several of the 64-runs sharing one absmax
    _both(Q.boundary_weight(dt), 256)


def test_thread_counts_agree():
    """Every split of the blocks over workers gives the same bytes (and the same offset)."""
    w = Q.normal_weight(64 * (3 * 256 + 1) + 2, "bf16")
    L = _lib.lib()
    n = w.numel()
    nblk = (n + 63) // 64
    code2 = dynamic_map()
    outs = []
    for threads in (1, 2, 3, 7, 0):
        packed = torch.full(((n + 1) // 2,), 0xEE, dtype=torch.uint8)
        aq = torch.full((nblk,), 0xEE, dtype=torch.uint8)
        a2 = torch.zeros((nblk + 255) // 256)
        off = torch.zeros(())
        rc = L.nf4_quant_bnb_nested_cpu(w.data_ptr(), _lib.BF16, n, 64, code2.data_ptr(), 256, packed.data_ptr(),
                                        aq.data_ptr(), a2.data_ptr(), off.data_ptr(), threads)
        assert rc == 0
        outs.append((packed, aq, a2, off))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))
    Q.check_nested(*outs[0], Q.expect_single(w, 64))


def test_float64_shapes_and_views():
    """fp64 is quantized as its fp32 rounding (quant_state.dtype stays float64); the shape is
    kept; a non-contiguous view is quantized in its logical order."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(12, 40, generator=g, dtype=torch.float64)
    packed, qs = nf4_quantize(w, compress_statistics=False)
    pr, qr = quantize_nf4(w, compress_statistics=False)
    assert qs.dtype == torch.float64 and qs.shape == w.shape
    assert torch.equal(packed, pr) and torch.equal(qs.absmax, qr.absmax)
    wt = torch.randn(40, 12, generator=g).to(torch.bfloat16).t()
    assert not wt.is_contiguous()
    packed, qs = nf4_quantize(wt, compress_statistics=False)
    pr, qr = quantize_nf4(wt, compress_statistics=False)
    assert qs.shape == wt.shape and torch.equal(packed, pr) and torch.equal(qs.absmax, qr.absmax)
    with pytest.raises(TypeError):
        nf4_quantize(torch.zeros(4, 64, dtype=torch.int32))
    with pytest.raises(ValueError):
        nf4_quantize(torch.zeros(4, 64), blocksize=96)


def test_empty_weight():
    packed, qs = nf4_quantize(torch.zeros(0, 64, dtype=torch.bfloat16))
    assert packed.shape == (0, 1) and qs.absmax.numel() == 0 and qs.state2.absmax.numel() == 0


def test_host_tensor_without_cpu_backend_raises(monkeypatch):
    monkeypatch.delenv("NF4_BACKEND")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nf4_quantize(torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        Linear4bit.from_float(torch.zeros(4, 64))


def test_from_float_module(tmp_path):
    """from_float: the quantizer's output in the module layout, an nn.Linear's bias carried
    over, no constructor run; it dequantizes (host path) and round-trips through a checkpoint
    like a constructor-built module."""
    from nf4_triton_dequantization_amd import load_nf4_safetensors, save_nf4_safetensors, triton_dequantize_nf4

    torch.manual_seed(11)
    lin = torch.nn.Linear(192, 24, bias=True).to(torch.bfloat16)
    mod = Linear4bit.from_float(lin, compute_dtype=torch.float16)
    assert isinstance(mod, Linear4bit) and (mod.out_features, mod.in_features) == (24, 192)
    qs = mod.weight.quant_state
    assert qs.dtype == torch.float16 and qs.shape == torch.Size((24, 192)) and mod.compute_dtype == torch.float16
    assert mod.weight.dtype == torch.uint8 and mod.weight.shape == (24 * 192 // 2, 1)
    assert torch.equal(mod.bias.data, lin.bias.data) and mod.bias.data_ptr() != lin.bias.data_ptr()
    Q.check_nested(mod.weight.data, qs.absmax, qs.state2.absmax, qs.offset, Q.expect_single(lin.weight.detach(), 64))
    assert Linear4bit.from_float(lin, bias=None).bias is None
    assert Linear4bit.from_float(lin.weight).bias is None
    assert Linear4bit.from_float(lin.weight.detach(), compress_statistics=False).weight.quant_state.state2 is None
    with pytest.raises(ValueError):
        Linear4bit.from_float(torch.zeros(64))
    # the reference-semantics host dequant accepts the module (layout check; values are the
    # reference's formula over these statistics, not the bnb one)
    assert triton_dequantize_nf4(mod).shape == (24, 192)
    path = str(tmp_path / "m.safetensors")
    save_nf4_safetensors(path, {"l.weight": (mod.weight.data, qs)})
    back = load_nf4_safetensors(path)["l"]
    bq = back.weight.quant_state
    assert torch.equal(back.weight.data, mod.weight.data) and torch.equal(bq.absmax, qs.absmax)
    assert torch.equal(bq.state2.absmax, qs.state2.absmax) and torch.equal(bq.state2.code, qs.state2.code)
    assert float(bq.offset) == float(qs.offset) and bq.dtype == torch.float16 and bq.blocksize == 64
