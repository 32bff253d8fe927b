"""The NF4 embedding gather on the host: the ``_cpu`` entries, ``nf4_embedding_bnb`` and
``Embedding4bit`` under ``NF4_BACKEND=cpu`` against the C oracle's dequantization of the whole
table indexed by the ids (raw bit patterns, equal), over the GPU suite's shape list -- nested
and single statistics, fp16 / bf16 / fp32 outputs, int32 and int64 ids -- and the error
messages of the Python call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _embed_cases import (DTYPES, IDS_NP, SHAPES, TORCH_DT, bits_of, case_id, expected, gather, ids_for,
                          make_module, table)
from nf4_triton_dequantization_amd import Embedding4bit, Linear4bit, _lib, nf4_embedding_bnb
from nf4_triton_dequantization_amd.bnb_layout import Params4bit


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("ids_t", ["int32", "int64"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("single", [False, True], ids=["nested", "single"])
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_cpu_entries_equal_the_oracle(coracle, shape, single, dt, ids_t):
    rows, dim, bs, bs2, _ = shape
    t = table(shape, single, dt)
    ids = np.concatenate([ids_for(rows), [-1, rows, rows + 1]]).astype(IDS_NP[ids_t])  # + ids out of range
    out = np.full((ids.size, dim), 0xCDCD, O.out_bits_dtype(dt))
    L = _lib.lib()
    code = _lib.IDS_I32 if ids_t == "int32" else _lib.IDS_I64
    if single:
        rc = L.nf4_embedding_bnb_single_cpu(_p(ids), code, ids.size, _p(t["packed"]), _p(t["absmax"]),
                                            t["absmax"].size, bs, _p(out), dt, rows, dim, 2)
    else:
        off = np.array([t["offset"]], np.float32)
        rc = L.nf4_embedding_bnb_cpu(_p(ids), code, ids.size, _p(t["packed"]), _p(t["a1"]), t["a1"].size,
                                     _p(t["code2"]), _p(t["a2"]), t["a2"].size, _p(off), bs, bs2, _p(out), dt, rows,
                                     dim, 2)
    assert rc == _lib.OK
    want = expected(coracle, shape, single, dt, ids)
    assert not want[-3:].any() and want[:-3].any()
    assert np.array_equal(out, want)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("single", [False, True], ids=["nested", "single"])
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_python_call_on_the_host_backend(coracle, monkeypatch, shape, single, dt):
    monkeypatch.setenv("NF4_BACKEND", "cpu")
    rows, dim = shape[:2]
    mod = make_module(shape, single, dt, "cpu")
    ids = torch.from_numpy(ids_for(rows, 6).reshape(2, 3))
    y = nf4_embedding_bnb(ids, mod)
    assert y.shape == (2, 3, dim) and y.dtype == getattr(torch, TORCH_DT[dt])
    assert np.array_equal(bits_of(y), expected(coracle, shape, single, dt, ids.numpy()))
    # int32 ids, a strided view, and out=
    wide = torch.from_numpy(ids_for(rows, 10)).to(torch.int32)
    view = wide[::2]
    out = torch.empty(5, dim, dtype=y.dtype)
    assert nf4_embedding_bnb(view, mod, out=out) is out
    assert np.array_equal(bits_of(out), expected(coracle, shape, single, dt, view.numpy()))


def test_host_tensors_raise_without_the_host_backend(monkeypatch):
    monkeypatch.delenv("NF4_BACKEND", raising=False)
    mod = make_module(SHAPES[0], False, O.BF16, "cpu")
    with pytest.raises(RuntimeError, match="needs a ROCm device tensor"):
        nf4_embedding_bnb(torch.zeros(2, dtype=torch.int64), mod)


@pytest.mark.parametrize("compress", [True, False], ids=["nested", "single"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_embedding4bit_from_float_equals_the_oracle_of_its_own_storage(coracle, monkeypatch, compress, dtype):
    monkeypatch.setenv("NF4_BACKEND", "cpu")
    torch.manual_seed(5)
    src = torch.nn.Embedding(37, 192)
    emb = Embedding4bit.from_float(src, dtype=dtype, compress_statistics=compress)
    assert (emb.num_embeddings, emb.embedding_dim) == (37, 192)
    assert isinstance(emb.weight, Params4bit) and tuple(emb.weight.quant_state.shape) == (37, 192)
    qs = emb.weight.quant_state
    assert qs.dtype == dtype
    dt = {torch.float16: O.F16, torch.bfloat16: O.BF16, torch.float32: O.F32}[dtype]
    packed = emb.weight.data.numpy().reshape(-1)
    if compress:
        w = coracle.dequant_bnb(packed, qs.absmax.numpy(), qs.state2.code.numpy(), qs.state2.absmax.numpy(),
                                float(qs.offset), 37 * 192, dt, 64, 256)
    else:
        w = coracle.dequant_bnb_single(packed, qs.absmax.numpy(), 37 * 192, dt, 64)
    ids = torch.tensor([[0, 36, 5], [5, 36, 35]])
    y = emb(ids)
    assert y.shape == (2, 3, 192) and y.dtype == dtype
    assert np.array_equal(bits_of(y), gather(w.reshape(37, 192), ids.numpy()))
    # the quantized rows are the source's, to NF4 accuracy: half the widest code gap (1 - 0.7230) of a
    # block's absmax, plus the 8-bit nested statistics' and the output rounding's few percent
    w0 = src.weight.detach()
    assert torch.allclose(y.float(), w0[ids], atol=0.2 * float(w0.abs().max()), rtol=0)


def test_default_dtype_is_the_weights_and_a_bare_weight_is_taken(monkeypatch):
    monkeypatch.setenv("NF4_BACKEND", "cpu")
    w = torch.randn(8, 64, dtype=torch.float16)
    emb = Embedding4bit.from_float(w)
    assert emb.weight.quant_state.dtype == torch.float16 and emb(torch.tensor([1])).dtype == torch.float16
    with pytest.raises(ValueError, match=r"\(8,\)"):
        Embedding4bit.from_float(torch.randn(8))


def test_as_linear_shares_the_params4bit(monkeypatch):
    monkeypatch.setenv("NF4_BACKEND", "cpu")
    emb = Embedding4bit.from_float(torch.randn(192, 256), dtype=torch.bfloat16)
    lin = emb.as_linear()
    assert isinstance(lin, Linear4bit) and lin.weight is emb.weight
    assert (lin.out_features, lin.in_features, lin.bias) == (192, 256, None)
    assert lin.weight.data.data_ptr() == emb.weight.data.data_ptr()
    assert "weight" in dict(lin.named_parameters())


def _module(**over):
    mod = make_module(SHAPES[0], False, O.BF16, "cpu")
    for k, v in over.items():
        if k == "blocksize2":
            mod.weight.quant_state.state2.blocksize = v
        else:
            setattr(mod.weight.quant_state, k, v)
    return mod


@pytest.mark.parametrize("over,ids,exc,match", [
    (dict(quant_type="fp4"), None, ValueError, "quant_type 'fp4'"),
    (dict(blocksize=32), None, ValueError, "blocksize 32"),
    (dict(blocksize=96), None, ValueError, "blocksize 96"),
    (dict(blocksize=8192), None, ValueError, "blocksize 8192"),
    (dict(blocksize2=3), None, ValueError, "state2.blocksize 3"),
    (dict(), torch.zeros(2, dtype=torch.int16), TypeError, "torch.int16"),
    (dict(), torch.zeros(2, dtype=torch.float32), TypeError, "torch.float32"),
    (dict(), torch.zeros(2, dtype=torch.int64, device="meta"), RuntimeError, "ids on 'meta'"),
])
def test_error_messages_name_the_offending_value(monkeypatch, over, ids, exc, match):
    monkeypatch.setenv("NF4_BACKEND", "cpu")
    mod = _module(**over)
    with pytest.raises(exc, match=match):
        nf4_embedding_bnb(torch.zeros(2, dtype=torch.int64) if ids is None else ids, mod)


def test_out_must_fit(monkeypatch):
    monkeypatch.setenv("NF4_BACKEND", "cpu")
    mod = _module()
    ids = torch.zeros(2, dtype=torch.int64)
    for bad in (torch.empty(2, 63, dtype=torch.bfloat16), torch.empty(2, 64, dtype=torch.float16),
                torch.empty(2, 128, dtype=torch.bfloat16)[:, ::2]):
        with pytest.raises(ValueError, match="out must be a contiguous torch.bfloat16 tensor of shape"):
            nf4_embedding_bnb(ids, mod, out=bad)
    assert nf4_embedding_bnb(torch.zeros((0, 3), dtype=torch.int64), mod).shape == (0, 3, 64)


def test_exports():
    import nf4_triton_dequantization_amd as P

    assert {"nf4_embedding_bnb", "Embedding4bit"} <= set(P.__all__)
    assert P.Embedding4bit is Embedding4bit and P.nf4_embedding_bnb is nf4_embedding_bnb
