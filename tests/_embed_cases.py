"""Inputs shared by the NF4 embedding suites (test_embed_cpu.py, test_gpu_embed.py).

A case is a [rows, dim] table on the flat bitsandbytes stream, drawn by the generators of
_gemm_bnb_cases.py (N = rows, K = dim; an odd rows * dim gets the one missing packed byte).
The expected value is always the C oracle's dequantization of the WHOLE table, reshaped to
[rows, dim] and indexed by the ids in numpy -- computed once per (case, mode, dtype) and
shared read-only; rows of ids outside [0, rows) are zero bits.
"""
from __future__ import annotations

import functools
import types

import numpy as np

import nf4_oracle as O
from _gemm_bnb_cases import drawn_weight_bnb, sensitive_weight_bnb, single_weight_bnb

# (rows, dim, blocksize, blocksize2, kind)
SHAPES = [
    (7, 64, 64, 256, "drawn"),       # one block per row; a lane group per row
    (5, 192, 64, 4, "drawn"),        # three blocks per row: rows straddle absmax2 groups
    (9, 128, 256, 16, "drawn"),      # a statistics block covers two rows (blocksize > dim)
    (6, 1024, 64, 256, "drawn"),     # more than one wave's worth per row; row slot != block index
    (16, 256, 64, 16, "sensitive"),  # an FMA in the scale or a single rounding changes the planted blocks
    (11, 100, 64, 256, "drawn"),     # general form; rows start mid-block
    (11, 77, 64, 256, "drawn"),      # general form; odd rows start on a low nibble; numel odd
    (11, 77, 128, 4, "drawn"),
]
ALIGNED = [s for s in SHAPES if s[1] % 64 == 0]
DTYPES = (O.F16, O.BF16, O.F32)
IDS_NP = {"int32": np.int32, "int64": np.int64}


def case_id(s):
    return f"{s[0]}x{s[1]}-bs{s[2]}-{s[3]}-{s[4]}"


def _pad_packed(packed, numel):
    need = (numel + 1) // 2
    if packed.size < need:  # odd rows * dim: the one missing byte (low nibble unused)
        packed = np.concatenate([packed, np.full(need - packed.size, 0x5A, np.uint8)])
    return np.ascontiguousarray(packed[:need])


@functools.lru_cache(maxsize=None)
def table(shape, single, dt):
    """dict(packed, a1, code2, a2, offset | absmax) of a case; read-only arrays."""
    rows, dim, bs, bs2, kind = shape
    numel = rows * dim
    if single:
        packed, absmax = single_weight_bnb(rows, dim, seed=rows * 1000 + dim, blocksize=bs)
        t = dict(packed=_pad_packed(packed, numel), absmax=absmax)
    elif kind == "sensitive":
        # (planted for the 16-bit type the output rounds to; an fp32 output takes the bf16 weight)
        packed, a1, code2, a2, offset, _ = sensitive_weight_bnb(rows, dim, "f16" if dt == O.F16 else "bf16")
        t = dict(packed=_pad_packed(packed, numel), a1=a1, code2=code2, a2=a2, offset=offset)
    else:
        packed, a1, code2, a2, offset = drawn_weight_bnb(rows, dim, seed=rows * 1000 + dim, blocksize=bs,
                                                         blocksize2=bs2)
        t = dict(packed=_pad_packed(packed, numel), a1=a1, code2=code2, a2=a2, offset=offset)
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def oracle_table(coracle, shape, single, dt, t=None, offset=None):
    """The oracle's whole table as bit patterns [rows, dim]."""
    rows, dim, bs, bs2, _ = shape
    t = t or table(shape, single, dt)
    if single:
        w = coracle.dequant_bnb_single(t["packed"], t["absmax"], rows * dim, dt, bs)
    else:
        w = coracle.dequant_bnb(t["packed"], t["a1"], t["code2"], t["a2"], t["offset"] if offset is None else offset,
                                rows * dim, dt, bs, bs2)
    return w.reshape(rows, dim)


_ORACLE = {}


def expected(coracle, shape, single, dt, ids):
    """Bit patterns ids.shape + (dim,): the oracle's rows, zero bits for ids outside [0, rows)."""
    key = (shape, single, dt)
    if key not in _ORACLE:
        w = oracle_table(coracle, shape, single, dt)
        w.setflags(write=False)
        _ORACLE[key] = w
    return gather(_ORACLE[key], ids)


def gather(w, ids):
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < w.shape[0])
    out = w[np.where(ok, ids, 0)]
    out[~ok] = 0
    return out


def ids_for(rows, count=None):
    """First row, last row, a repeated row and a descending run; `count` cycles / cuts it."""
    base = [0, rows - 1, rows // 2, rows // 2] + list(range(rows - 1, -1, -1))
    if count is None:
        return np.array(base, np.int64)
    return np.array([base[i % len(base)] for i in range(count)], np.int64)


TORCH_DT = {O.F16: "float16", O.BF16: "bfloat16", O.F32: "float32"}


def bits_of(x):
    """Raw bit patterns (numpy) of a torch tensor of fp16 / bf16 / fp32."""
    import torch

    x = x.detach().cpu().contiguous()
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16).numpy().view(
        np.uint32 if x.dtype == torch.float32 else np.uint16)


def make_module(shape, single, dt, device, t=None):
    """A module-like object (weight: Params4bit with a QuantState) over the case's table."""
    import torch

    from nf4_triton_dequantization_amd.bnb_layout import Params4bit, QuantState

    rows, dim, bs, bs2, _ = shape
    t = t or table(shape, single, dt)
    tt = lambda a: torch.from_numpy(np.array(a)).to(device)  # noqa: E731  (a writable copy)
    dtype = getattr(torch, TORCH_DT[dt])
    if single:
        qs = QuantState(absmax=tt(t["absmax"]), shape=torch.Size((rows, dim)), blocksize=bs, quant_type="nf4",
                        dtype=dtype)
    else:
        st2 = QuantState(absmax=tt(t["a2"]), code=tt(t["code2"]), blocksize=bs2, dtype=torch.float32)
        qs = QuantState(absmax=tt(t["a1"]), shape=torch.Size((rows, dim)), blocksize=bs, quant_type="nf4",
                        dtype=dtype, offset=torch.tensor(t["offset"], dtype=torch.float32, device=device),
                        state2=st2)
    w = Params4bit(tt(t["packed"]).view(-1, 1), qs)
    return types.SimpleNamespace(weight=w, out_features=rows, in_features=dim)
