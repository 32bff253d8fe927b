"""nf4_lora_add on the GPU through the C ABI (``-m gpu``), both dtypes: every shape of the row-tile,
K-chunk, rank and column-tile edges through the judge of _lora_cases.py (the float64 chain with
the GEMM bound carried through it), under the library's plan and under every cfg the plan admits;
``base`` null, in place and a separate tensor -- all three under the library's plan at every shape,
ONE of the three per explicit cfg, rotating with the cfg and the shape, so every (cfg, mode) pair
meets every M, K, r and N several times but not every (shape, cfg, mode) triple is run --; a
grouped call; the exact probes bit for bit; the rounding-chain probes of _lora_cases.py bit for bit
(every one of the header's four roundings changes its value there, and the expected bits are unique),
alone and three in one group; scale
0, negative and with all mantissa bits; the same bits on every call.  Every output lies between
sentinel bands that must stay untouched, and starts as NaN wherever the launch must write it."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from _lora_cases import TDT, check, drawn_case, exact_case, lora_oracle, rounding_case
from nf4_triton_dequantization_amd import _lib

pytestmark = pytest.mark.gpu

MS = (1, 5, 16, 17, 32, 33, 128)        # the row-tile edges
KS = (32, 96, 384)                      # fewer K chunks than waves, an uneven split, an even split
RS = (8, 24, 32, 64, 128)               # padding to the MFMA depth, none, several depth steps
NS = (16, 80, 192)                      # a tile mostly past the end, a ragged last tile, several tiles
CFGS = [None] + [(t, w) for t in _lib.LORA_TILES for w in _lib.LORA_WAVES]
MODES = ("null", "inplace", "separate")
BAND = 4096                             # elements of sentinel on either side of an output
SENTINEL = 0x5A5A
FULL_MANTISSA = float(np.float32(1.9999999))
assert np.float32(FULL_MANTISSA).view(np.uint32) == 0x3FFFFFFF


class Case:
    """One shape's inputs on the device with its references, computed once and never changed."""

    def __init__(self, gpu, M, K, r, N, dt, scale=1.5, seed=0, exact=False, rounding=False):
        self.M, self.K, self.r, self.N, self.dt, self.scale = M, K, r, N, dt, scale
        if exact:
            x, A, B, base, self.y_want, self.v_want = (t.to(gpu) for t in exact_case(M, K, r, N, dt, seed))
        elif rounding:
            x, A, B, base, self.y_want, self.v_want = (t.to(gpu) for t in rounding_case(M, K, r, N, dt, scale, seed))
        else:
            x, A, B, base = (t.to(gpu) for t in drawn_case(M, K, r, N, dt, seed))
        self.x, self.A, self.B, self.base = x, A, B, base
        self.ref = {"null": lora_oracle(x, A, B, scale, dt)}
        self.ref["inplace"] = self.ref["separate"] = lora_oracle(x, A, B, scale, dt, base)


_CASES = {}


def _case(gpu, *key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _CASES:
        _CASES[k] = Case(gpu, *key, **kw)
    return _CASES[k]


def _guarded(case, mode, gpu):
    """A [M, N] output between sentinel bands: NaN, or the base where the call is in place."""
    n = case.M * case.N
    buf = torch.empty(2 * BAND + n, dtype=TDT[case.dt], device=gpu)
    buf.view(torch.int16).fill_(SENTINEL)
    y = buf[BAND:BAND + n].view(case.M, case.N)
    if mode == "inplace":
        y.copy_(case.base)
    else:
        y.fill_(float("nan"))
    return buf, y


def _bands_intact(buf, n):
    bits = buf.view(torch.int16)
    return bool((bits[:BAND] == SENTINEL).all()) and bool((bits[BAND + n:] == SENTINEL).all())


def _desc(case, mode, y):
    base = {"null": None, "inplace": y.data_ptr(), "separate": case.base.data_ptr()}[mode]
    return _lib.LoraMat(case.A.data_ptr(), case.B.data_ptr(), base, y.data_ptr(), case.N, case.r, case.scale)


def _launch(x, M, K, descs, dt, cfg):
    arr = (_lib.LoraMat * len(descs))(*descs)
    c = _lib.LoraCfg(*cfg) if cfg is not None else None
    cp = ctypes.cast(ctypes.pointer(c), ctypes.c_void_p) if c is not None else None
    return _lib.lib().nf4_lora_add(x.data_ptr(), M, K, ctypes.cast(arr, ctypes.c_void_p), len(descs),
                                   _lib.BF16 if dt == "bf16" else _lib.F16, cp, torch.cuda.current_stream().cuda_stream)


def _run(case, mode, cfg, gpu):
    buf, y = _guarded(case, mode, gpu)
    rc = _launch(case.x, case.M, case.K, [_desc(case, mode, y)], case.dt, cfg)
    assert rc == _lib.OK, (rc, cfg)
    assert _bands_intact(buf, case.M * case.N), f"a write outside the output: {mode} {cfg}"
    return y


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", MS)
def test_every_shape_under_every_admitted_cfg(gpu, M, dt):
    """The library's plan takes all three base modes; an explicit cfg takes one, rotating, so every
    (cfg, mode) pair meets every M, K, r and N several times."""
    n = 0
    for K, r, N in itertools.product(KS, RS, NS):
        case = _case(gpu, M, K, r, N, dt)
        for ci, cfg in enumerate(CFGS):
            for mode in (MODES if cfg is None else (MODES[(ci + n) % 3],)):
                y = _run(case, mode, cfg, gpu)
                check(y, *case.ref[mode], f"M={M} K={K} r={r} N={N} {dt} {mode} cfg={cfg}")
        n += 1


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_grouped_call_of_three_adapters(gpu, dt):
    M, K = 17, 96
    cases = [_case(gpu, M, K, 8, 192, dt, scale=0.5, seed=1), _case(gpu, M, K, 128, 80, dt, scale=-2.0, seed=1),
             _case(gpu, M, K, 24, 16, dt, scale=3.0, seed=1)]
    x = cases[0].x
    for c in cases[1:]:
        assert torch.equal(c.x, x)                      # drawn first from the same seed: one shared x
    modes = ("inplace", "null", "separate")
    for cfg in CFGS:
        outs = [_guarded(c, m, gpu) for c, m in zip(cases, modes)]
        rc = _launch(x, M, K, [_desc(c, m, y) for c, m, (_, y) in zip(cases, modes, outs)], dt, cfg)
        assert rc == _lib.OK
        for c, m, (buf, y) in zip(cases, modes, outs):
            assert _bands_intact(buf, c.M * c.N)
            check(y, *c.ref[m], f"grouped N={c.N} r={c.r} {m} cfg={cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(1, 32, 8, 16), (5, 96, 24, 80), (33, 384, 128, 192), (128, 384, 64, 192)])
def test_exact_probes_bit_for_bit(gpu, shape, dt):
    case = _case(gpu, *shape, dt, scale=0.5, exact=True)
    for cfg in CFGS:
        for mode in MODES:
            y = _run(case, mode, cfg, gpu)
            want = case.v_want if mode == "null" else case.y_want
            assert torch.equal(y.view(torch.int16), want.view(torch.int16)), (shape, dt, mode, cfg)


PROBES = [(1, 32, 8, 16), (5, 96, 24, 80), (33, 384, 128, 192), (128, 384, 64, 192)]


def _mismatch(y, want, what):
    bad = (y.view(torch.int16) != want.view(torch.int16))
    if bool(bad.any()):
        m, n = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the header's chain; first at "
                             f"({m}, {n}): got {float(y[m, n])!r}, the chain gives {float(want[m, n])!r}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("scale", [1.5, 0.3])
@pytest.mark.parametrize("shape", PROBES)
def test_rounding_probes_bit_for_bit(gpu, shape, scale, dt):
    """t = rn(x A^T), u = rn(t B^T), v = rn(float(u) * scale), y = rn(float(base) + float(v)): inputs whose
    fp32 sums are exact in any order (sum |a| |b| below 2^24 in grid units; in fact below 2^18), so the
    bits are unique, and so large that each rounding changes 5 % of its elements or more.  A kernel that
    skips a rounding, folds the scale or the base into an unrounded value, or rounds in another mode
    differs in 6 % of the outputs or more (test_lora_cases_cpu.py)."""
    case = _case(gpu, *shape, dt, scale=scale, rounding=True)
    for cfg in CFGS:
        for mode in MODES:
            y = _run(case, mode, cfg, gpu)
            _mismatch(y, case.v_want if mode == "null" else case.y_want, f"{shape} {dt} scale={scale} {mode} cfg={cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rounding_probes_in_one_group(gpu, dt):
    """Three probes over one x in one call: r = 128 beside 24 and 8, each with its own scale and base mode."""
    M, K = 33, 384
    cases = [_case(gpu, M, K, 128, 192, dt, scale=1.5, rounding=True), _case(gpu, M, K, 24, 80, dt, scale=0.3, rounding=True),
             _case(gpu, M, K, 8, 16, dt, scale=1.5, rounding=True)]
    x = cases[0].x
    for c in cases[1:]:
        assert torch.equal(c.x, x)
    modes = ("inplace", "null", "separate")
    for cfg in CFGS:
        outs = [_guarded(c, m, gpu) for c, m in zip(cases, modes)]
        rc = _launch(x, M, K, [_desc(c, m, y) for c, m, (_, y) in zip(cases, modes, outs)], dt, cfg)
        assert rc == _lib.OK
        for c, m, (buf, y) in zip(cases, modes, outs):
            assert _bands_intact(buf, c.M * c.N)
            _mismatch(y, c.v_want if m == "null" else c.y_want, f"grouped N={c.N} r={c.r} {dt} {m} cfg={cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("scale", [0.0, -0.75, FULL_MANTISSA])
def test_scales(gpu, scale, dt):
    case = _case(gpu, 17, 96, 24, 80, dt, scale=scale)
    for mode in MODES:
        y = _run(case, mode, None, gpu)
        check(y, *case.ref[mode], f"scale={scale} {mode}")
        if scale == 0.0 and mode != "null":
            assert torch.equal(y, case.base)            # base + (+-0) is the base


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_two_calls_give_identical_bits(gpu, dt):
    for shape in ((33, 384, 64, 192), (128, 96, 128, 80), (1, 384, 8, 192)):
        case = _case(gpu, *shape, dt)
        for cfg in (None, (16, 1), (64, 2), (256, 4)):
            for mode in MODES:
                a = _run(case, mode, cfg, gpu).clone()
                b = _run(case, mode, cfg, gpu)
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, cfg, mode)
