"""nf4_lora_add_routed on the GPU through the C ABI (``-m gpu``), both dtypes.  A routed case is one
case of _lora_cases.py per adapter present, the rows interleaved as the ids say
(_lora_routed_cases.py), so every adapter group is judged by its own oracle and bound -- the
float64 chain with the GEMM bound carried through it -- and the probes bit for bit.

Shapes are the smallest that reach every path: K in {32, 96, 384} (96: chunk counts that do not
divide over the waves), N in {16, 80, 144} (144: a partial last tile at tile_n 64 and 128), r in
{8, 24, 40, 128}, M in {1, 5, 16, 17, 64, 65, 128} (17: the second row tile; 65 and 128: the second
ballot mask; 128 rows of one adapter: every row tile live), S in {1, 3, 8, 64}, and the routings
of _lora_routed_cases.ROUTINGS.  Every (K, r, N) meets every routing at every M and dtype (every
row on its own adapter needs M <= 64), the S
and the base mode (NULL, in place, separate) rotating with the shape and the routing; every
routing under every base mode at the mask and tile edges is a test of its own.  Every
output lies between sentinel bands that must stay untouched and starts as NaN wherever the launch
must write it.  Further: three stacks in one call, every cfg, the exact and the rounding-chain
probes, batch invariance (rows permuted, rows dropped), bit equality with nf4_lora_add per adapter
at the same waves (also for adapters zero-padded from r = 24 to a stack rank of 40; and once per
instantiation of the kernel template, all 16), the same bits
on every call, and the rows without an adapter."""
import ctypes
import itertools

import pytest
import torch

from _lora_cases import TDT
from _lora_routed_cases import INT32_MAX, INT32_MIN, ROUTINGS, Routed, routing
from nf4_triton_dequantization_amd import _lib

pytestmark = pytest.mark.gpu

MS = (1, 5, 16, 17, 64, 65, 128)
KS = (32, 96, 384)
RS = (8, 24, 40, 128)
NS = (16, 80, 144)
SS = (1, 3, 8, 64)
CFGS = [None] + [(t, w) for t in _lib.LORA_TILES for w in _lib.LORA_WAVES]
MODES = ("null", "inplace", "separate")
BAND = 4096                             # elements of sentinel on either side of an output
SENTINEL = 0x5A5A

_CASES = {}


def _case(gpu, K, r, N, dt, S, ids, **kw):
    k = (K, r, N, dt, S, tuple(ids), tuple(sorted(kw.items())))
    if k not in _CASES:
        _CASES[k] = Routed(gpu, K, r, N, dt, S, ids, **kw)
    return _CASES[k]


def _guarded(M, N, dt, base, mode, gpu):
    """A [M, N] output between sentinel bands: NaN, or the base where the call is in place."""
    buf = torch.empty(2 * BAND + M * N, dtype=TDT[dt], device=gpu)
    buf.view(torch.int16).fill_(SENTINEL)
    y = buf[BAND:BAND + M * N].view(M, N)
    if mode == "inplace":
        y.copy_(base)
    else:
        y.fill_(float("nan"))
    return buf, y


def _bands_intact(buf, n):
    bits = buf.view(torch.int16)
    return bool((bits[:BAND] == SENTINEL).all()) and bool((bits[BAND + n:] == SENTINEL).all())


def _stack(c, mode, y, base=None):
    base = c.base if base is None else base
    bp = {"null": None, "inplace": y.data_ptr(), "separate": base.data_ptr()}[mode]
    return _lib.LoraStack(c.A.data_ptr(), c.B.data_ptr(), c.scale.data_ptr(), bp, y.data_ptr(), c.N, c.a_stride, c.b_stride, c.r)


def _launch(x, ids, M, K, S, stacks, dt, cfg):
    arr = (_lib.LoraStack * len(stacks))(*stacks)
    c = _lib.LoraCfg(*cfg) if cfg is not None else None
    cp = ctypes.cast(ctypes.pointer(c), ctypes.c_void_p) if c is not None else None
    return _lib.lib().nf4_lora_add_routed(x.data_ptr(), ids.data_ptr(), M, K, S, ctypes.cast(arr, ctypes.c_void_p), len(stacks),
                                          _lib.BF16 if dt == "bf16" else _lib.F16, cp, torch.cuda.current_stream().cuda_stream)


def _run(c, mode, cfg, gpu, x=None, ids=None, base=None):
    x = c.x if x is None else x
    ids = c.ids if ids is None else ids
    base = c.base if base is None else base
    M = x.shape[0]
    buf, y = _guarded(M, c.N, c.dt, base, mode, gpu)
    rc = _launch(x, ids, M, c.K, c.S, [_stack(c, mode, y, base)], c.dt, cfg)
    assert rc == _lib.OK, (rc, cfg)
    assert _bands_intact(buf, M * c.N), f"a write outside the output: {mode} {cfg}"
    return y


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", MS)
def test_every_shape_meets_every_routing(gpu, M, dt):
    for i, (K, r, N) in enumerate(itertools.product(KS, RS, NS)):
        for j, name in enumerate(ROUTINGS):
            if name == "distinct" and M > 64:
                continue
            S, ids = routing(name, M, SS[(i + j) % 4])
            c = _case(gpu, K, r, N, dt, S, ids)
            mode = MODES[(i + j) % 3]
            c.judge(_run(c, mode, None, gpu), mode, f"M={M} K={K} r={r} N={N} S={S} {name} {dt} {mode}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", ROUTINGS)
def test_every_base_mode_at_the_mask_and_tile_edges(gpu, name, dt):
    for M, S in ((1, 64), (17, 3), (64, 64), (65, 8), (128, 1), (128, 64)):
        if name == "distinct" and M > 64:
            continue
        S, ids = routing(name, M, S, seed=1)
        c = _case(gpu, 96, 24, 144, dt, S, ids)
        for mode in MODES:
            c.judge(_run(c, mode, None, gpu), mode, f"M={M} S={S} {name} {dt} {mode}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_three_stacks_share_x_and_ids(gpu, dt):
    M, K = 65, 96
    S, ids = routing("mixed", M, 8, seed=2)
    cases = [_case(gpu, K, 8, 144, dt, S, ids), _case(gpu, K, 128, 80, dt, S, ids), _case(gpu, K, 24, 16, dt, S, ids)]
    x = cases[0].x
    for c in cases[1:]:
        assert torch.equal(c.x, x)                      # drawn from (seed, rows, K) alone: one shared x
    modes = ("inplace", "null", "separate")
    for cfg in (None, (16, 1), (64, 2), (128, 4), (256, 4)):
        outs = [_guarded(M, c.N, dt, c.base, m, gpu) for c, m in zip(cases, modes)]
        rc = _launch(x, cases[0].ids, M, K, S, [_stack(c, m, y) for c, m, (_, y) in zip(cases, modes, outs)], dt, cfg)
        assert rc == _lib.OK
        for c, m, (buf, y) in zip(cases, modes, outs):
            assert _bands_intact(buf, M * c.N)
            c.judge(y, m, f"three stacks N={c.N} r={c.r} {m} cfg={cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_cfg(gpu, dt):
    for M, S, name in ((65, 8, "mixed"), (17, 64, "distinct")):
        S, ids = routing(name, M, S, seed=3)
        c = _case(gpu, 96, 24, 144, dt, S, ids)
        for ci, cfg in enumerate(CFGS):
            for mode in (MODES if cfg is None else (MODES[ci % 3],)):
                c.judge(_run(c, mode, cfg, gpu), mode, f"M={M} {name} {dt} {mode} cfg={cfg}")


PROBES = [(32, 8, 16), (96, 24, 80), (384, 128, 144), (384, 40, 144)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["exact", "rounding"])
def test_probes_bit_for_bit(gpu, kind, dt):
    """``exact_case`` rows equal integer arithmetic and ``rounding_case`` rows equal ``chain16``'s bits:
    per adapter group, whatever the other rows of the batch are."""
    for K, r, N in PROBES:
        for M, S, name in ((5, 3, "one"), (17, 3, "zero_absent"), (65, 8, "mixed")):
            S, ids = routing(name, M, S, seed=4)
            c = _case(gpu, K, r, N, dt, S, ids, kind=kind)
            assert c.want
            for cfg in (None, (16, 1), (64, 2), (256, 4)):
                for mode in MODES:
                    c.judge(_run(c, mode, cfg, gpu), mode, f"{kind} K={K} r={r} N={N} M={M} {name} {dt} {mode} cfg={cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_batch_invariance(gpu, dt):
    """Permuting the rows with their ids and base, and dropping rows, leaves every remaining row's bits."""
    g = torch.Generator().manual_seed(5)
    for M, S, name, K, r, N in ((65, 8, "mixed", 96, 24, 144), (128, 3, "zero_absent", 384, 40, 80), (64, 64, "distinct", 32, 8, 16)):
        S, ids = routing(name, M, S, seed=5)
        c = _case(gpu, K, r, N, dt, S, ids)
        perm = torch.randperm(M, generator=g).to(gpu)
        keep = torch.sort(torch.randperm(M, generator=g)[:max(1, M // 3)]).values.to(gpu)
        for cfg in (None, (64, 1), (32, 2)):
            for mode in ("separate", "null", "inplace"):
                y = _run(c, mode, cfg, gpu)
                yp = _run(c, mode, cfg, gpu, c.x[perm].contiguous(), c.ids[perm].contiguous(), c.base[perm].contiguous())
                assert torch.equal(_bits(yp), _bits(y[perm])), (M, name, cfg, mode, "permuted")
                yk = _run(c, mode, cfg, gpu, c.x[keep].contiguous(), c.ids[keep].contiguous(), c.base[keep].contiguous())
                assert torch.equal(_bits(yk), _bits(y[keep])), (M, name, cfg, mode, "dropped")
                y1 = _run(c, mode, cfg, gpu, c.x[7:8].contiguous(), c.ids[7:8].contiguous(), c.base[7:8].contiguous())
                assert torch.equal(_bits(y1), _bits(y[7:8])), (M, name, cfg, mode, "one row")


def _lora_add(c, a, rows, mode, cfg, gpu, own):
    """nf4_lora_add on adapter a's rows (``own``: the unpadded adapter)."""
    x, base = c.x[rows].contiguous(), c.base[rows].contiguous()
    r = c.own_r if own else c.r
    A, B = c.A[a, :r].contiguous(), c.B[a, :, :r].contiguous()
    buf, y = _guarded(len(rows), c.N, c.dt, base, mode, gpu)
    bp = {"null": None, "inplace": y.data_ptr(), "separate": base.data_ptr()}[mode]
    mat = (_lib.LoraMat * 1)(_lib.LoraMat(A.data_ptr(), B.data_ptr(), bp, y.data_ptr(), c.N, r, c.scales[a]))
    cc = _lib.LoraCfg(*cfg)
    rc = _lib.lib().nf4_lora_add(x.data_ptr(), len(rows), c.K, ctypes.cast(mat, ctypes.c_void_p), 1,
                                 _lib.BF16 if c.dt == "bf16" else _lib.F16, ctypes.cast(ctypes.pointer(cc), ctypes.c_void_p),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.OK
    torch.cuda.synchronize()                             # x, A, B, base live until the launch has run
    assert _bands_intact(buf, len(rows) * c.N)
    return y


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rows_have_the_bits_of_nf4_lora_add_at_the_same_waves(gpu, dt):
    for M, S, name, K, r, N, own_r in ((65, 8, "mixed", 96, 24, 144, None), (128, 3, "zero_absent", 384, 128, 80, None),
                                       (17, 64, "distinct", 384, 8, 16, None), (65, 8, "mixed", 96, 40, 144, 24)):
        S, ids = routing(name, M, S, seed=6)
        c = _case(gpu, K, r, N, dt, S, ids, own_r=own_r)
        for waves in _lib.LORA_WAVES:
            for mode in MODES:
                y = _run(c, mode, (64, waves), gpu)
                c.judge(y, mode, f"M={M} {name} waves={waves}")
                for a, rows in c.groups.items():
                    for tile in (64, 256):               # the tile width takes no part in a row's sum
                        ya = _lora_add(c, a, rows, mode, (tile, waves), gpu, own=False)
                        assert torch.equal(_bits(y[rows]), _bits(ya)), (M, name, waves, mode, a, tile)
                    if own_r is not None:                # the unpadded adapter: exact zeros add nothing
                        ya = _lora_add(c, a, rows, mode, (64, waves), gpu, own=True)
                        assert torch.equal(_bits(y[rows]), _bits(ya)), (M, name, waves, mode, a, "unpadded")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_instantiation_matches_nf4_lora_add(gpu, dt):
    """r in {8, 24, 40, 128} are the 1, 2, 4 and 8 r tiles, M in {5, 17} the one and two row tiles per
    row block: with the dtype, all 16 instantiations of either kernel.  Every row on adapter 2 of 3,
    so the routed launch's one live slot does nf4_lora_add's whole work: the same bits."""
    for r, M in itertools.product(RS, (5, 17)):
        S, ids = routing("one", M, 3)
        assert S == 3 and ids == [2] * M
        c = _case(gpu, 96, r, 80, dt, S, ids)
        y = _run(c, "separate", (64, 2), gpu)
        ya = _lora_add(c, 2, list(range(M)), "separate", (64, 2), gpu, own=False)
        assert torch.equal(_bits(y), _bits(ya)), (r, M)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_two_calls_give_identical_bits(gpu, dt):
    for M, S, name, K, r, N in ((65, 8, "mixed", 96, 24, 144), (128, 1, "one", 384, 128, 80), (1, 64, "only_63", 384, 8, 144)):
        S, ids = routing(name, M, S, seed=7)
        c = _case(gpu, K, r, N, dt, S, ids)
        for cfg in (None, (16, 1), (64, 2), (256, 4)):
            for mode in MODES:
                a = _run(c, mode, cfg, gpu).clone()
                b = _run(c, mode, cfg, gpu)
                assert torch.equal(_bits(a), _bits(b)), (M, name, cfg, mode)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rows_without_an_adapter(gpu, dt):
    """Bit for bit the base (a -0 base stays -0), zeros under base NULL, untouched memory in place --
    at every tile width, with and without adapters present beside them."""
    for M, S, name in ((1, 1, "all_invalid"), (65, 64, "all_invalid"), (128, 8, "all_invalid"), (128, 8, "mixed")):
        S, ids = routing(name, M, S, seed=8)
        c = _case(gpu, 32, 8, 144, dt, S, ids)
        assert c.none and bool((_bits(c.base[c.none]) == -0x8000).any())
        assert {INT32_MIN, INT32_MAX, -1, S} & set(c.id_list)
        for cfg in (None, (16, 4), (64, 1), (128, 2), (256, 4)):
            y = _run(c, "separate", cfg, gpu)
            assert torch.equal(_bits(y[c.none]), _bits(c.base[c.none]))
            y = _run(c, "null", cfg, gpu)
            assert not bool(_bits(y[c.none]).any())     # +0, never -0
            # in place: the rows are not stored at all -- a poisoned "base" comes back as it was
            poison = c.base.clone()
            poison[c.none] = float("nan")
            y = _run(c, "inplace", cfg, gpu, base=poison)
            assert torch.equal(_bits(y[c.none]), _bits(poison[c.none]))
            c.judge(_run(c, "inplace", cfg, gpu), "inplace", f"M={M} {name} cfg={cfg}")
