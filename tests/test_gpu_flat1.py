"""The one-tile flat kernel with scalar, preloaded arguments (``-m gpu``).

One flat-eligible matrix under the default, uncapped grid goes to ``nf4_flat1_kernel``
(csrc/nf4_dequant.hip): every wave owns exactly one tile (2,048 elements of 16-bit
output, 1,024 of fp32), its arguments are scalars instead of the ``Batch`` struct, and the
valid-wave test uses the tile count passed as an argument.  The shapes here are the
smallest at which that body can go wrong -- a fraction of a tile, exactly one tile, last
workgroups with 1, 2 and 3 waves past the end, blocks-per-row of 1, 3 (the magic-number
division) and 64, and absmax arrays shorter than the block count (both modulo wraps) --
in every output type, every byte compared with the C oracle, the output prefilled with a
NaN pattern and 2^18 sentinel elements behind it checked untouched.

All cases are flat-eligible: n % 64 == 0, dense packed rows, 4-byte-aligned packed
pointer and 16-byte-aligned output.
"""
import ctypes

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _helpers import DT_CODE, GUARD_AFTER, assert_bits_equal, torch_dtype

pytestmark = pytest.mark.gpu

DTS = ("bf16", "f16", "f32")
# (m, n, absmax overrides)
SHAPES = {
    "1x64": (1, 64, {}),            # one scale block, a fraction of a tile; three of four waves own nothing
    "1x2048": (1, 2048, {}),        # exactly one 16-bit tile (two fp32 tiles)
    "1x1024": (1, 1024, {}),        # exactly one fp32 tile (half a 16-bit tile)
    "3x2048": (3, 2048, {}),        # 16-bit: one wave of the last workgroup past the end
    "5x2048": (5, 2048, {}),        # 16-bit: three waves of the last workgroup past the end
    "32x64": (32, 64, {}),          # bpr = 1: 32 rows in one tile
    "7x192": (7, 192, {}),          # bpr = 3: the non-power-of-two magic division
    "2x4096": (2, 4096, {}),        # bpr = 64: a tile of half a row
    "16x256_wrap": (16, 256, {"nb": 37, "n2": 3}),  # 64 blocks, 16 nested groups: both modulo wraps
}
assert GUARD_AFTER >= 1 << 18

NAN_BITS = {"bf16": 0x7FC1, "f16": 0x7E01, "f32": 0x7FC00001}
SENTINEL = {"bf16": 0x5A5A, "f16": 0x5A5A, "f32": 0x5A5A5A5A}


def _bits_view(t, dt):
    return t.view(torch.int32 if dt == "f32" else torch.int16)


def _out(numel, dt, dev):
    """`numel` outputs prefilled with a NaN pattern, GUARD_AFTER sentinel elements behind
    them; the output starts the (256-byte aligned) allocation, so it is 16-byte aligned."""
    buf = torch.empty(numel + GUARD_AFTER, dtype=torch_dtype(dt), device=dev)
    bits = _bits_view(buf, dt)
    bits[:numel] = NAN_BITS[dt]
    bits[numel:] = SENTINEL[dt]
    assert buf.data_ptr() % 16 == 0
    return buf


def _check(buf, numel, dt, want, what):
    bits = _bits_view(buf, dt).cpu().numpy()
    assert (bits[numel:] == SENTINEL[dt]).all(), f"{what}: write past the output"
    got = bits[:numel].view(np.uint32 if dt == "f32" else np.uint16)
    assert_bits_equal(got, np.asarray(want).reshape(-1), dt, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


_inputs_cache = {}


def _inputs(name):
    """Host inputs of one shape (computed once, shared, never modified)."""
    if name not in _inputs_cache:
        m, n, ov = SHAPES[name]
        p, a1, a2, single = O.golden_case_inputs(m, n, 4100 + sorted(SHAPES).index(name), dict(ov, single=0))
        _inputs_cache[name] = (m, n, p, a1, a2, single)
    return _inputs_cache[name]


_want_cache = {}


def _want_ref(coracle, name, dt):
    if (name, dt) not in _want_cache:
        m, n, p, a1, a2, _ = _inputs(name)
        _want_cache[(name, dt)] = coracle.dequant_ref(p, a1, a2, m, n, DT_CODE[dt])
    return _want_cache[(name, dt)]


def _ref(L, tp, t1, t2, buf, dt, m, n, cfg=None):
    if cfg is None:
        rc = L.nf4_dequant_ref(tp.data_ptr(), tp.numel(), t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(),
                               buf.data_ptr(), DT_CODE[dt], m, n, _stream())
    else:
        rc = L.nf4_dequant_ref_cfg(tp.data_ptr(), tp.numel(), t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(),
                                   buf.data_ptr(), DT_CODE[dt], m, n, ctypes.byref(cfg), _stream())
    assert rc == 0, rc


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_default_entry_matches_oracle(coracle, gpu, name, dt):
    from nf4_triton_dequantization_amd import _lib

    m, n, p, a1, a2, _ = _inputs(name)
    tp, t1, t2 = (torch.from_numpy(a).to(gpu) for a in (p, a1, a2))
    assert tp.data_ptr() % 4 == 0 and n % 64 == 0 and p.size == m * n // 2
    buf = _out(m * n, dt, gpu)
    _ref(_lib.lib(), tp, t1, t2, buf, dt, m, n)
    torch.cuda.synchronize()
    _check(buf, m * n, dt, _want_ref(coracle, name, dt), f"ref {name} {dt}")


@pytest.mark.parametrize("dt", DTS)
def test_other_modes_5x2048(coracle, gpu, dt):
    """Single-quant, bitsandbytes and bitsandbytes-single entries on 5x2048 (10,240 elements)."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    m, n, p, a1, _, single = _inputs("5x2048")
    numel, nblk = m * n, m * n // 64
    rng = np.random.default_rng(5 * 2048)
    code2 = np.sort(rng.uniform(-1, 1, 256).astype(np.float32))
    a2b = rng.uniform(1e-3, 1e-2, -(-nblk // 256)).astype(np.float32)
    tp, t1, ts, tc, t2 = (torch.from_numpy(a).to(gpu) for a in (p, a1, single, code2, a2b))
    assert a1.size == nblk and single.size == nblk

    buf = _out(numel, dt, gpu)
    rc = L.nf4_dequant_single(tp.data_ptr(), p.size, ts.data_ptr(), ts.numel(), buf.data_ptr(), DT_CODE[dt], m, n,
                              _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _check(buf, numel, dt, coracle.dequant_single(p, single, m, n, DT_CODE[dt]), f"single {dt}")

    buf = _out(numel, dt, gpu)
    rc = L.nf4_dequant_bnb(tp.data_ptr(), t1.data_ptr(), nblk, tc.data_ptr(), t2.data_ptr(), t2.numel(), 0.03125,
                           buf.data_ptr(), DT_CODE[dt], numel, 64, 256, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _check(buf, numel, dt, coracle.dequant_bnb(p, a1, code2, a2b, 0.03125, numel, DT_CODE[dt]), f"bnb {dt}")

    buf = _out(numel, dt, gpu)
    rc = L.nf4_dequant_bnb_single(tp.data_ptr(), ts.data_ptr(), nblk, buf.data_ptr(), DT_CODE[dt], numel, 64,
                                  _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _check(buf, numel, dt, coracle.dequant_bnb_single(p, single, numel, DT_CODE[dt]), f"bnb single {dt}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["5x2048", "7x192"])
def test_capped_grid_loop_kernel_equals_default(gpu, name, dt):
    """A call that names a grid cap (blocks_per_cu = 1) stays on nf4_flat_kernel, the kernel
    with the tile loop and the struct argument; byte for byte the default entry's output."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    m, n, p, a1, a2, _ = _inputs(name)
    tp, t1, t2 = (torch.from_numpy(a).to(gpu) for a in (p, a1, a2))
    new, old = _out(m * n, dt, gpu), _out(m * n, dt, gpu)
    _ref(L, tp, t1, t2, new, dt, m, n)
    _ref(L, tp, t1, t2, old, dt, m, n, _lib.LaunchCfg(4, 1, 1, 0))
    torch.cuda.synchronize()
    assert torch.equal(_bits_view(new, dt), _bits_view(old, dt)), f"{name} {dt}"
    assert not bool(torch.isnan(new[:m * n].float()).any())


def test_three_launches_in_one_graph(coracle, gpu):
    """Three default launches of 5x2048 captured on one stream: a linear chain, no parallel
    branches.  Replayed twice; every output equals the oracle's after each replay."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    m, n, p, a1, a2, _ = _inputs("5x2048")
    tp, t1, t2 = (torch.from_numpy(a).to(gpu) for a in (p, a1, a2))
    bufs = [_out(m * n, dt, gpu) for dt in DTS]
    for buf, dt in zip(bufs, DTS):  # every kernel loaded before the capture
        _ref(L, tp, t1, t2, buf, dt, m, n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for buf, dt in zip(bufs, DTS):
            _ref(L, tp, t1, t2, buf, dt, m, n)
    torch.cuda.synchronize()
    for _ in range(2):
        for buf, dt in zip(bufs, DTS):
            _bits_view(buf, dt)[:m * n] = NAN_BITS[dt]
        g.replay()
        torch.cuda.synchronize()
        for buf, dt in zip(bufs, DTS):
            _check(buf, m * n, dt, _want_ref(coracle, "5x2048", dt), f"graph replay {dt}")
