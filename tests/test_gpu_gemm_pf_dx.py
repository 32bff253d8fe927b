"""The fused input-gradient GEMM dx = g . W in bitsandbytes semantics (nf4_gemm_bnb_pf_dx,
nf4_gemm_bnb_pf_dx_single: 1..8192 rows) through the C ABI on the GPU (``-m gpu``).

N = 448, K = 384: seven reduction steps (N no multiple of 128), three column tiles, six blocks per
weight row, so the blocksize2 = 256 boundaries fall inside rows and inside steps and the last
group is partial; a non-zero offset.  Every product is judged against the float64 oracle of the C
oracle's exact 16-bit weights under the suite's GEMM bound; outputs are NaN-prefilled.  After every
call with a workspace the workspace reads 0 and nf4_gemm_check_workspace is clean.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_bnb_cases import drawn_weight_bnb, single_weight_bnb
from _gemm_cases import check_gemm, x_bits

pytestmark = pytest.mark.gpu

N, K = 448, 384
DX = 15  # NF4DQ_GEMM_PF_DX
CFGS = [None, (4, 1), (4, 3), (8, 1), (8, 5)]  # five slices over seven steps: the last one empty
_TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
_W = {}


def _weight(coracle, gpu, mode, dt):
    """(device operands, the oracle's 16-bit weight [N, K]) per (mode, dtype), made once."""
    if (mode, dt) not in _W:
        code = O.BF16 if dt == "bf16" else O.F16
        if mode == "nested":
            w = drawn_weight_bnb(N, K, seed=N + K)
            assert w[4] != 0.0
            bits = coracle.dequant_bnb(*w, N * K, code, 64, 256)
            ops = [np.ascontiguousarray(v) for v in w[:4]] + [np.array([w[4]], np.float32)]
        else:
            w = single_weight_bnb(N, K, seed=N + K + 1)
            bits = coracle.dequant_bnb_single(*w, N * K, code, 64)
            ops = [np.ascontiguousarray(v) for v in w]
        _W[mode, dt] = ([torch.from_numpy(v).to(gpu) for v in ops], bits.reshape(N, K))
    return _W[mode, dt]


@functools.lru_cache(maxsize=None)
def _g(M, dt):
    return x_bits(M, N, dt, 13)


def _call(ops, dt, g_ptr, M, dx_ptr, cfg=None, expect=0, n=N, k=K, blocksize=64, short=0):
    """One call on a fresh zeroed workspace (`short` bytes less than asked), left zero and clean."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    c = _lib.GemmCfg(DX, cfg[0], 1, cfg[1], 0) if cfg else None
    cp = ctypes.byref(c) if c else None
    wsz = L.nf4_gemm_bnb_pf_dx_workspace_bytes(M, n, k, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=ops[0].device)
    sp = torch.cuda.current_stream().cuda_stream
    tail = (dx_ptr, _lib.BF16 if dt == "bf16" else _lib.F16, n, k, ws.data_ptr() if wsz else None, wsz - short, cp, sp)
    p = [t.data_ptr() for t in ops]
    if len(ops) == 5:
        rc = L.nf4_gemm_bnb_pf_dx(g_ptr, M, p[0], n * k // 2, p[1], ops[1].numel(), p[2], p[3], ops[3].numel(), p[4],
                                  blocksize, 256, *tail)
    else:
        rc = L.nf4_gemm_bnb_pf_dx_single(g_ptr, M, p[0], n * k // 2, p[1], ops[1].numel(), blocksize, *tail)
    assert rc == expect, (cfg, _lib.strerror(rc))
    if wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg}"
    return wsz


def _gemm(ops, dt, gd, M, cfg=None, band=0):
    buf = torch.full((M + band, K), float("nan"), dtype=_TDT[dt], device=gd.device)
    _call(ops, dt, gd.data_ptr(), M, buf.data_ptr(), cfg)
    return buf


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 257])
def test_row_block_edges(coracle, gpu, dt, mode, M):
    """Rows around the 128- and 256-row block edges under the library's choice and both block
    heights with one slice and with 3 / 5; 64 sentinel rows behind row M - 1 stay as they were."""
    ops, bits = _weight(coracle, gpu, mode, dt)
    gt, gb = _g(M, dt)
    gd = gt.to(gpu)
    for cfg in CFGS:
        buf = _gemm(ops, dt, gd, M, cfg, band=64)
        assert bool(buf[M:].isnan().all()), f"rows past M written: M={M} cfg {cfg}"
        check_gemm(buf[:M], gb, np.ascontiguousarray(bits.T), dt, f"M={M} {mode} {dt} cfg {cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("slices", [1, 3])
def test_identity_rows_recover_the_exact_weights(coracle, gpu, dt, mode, slices):
    """g = rows n0 .. n0 + 127 of the identity: dx[m][k] is W[n0 + m][k] plus exact zeros and equals
    the oracle's weight by value, with no tolerance: the transposition, the slot permutation and
    the block a scale is taken from."""
    ops, bits = _weight(coracle, gpu, mode, dt)
    want = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu).view(_TDT[dt])
    eye = torch.eye(N, dtype=_TDT[dt], device=gpu)
    for waves in (4, 8):
        for n0 in (0, 128, 256, 320):
            ok = _gemm(ops, dt, eye[n0:n0 + 128].contiguous(), 128, (waves, slices)) == want[n0:n0 + 128]
            assert bool(ok.all()), (f"waves {waves} n0 {n0}: {int((~ok).sum())} weights differ, "
                                    f"first at {(~ok).nonzero()[0].tolist()}")


@pytest.mark.parametrize("cfg", [(4, 1), (4, 3), (8, 1), (8, 5)])
def test_a_row_does_not_see_its_batch(coracle, gpu, cfg):
    """Under one cfg two M = 257 calls give equal bits, and rows 0, 130 and 256 of them are the
    M = 1 call on that row."""
    ops, _ = _weight(coracle, gpu, "nested", "bf16")
    gd = _g(257, "bf16")[0].to(gpu)
    big, again = (_gemm(ops, "bf16", gd, 257, cfg).view(torch.int16) for _ in range(2))
    assert torch.equal(big, again)
    for m in (0, 130, 256):
        assert torch.equal(_gemm(ops, "bf16", gd[m:m + 1], 1, cfg).view(torch.int16), big[m:m + 1]), m


@pytest.mark.parametrize("case,kw,code", [
    ("K320", dict(k=320), "ERR_SHAPE"), ("N416", dict(n=416), "ERR_SHAPE"), ("blocksize128", dict(blocksize=128), "ERR_SHAPE"),
    ("M8193", dict(M=8193), "ERR_SHAPE"), ("misaligned_g", dict(g_off=8), "ERR_ARG"),
    ("short_workspace", dict(cfg=(4, 3), short=16), "ERR_ARG")])
def test_status_codes_come_before_any_launch(coracle, gpu, case, kw, code):
    from nf4_triton_dequantization_amd import _lib

    ops, _ = _weight(coracle, gpu, "nested", "bf16")
    gd = _g(129, "bf16")[0].to(gpu)
    dx = torch.full((129, K), float("nan"), dtype=torch.bfloat16, device=gpu)
    kw = dict(kw)
    _call(ops, "bf16", gd.data_ptr() + kw.pop("g_off", 0), kw.pop("M", 129), dx.data_ptr(), kw.pop("cfg", None),
          expect=getattr(_lib, code), **kw)
    torch.cuda.synchronize()
    assert bool(dx.isnan().all()), f"{case}: dx written"
