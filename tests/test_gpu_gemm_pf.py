"""The prefill fused GEMM in bitsandbytes semantics (nf4_gemm_bnb_pf, nf4_gemm_bnb_pf_single:
1..8192 rows) through the C ABI on the GPU (``-m gpu``).

N = 256, K = 768: two column tiles, 12 blocks per row (the blocksize2 = 256 boundary falls inside
a row), a non-zero offset.  Every product is judged against the float64 oracle of the C oracle's
exact 16-bit weights under the suite's GEMM bound; outputs are NaN-prefilled.  After every call
with a workspace the workspace reads 0 and nf4_gemm_check_workspace is clean.
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

N, K = 256, 768
PF, MT = 14, 8  # NF4DQ_GEMM_PF, NF4DQ_GEMM_MT
CFGS = [None] + [(w, k) for w in (4, 8) for k in (1, 3, 5)]  # five slices over 12 steps: the last one empty
_TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
_W = {}


def _weight(coracle, gpu, mode, dt):
    """(device operands, the oracle's 16-bit weight [N, K]) per (mode, dtype), made once."""
    if (mode, dt) not in _W:
        code = O.BF16 if dt == "bf16" else O.F16
        if mode == "nested":
            w = drawn_weight_bnb(N, K, seed=N + K)
            bits = coracle.dequant_bnb(*w, N * K, code, 64, 256)
            ops = [np.ascontiguousarray(v) for v in w[:4]] + [np.array([w[4]], np.float32)]
        else:
            w = single_weight_bnb(N, K, seed=N + K + 1)
            bits = coracle.dequant_bnb_single(*w, N * K, code, 64)
            ops = [np.ascontiguousarray(v) for v in w]
        _W[mode, dt] = ([torch.from_numpy(v).to(gpu) for v in ops], bits.reshape(N, K))
    return _W[mode, dt]


@functools.lru_cache(maxsize=None)
def _x(M, dt):
    return x_bits(M, K, dt, 11)


def _call(ops, dt, x_ptr, M, y_ptr, cfg=None, expect=0, n=N, blocksize=64, short=0):
    """One call on a fresh zeroed workspace (`short` bytes less than asked), left zero and clean."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    c = _lib.GemmCfg(cfg[2] if len(cfg) > 2 else PF, cfg[0], 1, cfg[1], 0) if cfg else None
    cp = ctypes.byref(c) if c else None
    wsz = L.nf4_gemm_bnb_pf_workspace_bytes(M, n, K, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=ops[0].device)
    sp = torch.cuda.current_stream().cuda_stream
    tail = (y_ptr, _lib.BF16 if dt == "bf16" else _lib.F16, n, K, ws.data_ptr() if wsz else None, wsz - short, cp, sp)
    p = [t.data_ptr() for t in ops]
    if len(ops) == 5:
        rc = L.nf4_gemm_bnb_pf(x_ptr, M, p[0], n * K // 2, p[1], ops[1].numel(), p[2], p[3], ops[3].numel(), p[4],
                               blocksize, 256, *tail)
    else:
        rc = L.nf4_gemm_bnb_pf_single(x_ptr, M, p[0], n * K // 2, p[1], ops[1].numel(), blocksize, *tail)
    assert rc == expect, (cfg, _lib.strerror(rc))
    if wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg}"
    return wsz


def _gemm(ops, dt, xd, M, cfg=None, band=0):
    buf = torch.full((M + band, N), float("nan"), dtype=_TDT[dt], device=xd.device)
    _call(ops, dt, xd.data_ptr(), M, buf.data_ptr(), cfg)
    return buf


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 255, 256, 257, 385])
def test_row_block_edges(coracle, gpu, dt, mode, M):
    """Rows around the 128- and 256-row block edges under the library's choice and both block
    heights with 1, 3 and 5 K slices; 64 sentinel rows behind row M - 1 stay as they were."""
    ops, bits = _weight(coracle, gpu, mode, dt)
    xt, xb = _x(M, dt)
    xd = xt.to(gpu)
    for cfg in CFGS:
        buf = _gemm(ops, dt, xd, M, cfg, band=64)
        assert bool(buf[M:].isnan().all()), f"rows past M written: M={M} cfg {cfg}"
        check_gemm(buf[:M], xb, bits, dt, f"M={M} {mode} {dt} cfg {cfg}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("ksplit", [1, 3])
def test_identity_rows_recover_the_exact_weights(coracle, gpu, dt, mode, ksplit):
    """x = rows k0 .. k0 + 255 of the identity: y[m][n] is W[n][k0 + m] plus exact zeros and equals
    the oracle's weight by value, with no tolerance."""
    ops, bits = _weight(coracle, gpu, mode, dt)
    want = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu).view(_TDT[dt])
    eye = torch.eye(K, dtype=_TDT[dt], device=gpu)
    for waves in (4, 8):
        rec = torch.cat([_gemm(ops, dt, eye[k0:k0 + 256].contiguous(), 256, (waves, ksplit)).t() for k0 in (0, 256, 512)], 1)
        ok = rec == want
        assert bool(ok.all()), f"waves {waves}: {int((~ok).sum())} weights differ, first at {(~ok).nonzero()[0].tolist()}"


@pytest.mark.parametrize("cfg", [(4, 1), (4, 3), (8, 1), (8, 5)])
def test_a_row_does_not_see_its_batch(coracle, gpu, cfg):
    """Under one cfg y[:129] of the M = 385 call equals the M = 129 call bit for bit, twice."""
    ops, _ = _weight(coracle, gpu, "nested", "bf16")
    xd = _x(385, "bf16")[0].to(gpu)
    big, small, again = (_gemm(ops, "bf16", xd, M, cfg).view(torch.int16) for M in (385, 129, 129))
    assert torch.equal(big[:129], small) and torch.equal(small, again)


@pytest.mark.parametrize("case,kw,code", [
    ("M8193", dict(M=8193), "ERR_SHAPE"), ("N192", dict(n=192), "ERR_SHAPE"), ("blocksize128", dict(blocksize=128), "ERR_SHAPE"),
    ("null_x", dict(x=None), "ERR_ARG"), ("waves2", dict(cfg=(2, 1)), "ERR_ARG"), ("ksplit13", dict(cfg=(4, 13)), "ERR_ARG"),
    ("names_mt", dict(cfg=(4, 1, MT)), "ERR_ARG"), ("short_workspace", dict(cfg=(4, 3), short=16), "ERR_ARG"),
    ("M0", dict(M=0), "OK")])
def test_status_codes_come_before_any_launch(coracle, gpu, case, kw, code):
    from nf4_triton_dequantization_amd import _lib

    ops, _ = _weight(coracle, gpu, "nested", "bf16")
    xd = _x(129, "bf16")[0].to(gpu)
    y = torch.full((129, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    kw = dict(kw)
    x_ptr = kw.pop("x", xd.data_ptr())
    _call(ops, "bf16", x_ptr, kw.pop("M", 129), y.data_ptr(), kw.pop("cfg", None), expect=getattr(_lib, code), **kw)
    torch.cuda.synchronize()
    assert bool(y.isnan().all()), f"{case}: y written"
