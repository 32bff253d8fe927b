"""The row-tiled fused GEMM in bitsandbytes semantics (nf4_gemm_bnb_mt, nf4_gemm_bnb_mt_single:
1..128 rows) through the C ABI on the GPU (``-m gpu``).

Every product is judged against the float64 oracle of the C oracle's exact 16-bit weights with
the suite's GEMM bound (``_gemm_cases.tol`` through ``check_gemm`` / ``check_close``); outputs
are NaN-prefilled, so a value never stored fails.  The exact-weight tests use the identity
walk of test_gpu_gemm_bnb.py: x = rows of the identity, so every output is one weight plus
exact zeros, compared with the oracle's weight by value with no tolerance (-0 == +0, the sum's
own zero; NaN equal to nothing).

After every call that had a workspace: the whole workspace reads 0 again (tickets and slabs)
and nf4_gemm_check_workspace is clean.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_bnb_cases import BLOCKSIZE2, drawn_weight_bnb, sensitive_weight_bnb, single_weight_bnb
from _gemm_cases import bits_to_f64, check_close, check_gemm, gemm_oracle, x_bits

pytestmark = pytest.mark.gpu

MT = 8  # NF4DQ_GEMM_MT


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _code(dt):
    return O.BF16 if dt == "bf16" else O.F16


def _lib_and_L():
    from nf4_triton_dequantization_amd import _lib

    return _lib, _lib.lib()


def _cfg(waves, ksplit):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(MT, waves, 1, ksplit, 2)


class _Weight:
    """A weight on the device with the oracle's 16-bit matrix [N, K] (host bits and, lazily, a
    device tensor).  mode: "nested" (packed, a1, code2, a2, offset) or "single" (packed, absmax)."""

    def __init__(self, coracle, gpu, mode, w, N, K, dt, bs2=256):
        self.mode, self.N, self.K, self.dt, self.bs2, self.gpu = mode, N, K, dt, bs2, gpu
        if mode == "nested":
            packed, a1, code2, a2, offset = w[:5]
            self.bits = coracle.dequant_bnb(packed, a1, code2, a2, offset, N * K, _code(dt), 64, bs2).reshape(N, K)
            self.t = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (packed, a1, code2, a2)]
            self.t.append(torch.tensor([offset], dtype=torch.float32, device=gpu))
        else:
            packed, absmax = w
            self.bits = coracle.dequant_bnb_single(packed, absmax, N * K, _code(dt), 64).reshape(N, K)
            self.t = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (packed, absmax)]
        assert np.isfinite(bits_to_f64(self.bits, dt)).all()

    def want(self):
        return torch.from_numpy(np.ascontiguousarray(self.bits).view(np.int16)).to(self.gpu).view(_tdt(self.dt))


_CACHE = {}


def _weight(coracle, gpu, mode, kind, N, K, dt):
    """One weight per (mode, kind, shape, dtype) for the whole module, never changed."""
    key = (mode, kind, N, K, dt)
    if key not in _CACHE:
        if mode == "single":
            _CACHE[key] = _Weight(coracle, gpu, mode, single_weight_bnb(N, K, seed=N + K + 1), N, K, dt)
        elif kind == "sensitive":
            _CACHE[key] = _Weight(coracle, gpu, mode, sensitive_weight_bnb(N, K, dt)[:5], N, K, dt, BLOCKSIZE2)
        else:
            _CACHE[key] = _Weight(coracle, gpu, mode, drawn_weight_bnb(N, K, seed=N + K), N, K, dt)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def _x(M, K, dt, seed=11):
    return x_bits(M, K, dt, seed)


def _call(W, x_ptr, M, y_ptr, cfg=None, ws=None, expect=0):
    """One call; with ws None a fresh zeroed workspace, checked clean and zero afterwards."""
    _lib, L = _lib_and_L()
    cp = ctypes.byref(cfg) if cfg is not None else None
    wsz = L.nf4_gemm_bnb_mt_workspace_bytes(M, W.N, W.K, cp)
    own = ws is None
    if own:
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=W.gpu)
    assert ws.numel() >= wsz
    sp = torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 if W.dt == "bf16" else _lib.F16
    wp = ws.data_ptr() if wsz else None
    if W.mode == "nested":
        q, a1, c2, a2, off = W.t
        rc = L.nf4_gemm_bnb_mt(x_ptr, M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                               a2.data_ptr(), a2.numel(), off.data_ptr(), 64, W.bs2, y_ptr, code, W.N, W.K, wp, wsz,
                               cp, sp)
    else:
        q, am = W.t
        rc = L.nf4_gemm_bnb_mt_single(x_ptr, M, q.data_ptr(), q.numel(), am.data_ptr(), am.numel(), 64, y_ptr, code,
                                      W.N, W.K, wp, wsz, cp, sp)
    assert rc == expect, (cfg and (cfg.waves, cfg.ksplit), _lib.strerror(rc))
    if own and wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg and (cfg.waves, cfg.ksplit)}"
    return wsz


def _gemm(W, xd, M, cfg=None):
    y = torch.full((M, W.N), float("nan"), dtype=_tdt(W.dt), device=W.gpu)
    _call(W, xd.data_ptr(), M, y.data_ptr(), cfg)
    return y


# ---- row-tile edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 48, 64, 65, 100, 127, 128])
def test_row_tile_edges(coracle, gpu, dt, mode, M):
    """N = 192, K = 768: 12 blocks per row, so the 256-block boundary of blocksize2 falls inside
    a row (row 21, block 4); a non-zero offset.  The library's choice (64-column workgroups, one
    K slice: the direct stores' rows) and three K slices (the slab's and the reducer's rows)."""
    N, K = 192, 768
    W = _weight(coracle, gpu, mode, "drawn", N, K, dt)
    if mode == "nested":
        assert W.t[3].numel() == N * K // 64 // 256 and float(W.t[4]) != 0.0
    xt, xb = _x(M, K, dt)
    xd = xt.to(gpu)
    check_gemm(_gemm(W, xd, M), xb, W.bits, dt, f"library choice M={M} {mode} {dt}")
    check_gemm(_gemm(W, xd, M, _cfg(2, 3)), xb, W.bits, dt, f"three K slices M={M} {mode} {dt}")


# ---- K forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [40, 128])
@pytest.mark.parametrize("K", [128, 384, 4096])
def test_k_forms_every_ksplit(coracle, gpu, dt, M, K):
    """N = 64; K = 128 (one chunk), 384 (three), 4096 (32): every ksplit the plan admits,
    1 .. min(K / 128, 16) -- among them splits that do not divide the chunk count (K = 384: 2
    slices of 2 + 1 chunks; K = 4096: 5 slices of 7, the last of 4; 12 .. 15 slices of 3 chunks,
    the last ones EMPTY) and the maximum -- and the library's own choice."""
    _lib, L = _lib_and_L()
    N = 64
    W = _weight(coracle, gpu, "nested", "drawn", N, K, dt)
    xt, xb = _x(M, K, dt)
    xd = xt.to(gpu)
    ref, bound = gemm_oracle(xb, W.bits, dt)
    chunks = K // 128
    top = min(chunks, 16)
    for ks in list(range(1, top + 1)) + [None]:
        y = _gemm(W, xd, M, None if ks is None else _cfg(2, ks))
        yb = y.view(torch.int16).cpu().numpy().view(np.uint16)
        check_close(bits_to_f64(yb, dt), ref, bound, f"K={K} M={M} ksplit={ks} {dt}")
    # one more slice than the plan admits, and 128-column workgroups over 64 columns: the caller's error
    y = torch.empty((M, N), dtype=_tdt(dt), device=gpu)
    for bad in (_cfg(2, top + 1), _cfg(4, 1), _cfg(2, 0)):
        _call(W, xd.data_ptr(), M, y.data_ptr(), bad, expect=_lib.ERR_ARG)


# ---- exact weights --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_identity_windows_recover_the_exact_weights(coracle, gpu, dt):
    """x = rows k0 .. k0 + 127 of the identity over sensitive_weight_bnb(64, 256): y[m][n] is
    W[n][k0 + m] plus exact zeros and must equal the oracle's 16-bit weight.  A fused
    multiply-add in the scale or a single rounding of the last product changes 16-bit values in
    this weight; it is asymmetric, so a swapped row / column or a permuted k shows too.  The
    library's choice (one K slice), two slices, and the single-statistics mode on a drawn weight."""
    N, K, M = 64, 256, 128
    eye = torch.eye(K, dtype=_tdt(dt), device=gpu)
    for W in (_weight(coracle, gpu, "nested", "sensitive", N, K, dt), _weight(coracle, gpu, "single", "drawn", N, K, dt)):
        want = W.want()
        for cfg in (None, _cfg(2, 2)):
            rec = torch.empty((N, K), dtype=_tdt(dt), device=gpu)
            for k0 in range(0, K, M):
                rec[:, k0:k0 + M] = _gemm(W, eye[k0:k0 + M], M, cfg).t()
            ok = rec == want
            assert bool(ok.all()), (f"{W.mode} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}: {int((~ok).sum())} of "
                                    f"{ok.numel()} weights differ, first at {(~ok).nonzero()[0].tolist()}")


# ---- guard bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [33, 127])
def test_nothing_outside_y_changes_and_nothing_past_x_is_used(coracle, gpu, dt, M):
    """y sits between two sentinel bands of 64 rows in one allocation; x is the head of a
    128-row buffer whose tail is NaN.  N = 128, K = 256: the library's choice (128-column
    workgroups, one K slice), 128 columns with two slices, 64 columns with two."""
    N, K, band = 128, 256, 64
    W = _weight(coracle, gpu, "nested", "drawn", N, K, dt)
    xt, xb = _x(M, K, dt)
    xbuf = torch.full((128, K), float("nan"), dtype=_tdt(dt), device=gpu)
    xbuf[:M] = xt.to(gpu)
    for cfg in (None, _cfg(4, 2), _cfg(2, 2)):
        buf = torch.full((band + M + band, N), 0x5A5B, dtype=torch.int16, device=gpu)
        buf[band:band + M] = torch.full((M, N), float("nan"), dtype=_tdt(dt), device=gpu).view(torch.int16)
        y = buf[band:band + M].view(_tdt(dt))
        _call(W, xbuf.data_ptr(), M, y.data_ptr(), cfg)
        what = f"M={M} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}"
        assert bool((buf[:band] == 0x5A5B).all()) and bool((buf[band + M:] == 0x5A5B).all()), f"band written: {what}"
        check_gemm(y, xb, W.bits, dt, what)


# ---- reproducible and re-entrant -------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_same_call_twice_on_one_workspace_gives_the_same_bits(coracle, gpu, dt):
    """N = 256, K = 1024, M = 100 (128-column workgroups, 4 K slices) twice on one workspace
    with another shape (N = 64, K = 384, M = 40, three slices) in between: identical bits, the
    workspace all zero after each call, nf4_gemm_check_workspace clean."""
    _lib, L = _lib_and_L()
    A = _weight(coracle, gpu, "nested", "drawn", 256, 1024, dt)
    B = _weight(coracle, gpu, "nested", "drawn", 64, 384, dt)
    (xa, xab), (xb_, xbb) = _x(100, 1024, dt), _x(40, 384, dt)
    xa, xb_ = xa.to(gpu), xb_.to(gpu)
    ca, cb = _cfg(4, 4), _cfg(2, 3)
    need = max(L.nf4_gemm_bnb_mt_workspace_bytes(100, 256, 1024, ctypes.byref(ca)),
               L.nf4_gemm_bnb_mt_workspace_bytes(40, 64, 384, ctypes.byref(cb)))
    assert need == 64 * 1024 + 256 + 4 * 100 * 256 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    sp = torch.cuda.current_stream().cuda_stream
    ys = []
    for W, xd, M, cfg in ((A, xa, 100, ca), (B, xb_, 40, cb), (A, xa, 100, ca)):
        y = torch.full((M, W.N), float("nan"), dtype=_tdt(dt), device=gpu)
        _call(W, xd.data_ptr(), M, y.data_ptr(), cfg, ws=ws)
        assert int(ws.count_nonzero()) == 0, "tickets or slab entries left set"
        ys.append(y)
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), sp) == 0
    check_gemm(ys[0], xab, A.bits, dt, f"first call {dt}")
    check_gemm(ys[1], xbb, B.bits, dt, f"other shape {dt}")
    assert torch.equal(ys[0].view(torch.int16), ys[2].view(torch.int16))


# ---- subnormal weights ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,scale", [("f16", 1e-4), ("bf16", 1e-37)])
def test_subnormal_weights_come_through_exactly(coracle, gpu, dt, scale):
    """As test_gpu_gemm_bnb.py::test_subnormal_weights_come_through_exactly, at M = 64: more
    than half the 16-bit weights subnormal, recovered by the identity walk (N = 64, K = 2048)."""
    N, K, M = 64, 2048, 64
    W = _Weight(coracle, gpu, "nested", drawn_weight_bnb(N, K, seed=7, subnormal_scale=scale), N, K, dt)
    bits = W.bits
    exp = (bits & 0x7C00) if dt == "f16" else (bits & 0x7F80)
    sub = (exp == 0) & ((bits & 0x7FFF) != 0)
    assert sub.mean() > 0.5
    eye = torch.eye(K, dtype=_tdt(dt), device=gpu)
    rec = torch.empty((N, K), dtype=_tdt(dt), device=gpu)
    for k0 in range(0, K, M):
        rec[:, k0:k0 + M] = _gemm(W, eye[k0:k0 + M], M).t()
    ok = rec == W.want()
    assert bool(ok.all()), f"{int((~ok).sum())} of {ok.numel()} weights differ, first at {(~ok).nonzero()[0].tolist()}"
