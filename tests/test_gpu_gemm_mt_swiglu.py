"""The fused gate/up SwiGLU launch (nf4_gemm_bnb_mt_swiglu: 1..128 rows) through the C ABI on the
GPU (``-m gpu``).

h = rn(rn(silu(g)) * u) with g and u what nf4_gemm_bnb_mt stores for the gate and the up weight.
Elementwise checks use the acceptance set of _swiglu_cases.py, computed on the CPU from reference
bits only (``s`` must be ``rn`` of the float64 silu, either neighbour within 2^-21 relative of a
rounding tie; ``h`` exactly ``rn(s * u)``; at most 1 % near-tie elements).  Products are judged
against the float64 chain of the float64 GEMMs of the C oracle's exact weights
(``swiglu_oracle``).  h is NaN-prefilled, so a value never stored fails.

After every call that had a workspace: the whole workspace reads 0 again (tickets and planes) and
nf4_gemm_check_workspace is clean.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_bnb_cases import code2_np, drawn_weight_bnb, single_weight_bnb
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits
from _swiglu_cases import accept, swiglu_oracle

pytestmark = pytest.mark.gpu

SG = 10  # NF4DQ_GEMM_MT_SWIGLU
MT = 8   # NF4DQ_GEMM_MT


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _code(dt):
    return O.BF16 if dt == "bf16" else O.F16


def _lib_and_L():
    from nf4_triton_dequantization_amd import _lib

    return _lib, _lib.lib()


def _cfg(waves, ksplit, kernel=SG):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(kernel, waves, 1, ksplit, 2)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class _Weight:
    """A weight on the device with the oracle's 16-bit matrix [I, K].  mode: "nested" (packed, a1,
    code2, a2, offset; blocksize2 ``bs2``) or "single" (packed, absmax)."""

    def __init__(self, coracle, gpu, mode, w, I, K, dt, bs2=256):
        self.mode, self.N, self.K, self.dt, self.bs2, self.gpu = mode, I, K, dt, bs2, gpu
        if mode == "nested":
            packed, a1, code2, a2, offset = w
            self.bits = coracle.dequant_bnb(packed, a1, code2, a2, offset, I * K, _code(dt), 64, bs2).reshape(I, K)
            self.t = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (packed, a1, code2, a2)]
            self.t.append(torch.tensor([offset], dtype=torch.float32, device=gpu))
        else:
            packed, absmax = w
            self.bits = coracle.dequant_bnb_single(packed, absmax, I * K, _code(dt), 64).reshape(I, K)
            self.t = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (packed, absmax)]
        assert np.isfinite(bits_to_f64(self.bits, dt)).all()

    def mat(self):
        _lib, _ = _lib_and_L()
        if self.mode == "nested":
            q, a1, c2, a2, off = self.t
            return _lib.GemmBnbMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(), a2.data_ptr(),
                                   a2.numel(), off.data_ptr(), 64, self.bs2, None, self.N)
        q, am = self.t
        return _lib.GemmBnbMat(q.data_ptr(), q.numel(), None, 0, None, am.data_ptr(), am.numel(), None, 64, 0, None, self.N)


_CACHE = {}


def _pair(coracle, gpu, mode, I, K, dt, scale=None):
    """(gate, up) for the whole module, never changed.  Nested: the gate weight has the dynamic map,
    offset 0.0123 and blocksize2 256, the up weight the map reversed and scaled by 0.75, offset
    -0.0371 and blocksize2 16 -- a kernel that used one weight's table, offset or blocksize2 for
    the other would not reproduce the oracle's weights.  ``scale`` multiplies both weights'
    statistics (the |g| = 40 case)."""
    key = (mode, I, K, dt, scale)
    if key not in _CACHE:
        f = np.float32(1.0 if scale is None else scale)
        if mode == "single":
            ws = []
            for seed in (I + K + 1, I + K + 2):
                packed, absmax = single_weight_bnb(I, K, seed=seed)
                ws.append(_Weight(coracle, gpu, mode, (packed, (absmax * f).astype(np.float32)), I, K, dt))
        else:
            p, a1, c2, a2, off = drawn_weight_bnb(I, K, seed=I + K)
            gate = _Weight(coracle, gpu, mode, (p, a1, c2, (a2 * f).astype(np.float32), float(np.float32(off) * f)), I, K, dt)
            p, a1, _, a2, _ = drawn_weight_bnb(I, K, seed=I + K + 5, blocksize2=16)
            c2u = (code2_np()[::-1] * np.float32(0.75)).astype(np.float32).copy()
            up = _Weight(coracle, gpu, mode, (p, a1, c2u, (a2 * f).astype(np.float32), float(np.float32(-0.0371) * f)),
                         I, K, dt, bs2=16)
            ws = [gate, up]
        _CACHE[key] = tuple(ws)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def _x(M, K, dt, seed=11):
    return x_bits(M, K, dt, seed)


def _call(G, U, x_ptr, M, h_ptr, cfg=None, ws=None, expect=0):
    """One call; with ws None a fresh zeroed workspace, checked clean and zero afterwards."""
    _lib, L = _lib_and_L()
    assert G.mode == U.mode and (G.N, G.K, G.dt) == (U.N, U.K, U.dt)
    cp = ctypes.byref(cfg) if cfg is not None else None
    wsz = L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(M, G.N, G.K, cp)
    own = ws is None
    if own:
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=G.gpu)
    assert ws.numel() >= wsz
    sp = torch.cuda.current_stream().cuda_stream
    mats = (_lib.GemmBnbMat * 2)(G.mat(), U.mat())
    rc = L.nf4_gemm_bnb_mt_swiglu(x_ptr, M, G.K, ctypes.cast(mats, ctypes.c_void_p), 1 if G.mode == "single" else 0,
                                  _lib.ACT_SILU, h_ptr, _lib.BF16 if G.dt == "bf16" else _lib.F16,
                                  ws.data_ptr() if wsz else None, wsz, cp, sp)
    assert rc == expect, (cfg and (cfg.waves, cfg.ksplit), _lib.strerror(rc))
    if own and wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or plane entries left set, cfg {cfg and (cfg.waves, cfg.ksplit)}"
    return wsz


def _swiglu(G, U, xd, M, cfg=None):
    h = torch.full((M, G.N), float("nan"), dtype=_tdt(G.dt), device=G.gpu)
    _call(G, U, xd.data_ptr(), M, h.data_ptr(), cfg)
    return h


def _mt(W, xd, M, ksplit):
    """nf4_gemm_bnb_mt / _single of one weight with `ksplit` K slices (64-column workgroups)."""
    _lib, L = _lib_and_L()
    cfg = _cfg(2, ksplit, MT)
    cp = ctypes.byref(cfg)
    wsz = L.nf4_gemm_bnb_mt_workspace_bytes(M, W.N, W.K, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=W.gpu)
    y = torch.full((M, W.N), float("nan"), dtype=_tdt(W.dt), device=W.gpu)
    sp = torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 if W.dt == "bf16" else _lib.F16
    wp = ws.data_ptr() if wsz else None
    if W.mode == "nested":
        q, a1, c2, a2, off = W.t
        rc = L.nf4_gemm_bnb_mt(xd.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                               a2.data_ptr(), a2.numel(), off.data_ptr(), 64, W.bs2, y.data_ptr(), code, W.N, W.K, wp,
                               wsz, cp, sp)
    else:
        q, am = W.t
        rc = L.nf4_gemm_bnb_mt_single(xd.data_ptr(), M, q.data_ptr(), q.numel(), am.data_ptr(), am.numel(), 64,
                                      y.data_ptr(), code, W.N, W.K, wp, wsz, cp, sp)
    assert rc == 0, _lib.strerror(rc)
    return y


def _check_chain(h, xb, G, U, dt, what):
    """h against the float64 chain of the float64 GEMMs (swiglu_oracle's derivation)."""
    (gr, gt), (ur, ut) = gemm_oracle(xb, G.bits, dt), gemm_oracle(xb, U.bits, dt)
    ref, bound = swiglu_oracle(gr, gt, ur, ut, dt)
    check_close(bits_to_f64(_bits(h), dt).reshape(ref.shape), ref, bound, what)


# ---- exact weights --------------------------------------------------------------------------------
def _identity_walk(G, U, gpu, dt, cfgs, what):
    """x = rows k0 .. k0 + 127 of the identity: g[m][n] = Wg[n][k0 + m] and u[m][n] = Wu[n][k0 + m]
    plus exact zeros, so h must lie in the acceptance set of the oracle's own bits.  (A weight
    that is -0 -- the code 0.0 under a negative scale -- comes out of the sum as +0, the sum's
    own zero, as in test_gpu_gemm_mt.py: g and u are taken as +0 there.)"""
    I, K, M = G.N, G.K, 128
    eye = torch.eye(K, dtype=_tdt(dt), device=gpu)
    g, u = (np.where(b == 0x8000, np.uint16(0), b) for b in (G.bits, U.bits))
    for cfg in cfgs:
        rec = np.empty((I, K), np.uint16)
        for k0 in range(0, K, M):
            rec[:, k0:k0 + M] = _bits(_swiglu(G, U, eye[k0:k0 + M], M, cfg)).T
        accept(rec, g, u, dt, f"{what} cfg {cfg and (cfg.waves, cfg.ksplit)}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
def test_identity_windows_give_the_chain_of_the_exact_weights(coracle, gpu, dt, mode):
    """I = 64, K = 256.  Gate and up have different code2 tables, offsets and blocksize2 (_pair).
    The library's choice (one K slice: the lane-local epilogue), two slices with two waves (the
    reducer's epilogue) and, on a second shape, I = 128 and K = 128 (one chunk)."""
    G, U = _pair(coracle, gpu, mode, 64, 256, dt)
    if mode == "nested":
        assert G.bs2 != U.bs2 and float(G.t[4]) != float(U.t[4]) and not torch.equal(G.t[2], U.t[2])
    assert not np.array_equal(G.bits, U.bits)
    _identity_walk(G, U, gpu, dt, (None, _cfg(2, 2)), f"{mode} {dt}")
    G, U = _pair(coracle, gpu, mode, 128, 128, dt)
    _identity_walk(G, U, gpu, dt, (None,), f"{mode} {dt} one chunk")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_identity_windows_with_g_reaching_40(coracle, gpu, dt):
    """The statistics (absmax2 and the offset) scaled so that the largest gate weight is 44: |g|
    reaches 40 with both signs (silu saturates to g on one side and underflows towards -0 on the
    other), and |u| grows with it."""
    G1, _ = _pair(coracle, gpu, "nested", 64, 256, dt)
    scale = float(np.float32(44.0 / np.abs(bits_to_f64(G1.bits, dt)).max()))
    G, U = _pair(coracle, gpu, "nested", 64, 256, dt, scale=scale)
    g = bits_to_f64(G.bits, dt)
    assert g.max() >= 40 and g.min() <= -40 and np.abs(bits_to_f64(U.bits, dt)).max() >= 20
    _identity_walk(G, U, gpu, dt, (None, _cfg(4, 2)), f"scaled {dt}")


# ---- row-tile edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 64, 65, 127, 128])
def test_row_tile_edges(coracle, gpu, dt, mode, M):
    """I = 192, K = 1152 (9 chunks): every row-tile count and the rows around their edges, the
    library's choice (four waves, one K slice: the direct stores' rows) and three K slices with two
    waves (the planes' and the reducer's rows).  h is judged against the float64 chain of the
    float64 GEMMs: the suite's gemm_oracle bound for g and u, propagated through the chain with
    |silu'| <= 1.1, plus one 16-bit ulp of |h| (swiglu_oracle has the derivation)."""
    I, K = 192, 1152
    G, U = _pair(coracle, gpu, mode, I, K, dt)
    xt, xb = _x(M, K, dt)
    xd = xt.to(gpu)
    _check_chain(_swiglu(G, U, xd, M), xb, G, U, dt, f"library choice M={M} {mode} {dt}")
    _check_chain(_swiglu(G, U, xd, M, _cfg(2, 3)), xb, G, U, dt, f"three K slices M={M} {mode} {dt}")


# ---- same slices, same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("ksplit", [1, 2, 4])
def test_same_slices_give_the_chain_of_the_row_tiled_outputs(coracle, gpu, dt, mode, ksplit):
    """nf4_gemm_bnb_mt twice and nf4_gemm_bnb_mt_swiglu once with the same ksplit at K = 1152 (9
    chunks: 5 + 4 at two slices; 3 + 3 + 3 and an EMPTY slice at four), I = 192, M = 100: the sums
    run in the same order, so h must lie in the acceptance set of the two row-tiled outputs' bits,
    element for element -- with two and with four waves."""
    I, K, M = 192, 1152, 100
    G, U = _pair(coracle, gpu, mode, I, K, dt)
    xd = _x(M, K, dt)[0].to(gpu)
    g, u = _bits(_mt(G, xd, M, ksplit)), _bits(_mt(U, xd, M, ksplit))
    for waves in (2, 4):
        h = _swiglu(G, U, xd, M, _cfg(waves, ksplit))
        accept(_bits(h), g, u, dt, f"ksplit {ksplit} waves {waves} {mode} {dt}")


# ---- weight order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gate_and_up_are_not_interchangeable(coracle, gpu, dt):
    """h(gate, up) differs from h(up, gate) on the drawn weights, and each is the chain of its own
    row-tiled outputs (I = 128, K = 256, M = 33, one K slice)."""
    I, K, M = 128, 256, 33
    G, U = _pair(coracle, gpu, "nested", I, K, dt)
    xd = _x(M, K, dt)[0].to(gpu)
    g, u = _bits(_mt(G, xd, M, 1)), _bits(_mt(U, xd, M, 1))
    h_gu, h_ug = _bits(_swiglu(G, U, xd, M, _cfg(4, 1))), _bits(_swiglu(U, G, xd, M, _cfg(4, 1)))
    assert (h_gu != h_ug).mean() > 0.9
    accept(h_gu, g, u, dt, f"(gate, up) {dt}")
    accept(h_ug, u, g, dt, f"(up, gate) {dt}")


# ---- guard bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [33, 127])
def test_nothing_outside_h_and_the_workspace_changes(coracle, gpu, dt, M):
    """h and the workspace each sit between two 64 KiB bands of a fixed pattern in one allocation
    (the method of test_gpu_redzones_bnb.py); x is the head of a 128-row buffer whose tail is NaN.
    I = 128, K = 256: the library's choice, four waves with two slices, two waves with two."""
    _lib, L = _lib_and_L()
    I, K, band = 128, 256, 64 * 1024
    G, U = _pair(coracle, gpu, "nested", I, K, dt)
    xt, xb = _x(M, K, dt)
    xbuf = torch.full((128, K), float("nan"), dtype=_tdt(dt), device=gpu)
    xbuf[:M] = xt.to(gpu)
    sp = torch.cuda.current_stream().cuda_stream
    for cfg in (None, _cfg(4, 2), _cfg(2, 2)):
        what = f"M={M} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}"
        wsz = L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(M, I, K, ctypes.byref(cfg) if cfg is not None else None)
        hbuf = torch.full((band + M * I * 2 + band,), 0x5A, dtype=torch.uint8, device=gpu)
        wbuf = torch.full((band + max(wsz, 16) + band,), 0xA5, dtype=torch.uint8, device=gpu)
        h = hbuf[band:band + M * I * 2].view(_tdt(dt)).view(M, I)
        h.fill_(float("nan"))
        ws = wbuf[band:band + max(wsz, 16)]
        ws.zero_()
        assert ws.data_ptr() % 16 == 0 and h.data_ptr() % 8 == 0
        _call(G, U, xbuf.data_ptr(), M, h.data_ptr(), cfg, ws=ws)
        assert bool((hbuf[:band] == 0x5A).all()) and bool((hbuf[band + M * I * 2:] == 0x5A).all()), f"write outside h: {what}"
        assert bool((wbuf[:band] == 0xA5).all()) and bool((wbuf[band + ws.numel():] == 0xA5).all()), \
            f"write outside the workspace: {what}"
        assert L.nf4_gemm_check_workspace(ws.data_ptr() if wsz else None, wsz, sp) == 0, what
        assert int(ws.count_nonzero()) == 0, f"workspace not all zero: {what}"
        _check_chain(h, xb, G, U, dt, what)


# ---- graph replay -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_a_captured_call_replays_on_new_x(coracle, gpu, dt):
    """M = 48, I = 192, K = 1152, three K slices: one capture; a replay after h was refilled with
    NaN and x changed in place gives the eager result for the new x, and leaves the workspace zero."""
    _lib, L = _lib_and_L()
    I, K, M = 192, 1152, 48
    G, U = _pair(coracle, gpu, "nested", I, K, dt)
    cfg = _cfg(4, 3)
    x0, x1 = _x(M, K, dt)[0].to(gpu), _x(M, K, dt, seed=12)[0].to(gpu)
    eager = [_swiglu(G, U, x, M, cfg).clone() for x in (x0, x1)]   # (also the warm-up: kernel attributes)
    assert not torch.equal(eager[0], eager[1])
    wsz = L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(M, I, K, ctypes.byref(cfg))
    assert wsz == 64 * 1024 + 256 + 3 * 2 * M * I * 4
    ws = torch.zeros(wsz, dtype=torch.uint8, device=gpu)
    x = x0.clone()
    h = torch.full((M, I), float("nan"), dtype=_tdt(dt), device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(G, U, x.data_ptr(), M, h.data_ptr(), cfg, ws=ws)
    for xn, want in ((x0, eager[0]), (x1, eager[1]), (x0, eager[0])):
        h.fill_(float("nan"))
        x.copy_(xn)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(h.view(torch.int16), want.view(torch.int16))
        assert int(ws.count_nonzero()) == 0
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0
