"""The fused expert GEMM of a mixture-of-experts block in bitsandbytes semantics
(nf4_gemm_bnb_moe) through the C ABI on the GPU (``-m gpu``).

Every product is judged against the float64 oracle of the C oracle's exact 16-bit weights OF THE
PAIR'S EXPERT with the suite's GEMM bound (``_gemm_cases.gemm_oracle`` / ``check_close``); a pair
whose id is outside 0..E-1 must read as zero bits.  Outputs are NaN-prefilled, so a value never
stored fails.  Every expert has its own offset and its own perturbed code2 table, its packed
bytes sit ``packed_stride`` apart with 0xFF in the padding, and its statistics rows are padded
with values that blow the bound -- the wrong expert's or a neighbour's bytes fail.  The
exact-weight test uses the identity walk of test_gpu_gemm_mt.py with pairs alternating experts.

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
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits

pytestmark = pytest.mark.gpu

MOE = 9  # NF4DQ_GEMM_MOE


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _code(dt):
    return O.BF16 if dt == "bf16" else O.F16


def _lib_and_L():
    from nf4_triton_dequantization_amd import _lib

    return _lib, _lib.lib()


def _cfg(waves, ksplit):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(MOE, waves, 1, ksplit, 2)


class _Stack:
    """E experts of one shape on the device, stacked with padded strides, and the oracle's 16-bit
    matrix [N, K] of each.  mode "nested": own a1 / a2 / offset and a code2 table per expert
    (code2_stride 256); "single": own fp32 absmax.  ``kind`` "sensitive": sensitive_weight_bnb
    per expert (one code2 table shared by all: code2_stride 0).  What the suites of this file fix
    can be named (test_gpu_gemm_family_drawn.py draws it): ``bs2`` the blocksize2 of a drawn stack
    (sensitive weights are built for 16), ``shared_code2`` one table for all experts (a drawn stack:
    the dynamic map itself), ``null_offset`` every offset 0 and the descriptor's pointer NULL,
    ``pads`` the bytes / bytes / floats by which packed_stride, nb_stride and n2_stride exceed the
    data (the first a multiple of 16)."""

    def __init__(self, coracle, gpu, mode, kind, E, N, K, dt, bs2=None, shared_code2=None, null_offset=False,
                 pads=(4096 + 16, 3, 1)):
        self.mode, self.E, self.N, self.K, self.dt, self.gpu = mode, E, N, K, dt, gpu
        nblk = N * K // 64
        assert bs2 is None or kind != "sensitive"
        self.bs2 = BLOCKSIZE2 if kind == "sensitive" else 256 if bs2 is None else bs2
        n2 = -(-nblk // self.bs2)
        assert pads[0] % 16 == 0 and min(pads) >= 0
        self.pstride, self.nbstride, self.n2stride = N * K // 2 + pads[0], nblk + pads[1], (nblk if mode == "single" else n2) + pads[2]
        self.null_offset = null_offset and mode == "nested"
        packed = np.full((E, self.pstride), 0xFF, np.uint8)
        self.bits = []
        if mode == "nested":
            a1 = np.full((E, self.nbstride), 0xFF, np.uint8)
            a2 = np.full((E, self.n2stride), 1e30, np.float32)
            self.shared_code2 = kind == "sensitive" if shared_code2 is None else shared_code2
            code2 = np.zeros((1 if self.shared_code2 else E, 256), np.float32)
            offset = np.zeros(E, np.float32)
            for e in range(E):
                if kind == "sensitive":
                    q, b1, c2, b2, off = sensitive_weight_bnb(N, K, dt, seed=e + 1)[:5]
                else:
                    q, b1, c2, b2, off = drawn_weight_bnb(N, K, seed=N + K + 7 * e, blocksize2=self.bs2)
                    if not self.shared_code2:
                        c2 = (c2 * np.float32(1.0 + 0.03 * e)).astype(np.float32)   # the expert's own table
                    off = float(np.float32(off) + np.float32(0.004) * np.float32(e))  # ... and offset, none 0
                packed[e, :q.size], a1[e, :nblk], a2[e, :n2] = q, b1, b2
                code2[0 if self.shared_code2 else e], offset[e] = c2, 0.0 if self.null_offset else off
                self.bits.append(coracle.dequant_bnb(q, b1, c2, b2, float(offset[e]), N * K, _code(dt), 64,
                                                     self.bs2).reshape(N, K))
            assert kind == "sensitive" or self.null_offset or (len(set(offset.tolist())) == E and (offset != 0).all())
            self.t = [torch.from_numpy(v).to(gpu) for v in (packed, a1, code2, a2, offset)]
        else:
            am = np.full((E, self.n2stride), 1e30, np.float32)
            for e in range(E):
                q, b = single_weight_bnb(N, K, seed=N + K + 1 + 7 * e)
                packed[e, :q.size], am[e, :nblk] = q, b
                self.bits.append(coracle.dequant_bnb_single(q, b, N * K, _code(dt), 64).reshape(N, K))
            self.t = [torch.from_numpy(v).to(gpu) for v in (packed, am)]
        for b in self.bits:
            assert np.isfinite(bits_to_f64(b, dt)).all()
        for i in range(1, E):  # the experts differ: the wrong one's weights fail
            assert (self.bits[i] != self.bits[0]).mean() > 0.5

    def desc(self):
        from nf4_triton_dequantization_amd import _lib

        if self.mode == "nested":
            q, a1, c2, a2, off = self.t
            return _lib.MoeExperts(q.data_ptr(), self.pstride, a1.data_ptr(), self.nbstride, c2.data_ptr(),
                                   0 if self.shared_code2 else 256, a2.data_ptr(), self.n2stride,
                                   None if self.null_offset else off.data_ptr(),
                                   self.N, self.K, self.E, 0, 64, self.bs2)
        q, am = self.t
        return _lib.MoeExperts(q.data_ptr(), self.pstride, None, 0, None, 0, am.data_ptr(), self.n2stride, None,
                               self.N, self.K, self.E, 1, 64, 0)


_CACHE = {}


def _stack(coracle, gpu, mode, kind, E, N, K, dt):
    """One stack per (mode, kind, shape, dtype) for the whole module, never changed."""
    key = (mode, kind, E, N, K, dt)
    if key not in _CACHE:
        _CACHE[key] = _Stack(coracle, gpu, mode, kind, E, N, K, dt)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def _x(M, K, dt, seed=11):
    return x_bits(M, K, dt, seed)


def _call(S, x_ptr, ids, P, x_div, y_ptr, cfg=None, ws=None, expect=0):
    """One call; with ws None a fresh zeroed workspace, checked clean and zero afterwards."""
    _lib, L = _lib_and_L()
    cp = ctypes.byref(cfg) if cfg is not None else None
    d = S.desc()
    dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_moe_workspace_bytes(P, dp, cp)
    own = ws is None
    if own:
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=S.gpu)
    assert ws.numel() >= wsz
    assert ids.dtype == torch.int32 and ids.numel() == P and ids.is_contiguous()
    sp = torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 if S.dt == "bf16" else _lib.F16
    rc = L.nf4_gemm_bnb_moe(x_ptr, ids.data_ptr(), P, x_div, dp, y_ptr, code, ws.data_ptr() if wsz else None, wsz, cp, sp)
    assert rc == expect, (cfg and (cfg.waves, cfg.ksplit), _lib.strerror(rc))
    if own and wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg and (cfg.waves, cfg.ksplit)}"
    return wsz


def _moe(S, xd, ids_np, x_div, cfg=None, ws=None):
    P = len(ids_np)
    ids = torch.from_numpy(np.asarray(ids_np, np.int32)).to(S.gpu)
    y = torch.full((P, S.N), float("nan"), dtype=_tdt(S.dt), device=S.gpu)
    _call(S, xd.data_ptr(), ids, P, x_div, y.data_ptr(), cfg, ws)
    return y


def _check(S, y, xb, ids_np, x_div, what):
    """Every pair's row against the oracle of ITS expert; rows of invalid ids must be zero bits."""
    ids_np = np.asarray(ids_np)
    P = len(ids_np)
    yb = y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert yb.shape == (P, S.N)
    rows = np.arange(P) // x_div
    valid = (ids_np >= 0) & (ids_np < S.E)
    assert (yb[~valid] == 0).all(), f"{what}: rows of ids outside 0..E-1 are not zero"
    for e in range(S.E):
        sel = np.nonzero(ids_np == e)[0]
        if sel.size:
            ref, bound = gemm_oracle(xb[rows[sel]], S.bits[e], S.dt)
            check_close(bits_to_f64(yb[sel], S.dt), ref, bound, f"{what} expert {e} ({sel.size} pairs)")


def _patterns(P, E):
    """name -> ids[P]: the routings of the issue that P admits."""
    p = np.arange(P)
    pats = {
        "one expert, the others idle": np.full(P, E - 2),          # at P = 128: eight full row tiles on one expert
        "round robin": p % E,
        "-1 and E among valid ids": np.array([-1, 0, E, 1, 2, E - 1])[p % 6],
        "the same expert twice within a token": (p // 2) % E,
    }
    if P >= 33:  # one expert with exactly 16 rows, one with 17, the rest spread over the others
        pats["16 and 17 rows"] = np.where(p < 16, 0, np.where(p < 33, 1, 2 + p % (E - 2)))
    return pats


# ---- row tiles and routing patterns ------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("P", [1, 2, 16, 17, 33, 100, 128])
def test_routing_patterns_and_row_tiles(coracle, gpu, dt, mode, P):
    """E = 4, N = 192, K = 768: 12 blocks per row, so the 256-block boundary of blocksize2 falls
    inside a row of every expert's own flat stream; per-expert offsets and code2 tables, padded
    strides.  Every routing pattern x x_div in {1, 2, 8} x the library's cfg and three K slices."""
    E, N, K = 4, 192, 768
    S = _stack(coracle, gpu, mode, "drawn", E, N, K, dt)
    if mode == "nested":
        assert S.t[3].shape[1] == N * K // 64 // 256 + 1 and S.t[2].shape[0] == E
    for x_div in (1, 2, 8):
        M = -(-P // x_div)
        xt, xb = _x(M, K, dt)
        xd = xt.to(gpu)
        for name, ids in _patterns(P, E).items():
            if name == "16 and 17 rows":
                assert (ids == 0).sum() == 16 and (ids == 1).sum() == 17
            for cfg in (None, _cfg(2, 3)):
                what = f"{name} P={P} x_div={x_div} {mode} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}"
                _check(S, _moe(S, xd, ids, x_div, cfg), xb, ids, x_div, what)


# ---- K forms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [128, 384, 4096])
def test_k_forms_every_ksplit(coracle, gpu, dt, K):
    """E = 2, N = 64; K = 128 (one chunk), 384 (three), 4096 (32): every ksplit the plan admits,
    1 .. min(K / 128, 16), empty last slices included, and the library's own choice; in every
    other call all 40 pairs go to expert 1 and expert 0 is idle (its tickets must stay 0)."""
    _lib, L = _lib_and_L()
    E, N, P = 2, 64, 40
    S = _stack(coracle, gpu, "nested", "drawn", E, N, K, dt)
    xt, xb = _x(P, K, dt)
    xd = xt.to(gpu)
    top = min(K // 128, 16)
    for i, ks in enumerate(list(range(1, top + 1)) + [None]):
        ids = np.arange(P) % E if i % 2 == 0 else np.full(P, 1)
        y = _moe(S, xd, ids, 1, None if ks is None else _cfg(2, ks))
        _check(S, y, xb, ids, 1, f"K={K} ksplit={ks} {dt} {'both' if i % 2 == 0 else 'expert 0 idle'}")
    # one more slice than the plan admits, and 128-column workgroups over 64 columns: the caller's error
    ids = torch.zeros(P, dtype=torch.int32, device=gpu)
    y = torch.empty((P, N), dtype=_tdt(dt), device=gpu)
    for bad in (_cfg(2, top + 1), _cfg(4, 1), _cfg(2, 0)):
        _call(S, xd.data_ptr(), ids, P, 1, y.data_ptr(), bad, expect=_lib.ERR_ARG)


# ---- exact weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_identity_walk_recovers_each_experts_exact_weights(coracle, gpu, dt):
    """E = 2 sensitive weights (64 x 256, blocksize2 16).  128 pairs alternate experts; x holds
    rows k0 .. k0 + 63 of the identity (x_div 2: a token's two pairs share the row; x_div 1: each
    pair has its own copy), so y[2 t + e][n] is W_e[n][k0 + t] plus exact zeros and must equal the
    oracle's 16-bit weight of expert e by value, with no tolerance.  A fused multiply-add in the
    scale, a single rounding of the last product, a swapped expert, row, column or k all show.
    The library's choice (one K slice) and two slices; nested and single statistics."""
    E, N, K, P = 2, 64, 256, 128
    T = P // 2
    eye = torch.eye(K, dtype=_tdt(dt), device=gpu)
    ids = np.arange(P) % E
    for S in (_stack(coracle, gpu, "nested", "sensitive", E, N, K, dt), _stack(coracle, gpu, "single", "drawn", E, N, K, dt)):
        want = torch.stack([torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).to(gpu).view(_tdt(dt)) for b in S.bits])
        for cfg, x_div in ((None, 2), (_cfg(2, 2), 1)):
            rec = torch.empty((E, N, K), dtype=_tdt(dt), device=gpu)
            for k0 in range(0, K, T):
                x = eye[k0:k0 + T] if x_div == 2 else eye[k0:k0 + T].repeat_interleave(2, dim=0)
                y = _moe(S, x.contiguous(), ids, x_div, cfg).view(T, E, N)
                rec[:, :, k0:k0 + T] = y.permute(1, 2, 0)
            ok = rec == want
            assert bool(ok.all()), (f"{S.mode} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}: {int((~ok).sum())} of "
                                    f"{ok.numel()} weights differ, first at {(~ok).nonzero()[0].tolist()}")


# ---- guard bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("P,x_div", [(33, 2), (127, 8), (5, 1)])
def test_nothing_outside_y_changes_and_nothing_past_x_is_used(coracle, gpu, dt, P, x_div):
    """y sits between two sentinel bands of 64 rows in one allocation and is NaN-prefilled; x has
    exactly ceil(P / x_div) rows, followed by NaN rows in the same buffer.  E = 8, N = 128, K = 256:
    the library's choice (128-column workgroups), 128 columns with two slices, 64 columns with two;
    ids with invalid ones among them, so the zeroing stays inside y as well."""
    E, N, K, band = 8, 128, 256, 64
    S = _stack(coracle, gpu, "nested", "drawn", E, N, K, dt)
    M = -(-P // x_div)
    xt, xb = _x(M, K, dt)
    xbuf = torch.full((M + 16, K), float("nan"), dtype=_tdt(dt), device=gpu)
    xbuf[:M] = xt.to(gpu)
    ids_np = np.array([3, -1, 0, E, 7, 5, 1, 2 ** 31 - 1, -2 ** 31, 6])[np.arange(P) % 10]
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(gpu)
    for cfg in (None, _cfg(4, 2), _cfg(2, 2)):
        buf = torch.full((band + P + band, N), 0x5A5B, dtype=torch.int16, device=gpu)
        buf[band:band + P] = torch.full((P, N), float("nan"), dtype=_tdt(dt), device=gpu).view(torch.int16)
        y = buf[band:band + P].view(_tdt(dt))
        _call(S, xbuf.data_ptr(), ids, P, x_div, y.data_ptr(), cfg)
        what = f"P={P} x_div={x_div} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}"
        assert bool((buf[:band] == 0x5A5B).all()) and bool((buf[band + P:] == 0x5A5B).all()), f"band written: {what}"
        assert bool(torch.isfinite(y.float()).all()), f"NaN or inf in y: {what}"
        _check(S, y, xb, ids_np, x_div, what)


# ---- reproducible and re-entrant -------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_same_call_twice_on_one_workspace_gives_the_same_bits(coracle, gpu, dt):
    """E = 4, N = 192, K = 768, 100 pairs, three K slices: twice on one workspace with another
    routing (two experts idle, invalid ids) in between: identical bits, the second routing right,
    the workspace all zero after each call, nf4_gemm_check_workspace clean."""
    _lib, L = _lib_and_L()
    E, N, K, P = 4, 192, 768, 100
    S = _stack(coracle, gpu, "nested", "drawn", E, N, K, dt)
    cfg = _cfg(2, 3)
    d = S.desc()
    need = L.nf4_gemm_bnb_moe_workspace_bytes(P, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), ctypes.byref(cfg))
    assert need == 64 * 1024 + 256 + 3 * P * N * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    sp = torch.cuda.current_stream().cuda_stream
    xt, xb = _x(P // 2, K, dt)
    xd = xt.to(gpu)
    a = np.arange(P) % E
    b = np.array([1, 3, -1, 3, E])[np.arange(P) % 5]
    ys = []
    for ids in (a, b, a):
        ys.append(_moe(S, xd, ids, 2, cfg, ws=ws))
        assert int(ws.count_nonzero()) == 0, "tickets or slab entries left set"
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), sp) == 0
    _check(S, ys[0], xb, a, 2, f"first call {dt}")
    _check(S, ys[1], xb, b, 2, f"other routing {dt}")
    assert torch.equal(ys[0].view(torch.int16), ys[2].view(torch.int16))
