"""The fused expert SwiGLU launch of a mixture-of-experts block in bitsandbytes semantics
(nf4_gemm_bnb_moe_swiglu) through the C ABI on the GPU (``-m gpu``).

h[p] = rn(rn(silu(g)) * u) with g and u what nf4_gemm_bnb_moe stores for pair p from the gate and
from the up stack.  Products are judged against the float64 chain of the float64 GEMMs of the C
oracle's exact 16-bit weights OF THE PAIR'S EXPERT (``gemm_oracle`` twice, ``swiglu_oracle``);
elementwise checks use the acceptance set of _swiglu_cases.py; a pair whose id is outside 0..E-1
must read as zero bits.  h is NaN-prefilled, so a value never stored fails.

The two stacks are built differently, so that a swapped stack, expert, table, offset or blocksize2
fails: the gate stack is test_gpu_gemm_moe's drawn one (blocksize2 256, a code2 table per expert,
code2_stride 256, offsets 0.0123 + 0.004 e); the up stack has blocksize2 16, ONE table shared by its
experts (the dynamic map reversed and scaled, code2_stride 0), offsets -0.0371 - 0.003 e and other
strides.  Both pad their strides with 0xFF / 1e30.

After every call that had a workspace: the whole workspace reads 0 again (tickets and planes) and
nf4_gemm_check_workspace is clean.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_gpu_gemm_moe as MOE
from _gemm_bnb_cases import code2_np, drawn_weight_bnb, single_weight_bnb
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits
from _swiglu_cases import NEAR_TIE_CAP, accept, allowed_s, rn16, swiglu_oracle, to_bits

pytestmark = pytest.mark.gpu

MSG = 11  # NF4DQ_GEMM_MOE_SWIGLU
HEADER = 64 * 1024 + 256
_tdt, _code = MOE._tdt, MOE._code


def _lib_and_L():
    from nf4_triton_dequantization_amd import _lib

    return _lib, _lib.lib()


def _cfg(waves, ksplit, kernel=MSG):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(kernel, waves, 1, ksplit, 2)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class _UpStack(MOE._Stack):
    """The up stack: as test_gpu_gemm_moe._Stack (whose ``desc`` it uses), but nested statistics
    have blocksize2 16 and ONE code2 table for all experts, the offsets are its own, and the padded
    strides differ from the gate stack's.  ``bs2``, ``shared_code2`` (False: the shared table scaled
    by 1 + 0.02 e per expert, code2_stride 256), ``null_offset`` and ``pads`` as in _Stack, for
    test_gpu_gemm_family_drawn.py."""

    def __init__(self, coracle, gpu, mode, E, N, K, dt, bs2=16, shared_code2=True, null_offset=False, pads=(2048 + 32, 5, 2)):
        self.mode, self.E, self.N, self.K, self.dt, self.gpu = mode, E, N, K, dt, gpu
        nblk = N * K // 64
        self.bs2 = bs2
        n2 = -(-nblk // self.bs2)
        assert pads[0] % 16 == 0 and min(pads) >= 0
        self.pstride, self.nbstride, self.n2stride = N * K // 2 + pads[0], nblk + pads[1], (nblk if mode == "single" else n2) + pads[2]
        self.null_offset = null_offset and mode == "nested"
        packed = np.full((E, self.pstride), 0xFF, np.uint8)
        self.bits = []
        if mode == "nested":
            self.shared_code2 = shared_code2
            a1 = np.full((E, self.nbstride), 0xFF, np.uint8)
            a2 = np.full((E, self.n2stride), 1e30, np.float32)
            code2 = (code2_np()[::-1] * np.float32(0.75)).astype(np.float32).reshape(1, 256).copy()
            if not shared_code2:
                code2 = (code2 * (np.float32(1.0) + np.float32(0.02) * np.arange(E, dtype=np.float32))[:, None]).astype(np.float32)
            offset = np.zeros(E, np.float32)
            for e in range(E):
                q, b1, _, b2, _ = drawn_weight_bnb(N, K, seed=N + K + 3 + 7 * e, blocksize2=self.bs2)
                packed[e, :q.size], a1[e, :nblk], a2[e, :n2] = q, b1, b2
                if not self.null_offset:
                    offset[e] = np.float32(-0.0371) - np.float32(0.003) * np.float32(e)
                self.bits.append(coracle.dequant_bnb(q, b1, code2[0 if shared_code2 else e], b2, float(offset[e]), N * K,
                                                     _code(dt), 64, self.bs2).reshape(N, K))
            assert self.null_offset or (len(set(offset.tolist())) == E and (offset != 0).all())
            self.t = [torch.from_numpy(v).to(gpu) for v in (packed, a1, code2, a2, offset)]
        else:
            am = np.full((E, self.n2stride), 1e30, np.float32)
            for e in range(E):
                q, b = single_weight_bnb(N, K, seed=N + K + 2 + 7 * e)
                packed[e, :q.size], am[e, :nblk] = q, b
                self.bits.append(coracle.dequant_bnb_single(q, b, N * K, _code(dt), 64).reshape(N, K))
            self.t = [torch.from_numpy(v).to(gpu) for v in (packed, am)]
        for b in self.bits:
            assert np.isfinite(bits_to_f64(b, dt)).all()


_CACHE = {}


def _pair(coracle, gpu, mode, E, I, K, dt):
    """(gate stack, up stack) per (mode, shape, dtype) for the whole module, never changed."""
    key = (mode, E, I, K, dt)
    if key not in _CACHE:
        G = MOE._stack(coracle, gpu, mode, "drawn", E, I, K, dt)
        U = _UpStack(coracle, gpu, mode, E, I, K, dt)
        if mode == "nested":
            assert G.bs2 == 256 and U.bs2 == 16 and not G.shared_code2 and U.shared_code2
            og, ou = G.t[4].cpu().numpy(), U.t[4].cpu().numpy()
            assert (og != 0).all() and (ou != 0).all() and not set(og.tolist()) & set(ou.tolist())
        assert (G.pstride, G.n2stride) != (U.pstride, U.n2stride)
        for e in range(E):
            assert (G.bits[e] != U.bits[e]).mean() > 0.5
        _CACHE[key] = (G, U)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def _x(M, K, dt, seed=11):
    return x_bits(M, K, dt, seed)


def _call(G, U, x_ptr, ids, P, x_div, h_ptr, cfg=None, ws=None, expect=0):
    """One call; with ws None a fresh zeroed workspace, checked clean and zero afterwards."""
    _lib, L = _lib_and_L()
    assert G.mode == U.mode and (G.E, G.N, G.K, G.dt) == (U.E, U.N, U.K, U.dt)
    cp = ctypes.byref(cfg) if cfg is not None else None
    descs = (_lib.MoeExperts * 2)(G.desc(), U.desc())
    dp = ctypes.cast(descs, ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_moe_swiglu_workspace_bytes(P, dp, cp)
    own = ws is None
    if own:
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=G.gpu)
    assert ws.numel() >= wsz
    assert ids.dtype == torch.int32 and ids.numel() == P and ids.is_contiguous()
    sp = torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 if G.dt == "bf16" else _lib.F16
    rc = L.nf4_gemm_bnb_moe_swiglu(x_ptr, ids.data_ptr(), P, x_div, dp, _lib.ACT_SILU, h_ptr, code,
                                   ws.data_ptr() if wsz else None, wsz, cp, sp)
    assert rc == expect, (cfg and (cfg.waves, cfg.ksplit), _lib.strerror(rc))
    if own and wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or plane entries left set, cfg {cfg and (cfg.waves, cfg.ksplit)}"
    return wsz


def _msg(G, U, xd, ids_np, x_div, cfg=None, ws=None):
    P = len(ids_np)
    ids = torch.from_numpy(np.asarray(ids_np, np.int32)).to(G.gpu)
    h = torch.full((P, G.N), float("nan"), dtype=_tdt(G.dt), device=G.gpu)
    _call(G, U, xd.data_ptr(), ids, P, x_div, h.data_ptr(), cfg, ws)
    return h


def _check(G, U, h, xb, ids_np, x_div, what):
    """Every pair's row against the float64 chain of the two float64 GEMMs of ITS expert; rows of
    invalid ids must be zero bits."""
    ids_np = np.asarray(ids_np)
    P = len(ids_np)
    hb = _bits(h)
    assert hb.shape == (P, G.N)
    rows = np.arange(P) // x_div
    valid = (ids_np >= 0) & (ids_np < G.E)
    assert (hb[~valid] == 0).all(), f"{what}: rows of ids outside 0..E-1 are not zero bits"
    for e in range(G.E):
        sel = np.nonzero(ids_np == e)[0]
        if sel.size:
            (gr, gt), (ur, ut) = gemm_oracle(xb[rows[sel]], G.bits[e], G.dt), gemm_oracle(xb[rows[sel]], U.bits[e], G.dt)
            ref, bound = swiglu_oracle(gr, gt, ur, ut, G.dt)
            check_close(bits_to_f64(hb[sel], G.dt), ref, bound, f"{what} expert {e} ({sel.size} pairs)")


# ---- row tiles and routing patterns ------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("P", [1, 2, 16, 17, 33, 100, 128])
def test_routing_patterns_and_row_tiles(coracle, gpu, dt, mode, P):
    """E = 4, I = 192, K = 768: 12 blocks per row, so a blocksize2 boundary (256 in the gate stack,
    16 in the up stack) falls inside a row.  Every routing pattern of test_gpu_gemm_moe (one expert
    with the others idle; round robin; -1 and E among valid ids; the same expert twice in a token;
    exactly 16 and 17 rows on two experts) x x_div in {1, 2, 8} x the library's cfg and (2 waves,
    3 slices)."""
    E, I, K = 4, 192, 768
    G, U = _pair(coracle, gpu, mode, E, I, K, dt)
    for x_div in (1, 2, 8):
        M = -(-P // x_div)
        xt, xb = _x(M, K, dt)
        xd = xt.to(gpu)
        for name, ids in MOE._patterns(P, E).items():
            if name == "16 and 17 rows":
                assert (ids == 0).sum() == 16 and (ids == 1).sum() == 17
            for cfg in (None, _cfg(2, 3)):
                what = f"{name} P={P} x_div={x_div} {mode} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}"
                _check(G, U, _msg(G, U, xd, ids, x_div, cfg), xb, ids, x_div, what)


# ---- same slices, same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("ksplit", [1, 2, 4])
def test_same_slices_give_the_chain_of_the_expert_gemms_outputs(coracle, gpu, dt, mode, ksplit):
    """nf4_gemm_bnb_moe on each stack and the new entry with the same ksplit at K = 1152 (9 chunks:
    5 + 4 at two slices; 3 + 3 + 3 and an EMPTY slice at four), I = 192, P = 100 over 4 experts:
    the sums run in the same order, so h must lie in the acceptance set of the two outputs' bits,
    element for element -- with two and with four waves.  The acceptance set caps near-tie elements
    at 1 %: the oracle's own g for these inputs is checked on the CPU first to stay under half of
    that."""
    E, I, K, P = 4, 192, 1152, 100
    G, U = _pair(coracle, gpu, mode, E, I, K, dt)
    xt, xb = _x(P // 2, K, dt)
    xd = xt.to(gpu)
    ids = np.array([0, 1, 2, 3, 3, 1, -1, 2, 0, 0])[np.arange(P) % 10]
    rows = np.arange(P) // 2
    near = []
    for e in range(E):
        sel = np.nonzero(ids == e)[0]
        g64 = gemm_oracle(xb[rows[sel]], G.bits[e], dt)[0]
        near.append(allowed_s(to_bits(rn16(g64, dt), dt), dt)[2].ravel())
    assert np.concatenate(near).mean() <= NEAR_TIE_CAP / 2, "the inputs themselves sit too close to the cap"
    g = _bits(MOE._moe(G, xd, ids, 2, MOE._cfg(2, ksplit)))
    u = _bits(MOE._moe(U, xd, ids, 2, MOE._cfg(2, ksplit)))
    assert (g[ids < 0] == 0).all() and (u[ids < 0] == 0).all()
    for waves in (2, 4):
        h = _bits(_msg(G, U, xd, ids, 2, _cfg(waves, ksplit)))
        assert (h[ids < 0] == 0).all()
        accept(h, g, u, dt, f"ksplit {ksplit} waves {waves} {mode} {dt}")


# ---- exact weights --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
def test_identity_windows_give_the_chain_of_each_experts_exact_weights(coracle, gpu, dt, mode):
    """E = 2, I = 64, K = 256; 128 pairs alternate experts and x holds rows k0 .. k0 + 63 of the
    identity (x_div 2), so g and u of h[2 t + e][n] are Wg_e[n][k0 + t] and Wu_e[n][k0 + t] plus
    exact zeros: h must lie in the acceptance set of the oracle's own 16-bit weights of expert e.
    (A weight that is -0 comes out of the sum as +0, as in test_gpu_gemm_mt_swiglu.py.)  One K
    slice (the lane-local epilogue) and two (the reducer's)."""
    E, I, K, P = 2, 64, 256, 128
    T = P // 2
    G, U = _pair(coracle, gpu, mode, E, I, K, dt)
    eye = torch.eye(K, dtype=_tdt(dt), device=gpu)
    ids = np.arange(P) % E
    for cfg in (None, _cfg(2, 2)):
        rec = np.empty((E, I, K), np.uint16)
        for k0 in range(0, K, T):
            h = _bits(_msg(G, U, eye[k0:k0 + T].contiguous(), ids, 2, cfg)).reshape(T, E, I)
            rec[:, :, k0:k0 + T] = h.transpose(1, 2, 0)
        for e in range(E):
            g, u = (np.where(b == 0x8000, np.uint16(0), b) for b in (G.bits[e], U.bits[e]))
            accept(rec[e], g, u, dt, f"expert {e} {mode} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}")


# ---- every instantiation --------------------------------------------------------------------------
@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("P", [16, 48, 80, 128])
@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_instantiation(coracle, gpu, dt, mode, waves, P, ksplit):
    """I = 128, K = 640 (five chunks: one slice wraps the weight ring, two get 3 + 2), 2 / 4 / 6 / 8
    row tiles.  All pairs go to expert 1 but the last, which goes to expert 0: one workgroup runs
    the instantiation with all its row tiles live, another with one."""
    E, I, K = 2, 128, 640
    G, U = _pair(coracle, gpu, mode, E, I, K, dt)
    ids = np.ones(P, np.int32)
    ids[-1] = 0
    xt, xb = _x(P, K, dt)
    what = f"{dt} {mode} waves={waves} P={P} ksplit={ksplit}"
    _check(G, U, _msg(G, U, xt.to(gpu), ids, 1, _cfg(waves, ksplit)), xb, ids, 1, what)


# ---- stack order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gate_and_up_are_not_interchangeable(coracle, gpu, dt):
    """h(gate, up) differs from h(up, gate), and each is the chain of its own expert-GEMM outputs
    (E = 4, I = 192, K = 768, 33 pairs, one K slice)."""
    E, I, K, P = 4, 192, 768, 33
    G, U = _pair(coracle, gpu, "nested", E, I, K, dt)
    xd = _x(P, K, dt)[0].to(gpu)
    ids = np.arange(P) % E
    g, u = _bits(MOE._moe(G, xd, ids, 1, MOE._cfg(2, 1))), _bits(MOE._moe(U, xd, ids, 1, MOE._cfg(2, 1)))
    h_gu, h_ug = _bits(_msg(G, U, xd, ids, 1, _cfg(4, 1))), _bits(_msg(U, G, xd, ids, 1, _cfg(4, 1)))
    assert (h_gu != h_ug).mean() > 0.9
    accept(h_gu, g, u, dt, f"(gate, up) {dt}")
    accept(h_ug, u, g, dt, f"(up, gate) {dt}")


# ---- guard bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("P,x_div", [(33, 2), (127, 8), (5, 1)])
def test_nothing_outside_h_changes_and_nothing_past_x_is_used(coracle, gpu, dt, P, x_div):
    """h sits between two sentinel bands of 64 rows in one allocation and is NaN-prefilled; x has
    exactly ceil(P / x_div) rows, followed by NaN rows in the same buffer.  E = 4, I = 192, K = 768:
    the library's choice, four waves with two slices, two waves with two; the ids hold INT_MIN,
    INT_MAX, -1 and E among valid ones, so the zeroing stays inside h as well."""
    E, I, K, band = 4, 192, 768, 64
    G, U = _pair(coracle, gpu, "nested", E, I, K, dt)
    M = -(-P // x_div)
    xt, xb = _x(M, K, dt)
    xbuf = torch.full((M + 16, K), float("nan"), dtype=_tdt(dt), device=gpu)
    xbuf[:M] = xt.to(gpu)
    ids_np = np.array([3, -1, 0, E, 2, 1, 2 ** 31 - 1, -2 ** 31, 3])[np.arange(P) % 9]
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(gpu)
    for cfg in (None, _cfg(4, 2), _cfg(2, 2)):
        buf = torch.full((band + P + band, I), 0x5A5B, dtype=torch.int16, device=gpu)
        buf[band:band + P] = torch.full((P, I), float("nan"), dtype=_tdt(dt), device=gpu).view(torch.int16)
        h = buf[band:band + P].view(_tdt(dt))
        _call(G, U, xbuf.data_ptr(), ids, P, x_div, h.data_ptr(), cfg)
        what = f"P={P} x_div={x_div} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)}"
        assert bool((buf[:band] == 0x5A5B).all()) and bool((buf[band + P:] == 0x5A5B).all()), f"band written: {what}"
        assert bool(torch.isfinite(h.float()).all()), f"NaN or inf in h: {what}"
        _check(G, U, h, xb, ids_np, x_div, what)


# ---- reproducible and re-entrant -------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_same_call_twice_on_one_workspace_gives_the_same_bits(coracle, gpu, dt):
    """E = 4, I = 192, K = 768, 100 pairs, three K slices: twice on one workspace with another
    routing (two experts idle, invalid ids) in between: identical bits, the second routing right,
    the workspace all zero after each call, nf4_gemm_check_workspace clean."""
    _lib, L = _lib_and_L()
    E, I, K, P = 4, 192, 768, 100
    G, U = _pair(coracle, gpu, "nested", E, I, K, dt)
    cfg = _cfg(2, 3)
    descs = (_lib.MoeExperts * 2)(G.desc(), U.desc())
    need = L.nf4_gemm_bnb_moe_swiglu_workspace_bytes(P, ctypes.cast(descs, ctypes.c_void_p), ctypes.byref(cfg))
    assert need == HEADER + 3 * 2 * P * I * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    sp = torch.cuda.current_stream().cuda_stream
    xt, xb = _x(P // 2, K, dt)
    xd = xt.to(gpu)
    a = np.arange(P) % E
    b = np.array([1, 3, -1, 3, E])[np.arange(P) % 5]
    hs = []
    for ids in (a, b, a):
        hs.append(_msg(G, U, xd, ids, 2, cfg, ws=ws))
        assert int(ws.count_nonzero()) == 0, "tickets or plane entries left set"
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), sp) == 0
    _check(G, U, hs[0], xb, a, 2, f"first call {dt}")
    _check(G, U, hs[1], xb, b, 2, f"other routing {dt}")
    assert torch.equal(hs[0].view(torch.int16), hs[2].view(torch.int16))


# ---- graph replay -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_a_captured_call_follows_new_ids_and_new_x(coracle, gpu, dt):
    """E = 4, I = 192, K = 768, 48 pairs (x_div 2), three K slices: one capture; each replay after h
    was refilled with NaN and the ids tensor and x were overwritten in place gives the eager result
    for its own inputs, and leaves the workspace zero."""
    _lib, L = _lib_and_L()
    E, I, K, P = 4, 192, 768, 48
    G, U = _pair(coracle, gpu, "nested", E, I, K, dt)
    cfg = _cfg(4, 3)
    xs = [_x(P // 2, K, dt)[0].to(gpu), _x(P // 2, K, dt, seed=12)[0].to(gpu)]
    routes = [np.arange(P) % E, np.array([2, 2, -1, 0, E, 2, 3])[np.arange(P) % 7]]
    cases = [(xs[0], routes[0]), (xs[1], routes[1]), (xs[0], routes[1]), (xs[0], routes[0])]
    eager = [_msg(G, U, x, r, 2, cfg).clone() for x, r in cases]   # (also the warm-up: kernel attributes)
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[0], eager[2])
    descs = (_lib.MoeExperts * 2)(G.desc(), U.desc())
    wsz = L.nf4_gemm_bnb_moe_swiglu_workspace_bytes(P, ctypes.cast(descs, ctypes.c_void_p), ctypes.byref(cfg))
    assert wsz == HEADER + 3 * 2 * P * I * 4
    ws = torch.zeros(wsz, dtype=torch.uint8, device=gpu)
    x = xs[0].clone()
    ids = torch.from_numpy(routes[0].astype(np.int32)).to(gpu)
    h = torch.full((P, I), float("nan"), dtype=_tdt(dt), device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(G, U, x.data_ptr(), ids, P, 2, h.data_ptr(), cfg, ws=ws)
    for (xn, rn), want in zip(cases, eager):
        h.fill_(float("nan"))
        x.copy_(xn)
        ids.copy_(torch.from_numpy(rn.astype(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(h.view(torch.int16), want.view(torch.int16))
        assert int(ws.count_nonzero()) == 0
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0


# ---- bad cfgs ---------------------------------------------------------------------------------------
def test_bad_cfgs_are_the_callers_error(coracle, gpu):
    """E = 2, I = 64, K = 384 (three chunks): one slice too many, waves whose columns do not divide I
    (8 waves would own 128 columns of 64; with I % 64 == 0 both wave counts of the family, 32 and 64
    columns, always divide), 3 waves, ksplit 0 and another family's kernel number (the expert
    GEMM's, the SwiGLU launch's) each return NF4DQ_ERR_ARG; the same fields in range are accepted."""
    _lib, _ = _lib_and_L()
    E, I, K, P = 2, 64, 384, 40
    G, U = _pair(coracle, gpu, "nested", E, I, K, "bf16")
    xt, xb = _x(P, K, "bf16")
    xd = xt.to(gpu)
    ids_np = np.arange(P) % E
    ids = torch.from_numpy(ids_np.astype(np.int32)).to(gpu)
    h = torch.full((P, I), float("nan"), dtype=torch.bfloat16, device=gpu)
    for bad in (_cfg(2, K // 128 + 1), _cfg(8, 1), _cfg(3, 1), _cfg(2, 0), _cfg(2, 1, kernel=MOE.MOE), _cfg(2, 1, kernel=10)):
        _call(G, U, xd.data_ptr(), ids, P, 1, h.data_ptr(), bad, expect=_lib.ERR_ARG)
    assert bool(torch.isnan(h.float()).all()), "a rejected call wrote h"
    for good in (_cfg(2, K // 128), _cfg(4, 1), _cfg(2, 1, kernel=0)):
        _check(G, U, _msg(G, U, xd, ids_np, 1, good), xb, ids_np, 1, f"cfg {(good.kernel, good.waves, good.ksplit)}")
