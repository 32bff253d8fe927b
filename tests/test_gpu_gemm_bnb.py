"""The fused GEMM in bitsandbytes semantics (nf4_gemm_bnb, nf4_gemm_bnb_single,
nf4_linear_bnb, Linear4bit.forward) on the GPU (``-m gpu``).

Method: the identity walk of test_gpu_gemm_exact.py.  With x = rows k0 .. k0+M-1 of the K x K
identity every output is one weight plus exact zeros, so walking k0 over K recovers the
dequantized matrix the kernel multiplied by.  It is compared with the C oracle's
``dequant_bnb`` / ``dequant_bnb_single`` BY VALUE WITH NO TOLERANCE (-0 == +0 allowed, NaN
never).  Weights: the sensitive weight of tests/_gemm_bnb_cases.py (a fused multiply-add in
the scale, or a single rounding of the last product, each give another 16-bit value in 64 of
its blocks; test_gemm_bnb_cases_cpu.py proves that on the oracle alone) and drawn ones.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_bnb_cases import BLOCKSIZE2, drawn_weight_bnb, sensitive_weight_bnb, single_weight_bnb
from _gemm_cases import (GEMV_FORMS, bits_to_f64, cfg_tuple, check_close, check_gemm, gemm_cfgs, gemm_oracle, tol,
                         x_bits)

pytestmark = pytest.mark.gpu

FAMILY = {1: "K128", 2: "STREAM", 3: "PERSIST", 4: "XS", 5: "XR", 7: "GEMV"}  # NF4DQ_GEMM_* numbers
WITH_MODE = {"K128", "PERSIST", "XR", "GEMV"}


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _code(dt):
    return O.BF16 if dt == "bf16" else O.F16


def _to_dev(bits, dt, gpu):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu).view(_tdt(dt))


def _want_nested(coracle, w, N, K, dt, gpu, bs=64, bs2=256):
    """The oracle's weights [N, K] on the device; all finite (0 x inf would not be exact)."""
    packed, a1, code2, a2, offset = w[:5]
    bits = coracle.dequant_bnb(packed, a1, code2, a2, offset, N * K, _code(dt), bs, bs2).reshape(N, K)
    assert np.isfinite(bits_to_f64(bits, dt)).all()
    return _to_dev(bits, dt, gpu), bits


def _want_single(coracle, packed, absmax, N, K, dt, gpu, bs=64):
    bits = coracle.dequant_bnb_single(packed, absmax, N * K, _code(dt), bs).reshape(N, K)
    assert np.isfinite(bits_to_f64(bits, dt)).all()
    return _to_dev(bits, dt, gpu), bits


def _starts(K, M):
    return [min(k0, K - M) for k0 in range(0, K, M)]


def _assemble(Y, starts, N, K, M):
    rec = torch.empty((N, K), dtype=Y.dtype, device=Y.device)
    full = K // M
    rec[:, :full * M] = Y[:full].permute(2, 0, 1).reshape(N, full * M)
    if K % M:
        rec[:, K - M:] = Y[-1].t()
    return rec


def _assert_exact(rec, want, what):
    ok = rec == want  # by value: -0 == +0, NaN equal to nothing
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} weights differ "
                             f"({int(torch.isnan(rec.float()).sum())} NaN); first at row {r} column {c}: "
                             f"got {float(rec[r, c])!r} want {float(want[r, c])!r}; rows "
                             f"{sorted(set(bad[:, 0].tolist()))[:8]} columns {sorted(set(bad[:, 1].tolist()))[:8]}")


def _identity(K, dt, gpu):
    return torch.eye(K, dtype=_tdt(dt), device=gpu)


def _dev_nested(w, gpu):
    packed, a1, code2, a2, offset = w[:5]
    t = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in (packed, a1, code2, a2)]
    return t + [torch.tensor([offset], dtype=torch.float32, device=gpu)]


def _recover_cfg(L, _lib, eye, t, dt, N, K, M, cfg, bs=64, bs2=256):
    """W recovered through nf4_gemm_bnb with `cfg` (None = the library's choice), or None if
    the entry rejects the cfg (ERR_ARG).  After the walk: the split-K error word clean
    (it is sticky) and every ticket and slab entry back at 0."""
    starts = _starts(K, M)
    Y = torch.full((len(starts), M, N), float("nan"), dtype=eye.dtype, device=eye.device)
    cp = ctypes.byref(cfg) if cfg is not None else None
    wsz = L.nf4_gemm_bnb_workspace_bytes(M, N, K, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=eye.device)
    sp = torch.cuda.current_stream().cuda_stream
    q, a1, c2, a2, off = t
    for i, k0 in enumerate(starts):
        rc = L.nf4_gemm_bnb(eye.data_ptr() + k0 * K * 2, M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                            c2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), bs, bs2, Y[i].data_ptr(),
                            _lib.BF16 if dt == "bf16" else _lib.F16, N, K, ws.data_ptr() if wsz else None, wsz, cp, sp)
        if rc == _lib.ERR_ARG and i == 0 and cfg is not None:
            return None
        assert rc == 0, (cfg and cfg_tuple(cfg), k0, _lib.strerror(rc))
    assert L.nf4_gemm_check_workspace(ws.data_ptr() if wsz else None, wsz, sp) == 0, cfg and cfg_tuple(cfg)
    if wsz:
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg and cfg_tuple(cfg)}"
    return _assemble(Y, starts, N, K, M)


class _RefAccepts:
    """Which cfgs the bnb entries must accept for a shape: a family that has the mode and a
    decomposition nf4_gemm_ref_cfg itself accepts there (asked of that entry with one real
    launch on reference-mode statistics of full size, so nothing wraps)."""

    def __init__(self, L, _lib, N, K, dt, gpu):
        self.L, self._lib, self.N, self.K, self.dt = L, _lib, N, K, dt
        bpr = K // 64
        self.q = torch.zeros(N * K // 2, dtype=torch.uint8, device=gpu)
        self.a1 = torch.ones(N * bpr, dtype=torch.uint8, device=gpu)
        self.a2 = torch.ones(N * (-(-bpr // 4)), dtype=torch.float32, device=gpu)
        self.x = torch.zeros((32, K), dtype=_tdt(dt), device=gpu)
        self.y = torch.empty((32, N), dtype=_tdt(dt), device=gpu)

    def __call__(self, cfg, M):
        L, _lib, N, K = self.L, self._lib, self.N, self.K
        if FAMILY.get(cfg.kernel) not in WITH_MODE:
            return False
        wsz = L.nf4_gemm_workspace_bytes_cfg(M, N, K, ctypes.byref(cfg))
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=self.q.device)
        rc = L.nf4_gemm_ref_cfg(self.x.data_ptr(), M, self.q.data_ptr(), self.q.numel(), self.a1.data_ptr(),
                                self.a1.numel(), self.a2.data_ptr(), self.a2.numel(), self.y.data_ptr(),
                                _lib.BF16 if self.dt == "bf16" else _lib.F16, N, K, ws.data_ptr() if wsz else None, wsz,
                                ctypes.byref(cfg), torch.cuda.current_stream().cuda_stream)
        assert rc in (0, _lib.ERR_ARG), (cfg_tuple(cfg), _lib.strerror(rc))
        return rc == 0


def _module_nested(w, N, K, dt, gpu, bs=64, bs2=256):
    """A Linear4bit-shaped module over hand-made nested statistics (any block sizes)."""
    from nf4_triton_dequantization_amd import QuantState

    q, a1, c2, a2, off = _dev_nested(w, gpu)
    st2 = QuantState(absmax=a2, code=c2, blocksize=bs2, dtype=torch.float32)
    qs = QuantState(absmax=a1, shape=torch.Size((N, K)), blocksize=bs, quant_type="nf4", dtype=_tdt(dt),
                    offset=off.reshape(()), state2=st2)
    return SimpleNamespace(weight=SimpleNamespace(data=q.view(-1, 1), quant_state=qs), out_features=N, in_features=K,
                           bias=None)


def _module_single(packed, absmax, N, K, dt, gpu, bs=64):
    from nf4_triton_dequantization_amd import QuantState

    qs = QuantState(absmax=torch.from_numpy(absmax).to(gpu), shape=torch.Size((N, K)), blocksize=bs,
                    quant_type="nf4", dtype=_tdt(dt))
    return SimpleNamespace(weight=SimpleNamespace(data=torch.from_numpy(packed).to(gpu).view(-1, 1), quant_state=qs),
                           out_features=N, in_features=K, bias=None)


def _recover_linear(eye, mod, N, K, M):
    from nf4_triton_dequantization_amd import nf4_linear_bnb

    starts = _starts(K, M)
    Y = torch.stack([nf4_linear_bnb(eye[k0:k0 + M], mod) for k0 in starts])
    return _assemble(Y, starts, N, K, M)


def _weight(kind, N, K, dt):
    if kind == "sensitive":
        return sensitive_weight_bnb(N, K, dt)[:5], BLOCKSIZE2
    return drawn_weight_bnb(N, K, seed=N + K), 256


# ---- explicit configurations ----------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sensitive", "drawn"])
@pytest.mark.parametrize("M", [32, 5])
def test_every_accepted_cfg_recovers_exact_weights(coracle, gpu, dt, kind, M):
    """N = 128, K = 1024: every entry of the shared decomposition list; nf4_gemm_bnb must
    accept exactly those of a family with the mode that nf4_gemm_ref_cfg accepts there, K128 and
    XR among them, and the persistent kernel at M = 5."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 128, 1024
    w, bs2 = _weight(kind, N, K, dt)
    want, _ = _want_nested(coracle, w, N, K, dt, gpu, 64, bs2)
    t = _dev_nested(w, gpu)
    eye = _identity(K, dt, gpu)
    ran = {}
    expected = _RefAccepts(L, _lib, N, K, dt, gpu)
    for cfg in gemm_cfgs(K, M):
        rec = _recover_cfg(L, _lib, eye, t, dt, N, K, M, cfg, 64, bs2)
        assert (rec is not None) == expected(cfg, M), f"accepted {rec is not None}: {FAMILY[cfg.kernel]} {cfg_tuple(cfg)} M={M}"
        if rec is None:
            continue
        _assert_exact(rec, want, f"{FAMILY[cfg.kernel]} cfg {cfg_tuple(cfg)} M={M} {dt} {kind}")
        ran[FAMILY[cfg.kernel]] = ran.get(FAMILY[cfg.kernel], 0) + 1
    print(f"bnb exact {dt} {kind} M={M}: configurations run {ran}")
    assert set(ran) <= WITH_MODE, ran
    for fam in ("K128", "XR") + (("PERSIST",) if M <= 16 else ()):
        assert ran.get(fam, 0) >= 1, (fam, ran)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sensitive", "drawn"])
def test_gemv_forms_recover_exact_weights(coracle, gpu, dt, kind):
    """The decode GEMV at M = 1, N = 64, K = 2048: its six forms."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 64, 2048
    w, bs2 = _weight(kind, N, K, dt)
    want, _ = _want_nested(coracle, w, N, K, dt, gpu, 64, bs2)
    t = _dev_nested(w, gpu)
    eye = _identity(K, dt, gpu)
    for waves, rows in GEMV_FORMS:
        cfg = _lib.GemmCfg(_lib.GEMM_GEMV, waves, rows, 1, 0)
        rec = _recover_cfg(L, _lib, eye, t, dt, N, K, 1, cfg, 64, bs2)
        assert rec is not None, (waves, rows)
        _assert_exact(rec, want, f"GEMV ({waves}, {rows}) {dt} {kind}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [5, 32])
def test_k128_gathered_scales_at_large_k(coracle, gpu, dt, M):
    """The 128-deep kernel keeps a slice's scales in LDS while that table is at most 48 KiB;
    beyond it every chunk gathers its statistics and, in nested mode, looks code2 up in an LDS
    table of its own.  N = 64, K = 16384, cfg {K128, 8 waves, depth 1, one K slice, 4 strips}:
    a 64 KiB table, so the gathered form, nested and single; random x against the float64
    oracle of the exact weights (an identity walk would need a 512 MiB identity)."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 64, 16384
    cfg = _lib.GemmCfg(_lib.GEMM_K128, 8, 1, 1, 4)
    assert 16 * 4 * 2 * (K // 128) * 4 > 48 * 1024  # the plan's k128_scale_bytes for this cfg
    code = _lib.BF16 if dt == "bf16" else _lib.F16
    xt, xb = x_bits(M, K, dt, seed=12)
    xd = xt.to(gpu)
    sp = torch.cuda.current_stream().cuda_stream
    assert L.nf4_gemm_bnb_workspace_bytes(M, N, K, ctypes.byref(cfg)) == 0
    w = drawn_weight_bnb(N, K, seed=13)
    _, wb = _want_nested(coracle, w, N, K, dt, gpu)
    q, a1, c2, a2, off = _dev_nested(w, gpu)
    y = torch.full((M, N), float("nan"), dtype=_tdt(dt), device=gpu)
    rc = L.nf4_gemm_bnb(xd.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                        a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256, y.data_ptr(), code, N, K, None, 0,
                        ctypes.byref(cfg), sp)
    assert rc == 0, _lib.strerror(rc)
    check_gemm(y, xb, wb, dt, f"K128 gathered nested M={M} {dt}")
    packed, absmax = single_weight_bnb(N, K, seed=14)
    _, wb = _want_single(coracle, packed, absmax, N, K, dt, gpu)
    qs, am = torch.from_numpy(packed).to(gpu), torch.from_numpy(absmax).to(gpu)
    y2 = torch.full((M, N), float("nan"), dtype=_tdt(dt), device=gpu)
    rc = L.nf4_gemm_bnb_single(xd.data_ptr(), M, qs.data_ptr(), qs.numel(), am.data_ptr(), am.numel(), 64,
                               y2.data_ptr(), code, N, K, None, 0, ctypes.byref(cfg), sp)
    assert rc == 0, _lib.strerror(rc)
    check_gemm(y2, xb, wb, dt, f"K128 gathered single M={M} {dt}")


# ---- a nested group ending inside a row -----------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K,M", [(768, 5), (768, 32), (1536, 5)])
def test_nested_group_boundary_inside_a_row(coracle, gpu, dt, K, M):
    """blocksize2 = 256, N = 64, K = 768 (12 blocks per row): the 256th block is row 21,
    block 4, so f >> 8 changes in the middle of a row.  Every accepted cfg: the
    register-resident and 128-deep kernels.  (No decomposition of the persistent kernel is
    valid at K = 768 -- three 256-deep chunks, rings of 2 or 4 -- in either mode; K = 1536,
    24 blocks per row, the 256th block row 10, block 16, is the smallest such K it takes.)"""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N = 64
    w = drawn_weight_bnb(N, K, seed=5)
    assert w[3].size == N * K // 64 // 256 and (K // 64) % 256 != 0 and 256 % (K // 64) != 0
    want, _ = _want_nested(coracle, w, N, K, dt, gpu)
    t = _dev_nested(w, gpu)
    eye = _identity(K, dt, gpu)
    ran = {}
    expected = _RefAccepts(L, _lib, N, K, dt, gpu)
    for cfg in gemm_cfgs(K, M):
        rec = _recover_cfg(L, _lib, eye, t, dt, N, K, M, cfg)
        assert (rec is not None) == expected(cfg, M), f"accepted {rec is not None}: {FAMILY[cfg.kernel]} {cfg_tuple(cfg)} M={M}"
        if rec is None:
            continue
        _assert_exact(rec, want, f"{FAMILY[cfg.kernel]} cfg {cfg_tuple(cfg)} M={M} {dt}")
        ran[FAMILY[cfg.kernel]] = ran.get(FAMILY[cfg.kernel], 0) + 1
    print(f"bnb boundary {dt} K={K} M={M}: configurations run {ran}")
    for fam in ("K128", "XR") + (("PERSIST",) if K == 1536 else ()):
        assert ran.get(fam, 0) >= 1, (fam, ran)
    _assert_exact(_recover_cfg(L, _lib, eye, t, dt, N, K, M, None), want, f"library choice M={M} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_nested_group_boundary_inside_a_row_gemv(coracle, gpu, dt):
    """N = 64, K = 6144 (96 blocks per row, three GEMV pieces) at M = 1: the 256th block is
    row 2, block 64.  The library's choice (the GEMV) and one more form."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 64, 6144
    w = drawn_weight_bnb(N, K, seed=6)
    want, _ = _want_nested(coracle, w, N, K, dt, gpu)
    t = _dev_nested(w, gpu)
    eye = _identity(K, dt, gpu)
    _assert_exact(_recover_cfg(L, _lib, eye, t, dt, N, K, 1, None), want, f"library choice {dt}")
    cfg = _lib.GemmCfg(_lib.GEMM_GEMV, 8, 4, 1, 0)
    _assert_exact(_recover_cfg(L, _lib, eye, t, dt, N, K, 1, cfg), want, f"GEMV (8, 4) {dt}")


# ---- block sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("bs", [128, 4096])
@pytest.mark.parametrize("M", [1, 8])
def test_block_sizes_nested_and_single(coracle, gpu, dt, bs, M):
    """blocksize 128 and 4096 (a 4096-block spans four rows of K = 1024) through
    nf4_linear_bnb, nested (blocksize2 = 4: the smallest) and single."""
    N, K = 128, 1024
    eye = _identity(K, dt, gpu)
    w = drawn_weight_bnb(N, K, seed=bs, blocksize=bs, blocksize2=4)
    want, _ = _want_nested(coracle, w, N, K, dt, gpu, bs, 4)
    _assert_exact(_recover_linear(eye, _module_nested(w, N, K, dt, gpu, bs, 4), N, K, M), want,
                  f"nested blocksize {bs} M={M} {dt}")
    packed, absmax = single_weight_bnb(N, K, seed=bs + 1, blocksize=bs)
    want, _ = _want_single(coracle, packed, absmax, N, K, dt, gpu, bs)
    _assert_exact(_recover_linear(eye, _module_single(packed, absmax, N, K, dt, gpu, bs), N, K, M), want,
                  f"single blocksize {bs} M={M} {dt}")


# ---- single mode ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 8, 17])
def test_single_mode_library_choice(coracle, gpu, dt, M):
    """A compress_statistics=False weight (fp32 absmax per 64-block), N = 128, K = 2048: the
    GEMV (M = 1), the persistent kernel (8), the 128-deep kernel (17)."""
    from nf4_triton_dequantization_amd import Linear4bit

    N, K = 128, 2048
    wf = torch.from_numpy(O.normal_f32(77, N * K, stream=9).reshape(N, K)).to(gpu)
    mod = Linear4bit.from_float(wf, compute_dtype=_tdt(dt), compress_statistics=False)
    qs = mod.weight.quant_state
    assert qs.absmax.dtype == torch.float32 and getattr(qs, "state2", None) is None
    want, _ = _want_single(coracle, mod.weight.data.view(-1).cpu().numpy(), qs.absmax.cpu().numpy(), N, K, dt, gpu)
    _assert_exact(_recover_linear(_identity(K, dt, gpu), mod, N, K, M), want, f"single M={M} {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_single_mode_every_accepted_cfg(coracle, gpu, dt):
    """nf4_gemm_bnb_single through every accepted cfg at N = 128, K = 1024, M = 5 and 32."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 128, 1024
    packed, absmax = single_weight_bnb(N, K, seed=3)
    want, _ = _want_single(coracle, packed, absmax, N, K, dt, gpu)
    q, am = torch.from_numpy(packed).to(gpu), torch.from_numpy(absmax).to(gpu)
    eye = _identity(K, dt, gpu)
    sp = torch.cuda.current_stream().cuda_stream
    expected = _RefAccepts(L, _lib, N, K, dt, gpu)
    for M in (5, 32):
        starts = _starts(K, M)
        ran = {}
        for cfg in gemm_cfgs(K, M):
            wsz = L.nf4_gemm_bnb_workspace_bytes(M, N, K, ctypes.byref(cfg))
            ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=gpu)
            Y = torch.full((len(starts), M, N), float("nan"), dtype=eye.dtype, device=gpu)
            rejected = False
            for i, k0 in enumerate(starts):
                rc = L.nf4_gemm_bnb_single(eye.data_ptr() + k0 * K * 2, M, q.data_ptr(), q.numel(), am.data_ptr(),
                                           am.numel(), 64, Y[i].data_ptr(), _lib.BF16 if dt == "bf16" else _lib.F16,
                                           N, K, ws.data_ptr() if wsz else None, wsz, ctypes.byref(cfg), sp)
                if rc == _lib.ERR_ARG and i == 0:
                    rejected = True
                    break
                assert rc == 0, (cfg_tuple(cfg), k0, _lib.strerror(rc))
            assert (not rejected) == expected(cfg, M), f"accepted {not rejected}: {FAMILY[cfg.kernel]} {cfg_tuple(cfg)} M={M}"
            if rejected:
                continue
            assert L.nf4_gemm_check_workspace(ws.data_ptr() if wsz else None, wsz, sp) == 0, cfg_tuple(cfg)
            if wsz:
                assert int(ws.count_nonzero()) == 0, cfg_tuple(cfg)
            _assert_exact(_assemble(Y, starts, N, K, M), want, f"single {FAMILY[cfg.kernel]} {cfg_tuple(cfg)} M={M} {dt}")
            ran[FAMILY[cfg.kernel]] = ran.get(FAMILY[cfg.kernel], 0) + 1
        print(f"bnb single {dt} M={M}: configurations run {ran}")
        assert set(ran) <= WITH_MODE, ran
        for fam in ("K128", "XR") + (("PERSIST",) if M <= 16 else ()):
            assert ran.get(fam, 0) >= 1, (fam, ran)


# ---- the offset lives on the device ---------------------------------------------------------
@pytest.mark.parametrize("M", [1, 8])
def test_offset_is_read_on_the_device_every_call(coracle, gpu, M):
    """After one walk, quant_state.offset is changed in place on the device; the next walk's
    weights follow the new offset: nothing was cached or read on the host."""
    N, K, dt = 128, 2048, "bf16"
    w = list(drawn_weight_bnb(N, K, seed=9))
    mod = _module_nested(w, N, K, dt, gpu)
    eye = _identity(K, dt, gpu)
    want, _ = _want_nested(coracle, w, N, K, dt, gpu)
    _assert_exact(_recover_linear(eye, mod, N, K, M), want, f"first offset M={M}")
    new = float(np.float32(0.0625 + w[4]))
    mod.weight.quant_state.offset.fill_(new)
    w[4] = new
    want2, _ = _want_nested(coracle, w, N, K, dt, gpu)
    assert not bool((want2 == want).all())
    _assert_exact(_recover_linear(eye, mod, N, K, M), want2, f"offset changed in place M={M}")


@pytest.mark.parametrize("off", [None, 0.03125])
def test_offset_none_and_python_number(coracle, gpu, off):
    """quant_state.offset = None is a null pointer (0), a Python number a device scalar."""
    N, K, dt, M = 128, 1024, "f16", 8
    w = list(drawn_weight_bnb(N, K, seed=10))
    w[4] = 0.0 if off is None else off
    mod = _module_nested(w, N, K, dt, gpu)
    mod.weight.quant_state.offset = off
    want, _ = _want_nested(coracle, w, N, K, dt, gpu)
    _assert_exact(_recover_linear(_identity(K, dt, gpu), mod, N, K, M), want, f"offset {off!r}")


# ---- the product's own quantizer and dequantizer --------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("M", [1, 8, 32])
def test_from_float_module_equals_its_own_dequantizer(gpu, dt, nested, M):
    """Linear4bit.from_float: the weights recovered through forward equal
    dequantize_nf4_bnb(module), element for element."""
    from nf4_triton_dequantization_amd import Linear4bit, dequantize_nf4_bnb

    N, K = 128, 2048
    wf = torch.from_numpy(O.normal_f32(5, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    mod = Linear4bit.from_float(wf, compute_dtype=_tdt(dt), compress_statistics=nested)
    want = dequantize_nf4_bnb(mod)
    assert bool(torch.isfinite(want.float()).all())
    eye = _identity(K, dt, gpu)
    starts = _starts(K, M)
    with torch.no_grad():
        rec = _assemble(torch.stack([mod(eye[k0:k0 + M]) for k0 in starts]), starts, N, K, M)
    _assert_exact(rec, want, f"from_float nested={nested} M={M} {dt}")


def _oracle_bits_of(coracle, mod, N, K, dt):
    qs = mod.weight.quant_state
    return coracle.dequant_bnb(mod.weight.data.view(-1).cpu().numpy(), qs.absmax.cpu().numpy(),
                               qs.state2.code.cpu().numpy(), qs.state2.absmax.cpu().numpy(), float(qs.offset),
                               N * K, _code(dt), int(qs.blocksize), int(qs.state2.blocksize)).reshape(N, K)


@pytest.fixture(scope="module")
def float_module(gpu):
    """One quantized module per dtype (N = 256, K = 1024, with a bias), shared and unchanged."""
    from nf4_triton_dequantization_amd import Linear4bit

    N, K = 256, 1024
    wf = torch.from_numpy(O.normal_f32(21, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    bias = torch.from_numpy(O.normal_f32(22, N, stream=9)).to(gpu)
    return {dt: Linear4bit.from_float(wf, compute_dtype=_tdt(dt), bias=bias) for dt in ("bf16", "f16")}, N, K


def _with_bias(ref, bound, bias64, dt):
    """y = RNE16(RNE16(x . W^T) + b): the oracle plus the bias, and the GEMM's bound plus the
    one more rounding of the 16-bit add (half an ulp of the result)."""
    p = 8 if dt == "bf16" else 11
    exp = ref + bias64[None, :]
    return exp, bound + 2.0 ** -p * np.abs(exp)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_random_x_through_the_module(coracle, gpu, float_module, dt):
    """module(x) for x [2, 3, K] (M = 6) with a bias, against the float64 oracle of the exact
    weights (the suite's own tolerance)."""
    mods, N, K = float_module
    mod = mods[dt]
    wb = _oracle_bits_of(coracle, mod, N, K, dt)
    xt, xb = x_bits(6, K, dt, seed=3)
    with torch.no_grad():
        y = mod(xt.to(gpu).reshape(2, 3, K))
    assert y.shape == (2, 3, N) and y.dtype == _tdt(dt)
    ref, bound = gemm_oracle(xb, wb, dt)
    b16 = mod.bias.detach().to(_tdt(dt)).view(torch.int16).cpu().numpy().view(np.uint16)
    exp, bound = _with_bias(ref, bound, bits_to_f64(b16, dt), dt)
    yb = y.reshape(6, N).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    check_close(bits_to_f64(yb, dt), exp, bound, f"module(x) {dt}")
    # and without the bias through check_gemm itself
    from nf4_triton_dequantization_amd import nf4_linear_bnb

    check_gemm(nf4_linear_bnb(xt.to(gpu), mod), xb, wb, dt, f"nf4_linear_bnb {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gradients_take_the_differentiable_path(coracle, gpu, float_module, dt):
    """x.requires_grad_(): the result is differentiable and x.grad = dy @ W within the
    GEMM tolerance; under no_grad the same input takes the fused path."""
    mods, N, K = float_module
    mod = mods[dt]
    wb = _oracle_bits_of(coracle, mod, N, K, dt)
    xt, xb = x_bits(6, K, dt, seed=4)
    x = xt.to(gpu).requires_grad_()
    y = mod(x)
    assert y.requires_grad and y.grad_fn is not None
    ref, bound = gemm_oracle(xb, wb, dt)
    b16 = mod.bias.detach().to(_tdt(dt)).view(torch.int16).cpu().numpy().view(np.uint16)
    exp, bound = _with_bias(ref, bound, bits_to_f64(b16, dt), dt)
    check_close(y.detach().double().cpu().numpy(), exp, bound, f"forward with grad {dt}")
    dyt, dyb = x_bits(6, N, dt, seed=5)
    y.backward(dyt.to(gpu))
    assert x.grad is not None and x.grad.shape == x.shape
    dy64, w64 = bits_to_f64(dyb, dt), bits_to_f64(wb, dt)
    gref = dy64 @ w64
    check_close(x.grad.double().cpu().numpy(), gref, tol(gref, np.abs(dy64) @ np.abs(w64), dt), f"x.grad {dt}")


@pytest.mark.parametrize("M,N", [(40, 128), (8, 96)])
def test_shapes_outside_the_fused_path_fall_back(coracle, gpu, M, N):
    """M = 40 (above 32 rows) and N = 96 (not a multiple of 64): dequantize + matmul."""
    from nf4_triton_dequantization_amd import Linear4bit

    K, dt = 1024, "bf16"
    wf = torch.from_numpy(O.normal_f32(31, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    mod = Linear4bit.from_float(wf, compute_dtype=_tdt(dt))
    wb = _oracle_bits_of(coracle, mod, N, K, dt)
    xt, xb = x_bits(M, K, dt, seed=6)
    with torch.no_grad():
        y = mod(xt.to(gpu))
    check_gemm(y, xb, wb, dt, f"fallback M={M} N={N}")


# ---- subnormal weights ----------------------------------------------------------------------
@pytest.mark.parametrize("dt,scale", [("f16", 1e-4), ("bf16", 1e-37)])
@pytest.mark.parametrize("M", [1, 8])
def test_subnormal_weights_come_through_exactly(coracle, gpu, dt, scale, M):
    """absmax2 and the offset scaled so that more than half the 16-bit weights are subnormal:
    the GEMV's dot (M = 1) and the persistent kernel's MFMA operands (M = 8) keep them."""
    N, K = 64, 2048
    w = drawn_weight_bnb(N, K, seed=7, subnormal_scale=scale)
    want, bits = _want_nested(coracle, w, N, K, dt, gpu)
    exp = (bits & 0x7C00) if dt == "f16" else (bits & 0x7F80)
    sub = (exp == 0) & ((bits & 0x7FFF) != 0)
    print(f"bnb subnormal {dt}: {sub.mean():.1%} of the weights subnormal, {((bits & 0x7FFF) == 0).mean():.1%} zero")
    assert sub.mean() > 0.5
    rec = _recover_linear(_identity(K, dt, gpu), _module_nested(w, N, K, dt, gpu), N, K, M)
    _assert_exact(rec, want, f"subnormal weights M={M} {dt}")


# ---- one launch, no host synchronisation ----------------------------------------------------
@pytest.mark.parametrize("M", [1, 8])
def test_forward_is_capturable_and_never_falls_back(gpu, monkeypatch, M):
    """Linear4bit.from_float(linear)(x) at decode sizes: with the unfused path made to raise,
    forward still runs, and it can be captured into a graph -- a host read of the offset
    (``.item()``) would synchronise, which a capture refuses -- whose replay gives the eager
    result."""
    from nf4_triton_dequantization_amd import Linear4bit, kernel

    N, K = 256, 2048
    lin = torch.nn.Linear(K, N, bias=True, device=gpu, dtype=torch.bfloat16)
    mod = Linear4bit.from_float(lin)
    x = torch.randn((M, K), device=gpu, dtype=torch.bfloat16)

    def unfused(*a, **k):
        raise AssertionError("Linear4bit.forward fell back to dequantize + matmul at a decode size")

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", unfused)
    with torch.no_grad():
        y0 = mod(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = mod(x)
        g.replay()
        torch.cuda.synchronize()
    assert y.shape == (M, N) and bool(torch.isfinite(y.float()).all())
    assert torch.equal(y, y0)
