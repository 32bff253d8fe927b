"""nf4_gemm_bnb / nf4_gemm_bnb_single: every validation rule answers its code before any
device work (no GPU needed; fake pointers as in test_abi.py -- every call here either fails
validation or is a zero-size call, so none is ever dereferenced or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
N, K = 128, 1024
NBLK = N * K // 64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _nested(L, *, x=FAKE, M=4, packed=FAKE, plen=N * K // 2, a1=FAKE, nb=NBLK, code2=FAKE, a2=FAKE, n2=NBLK // 256,
            offset=None, bs=64, bs2=256, y=FAKE, dt=_lib.BF16, n=N, k=K, ws=None, wsb=0, cfg=None):
    return L.nf4_gemm_bnb(x, M, packed, plen, a1, nb, code2, a2, n2, offset, bs, bs2, y, dt, n, k, ws, wsb,
                          ctypes.byref(cfg) if cfg is not None else None, None)


def _single(L, *, x=FAKE, M=4, packed=FAKE, plen=N * K // 2, am=FAKE, nabs=NBLK, bs=64, y=FAKE, dt=_lib.BF16, n=N,
            k=K, ws=None, wsb=0, cfg=None):
    return L.nf4_gemm_bnb_single(x, M, packed, plen, am, nabs, bs, y, dt, n, k, ws, wsb,
                                 ctypes.byref(cfg) if cfg is not None else None, None)


# a cfg no family accepts: whatever else is right, the call ends at NF4DQ_ERR_ARG before the
# workspace check and the launch -- so a rule that must NOT fire shows as ERR_ARG, not a launch
BAD = dict(cfg=_lib.GemmCfg(_lib.GEMM_K128, 3, 1, 1, 1))


def test_symbols_exported(L):
    for name in ("nf4_gemm_bnb", "nf4_gemm_bnb_single", "nf4_gemm_bnb_workspace_bytes"):
        assert hasattr(L, name)


def test_zero_size_calls_are_ok(L):
    assert _nested(L, M=0) == _lib.OK
    assert _nested(L, n=0, plen=0) == _lib.OK
    assert _single(L, M=0) == _lib.OK
    assert _single(L, n=0, plen=0) == _lib.OK
    assert _nested(L, M=0, x=None, packed=None, a1=None, code2=None, a2=None, y=None) == _lib.OK


def test_argument_errors(L):
    assert _nested(L, dt=_lib.F32) == _lib.ERR_ARG  # 16-bit outputs only
    assert _nested(L, M=-1) == _lib.ERR_ARG
    assert _nested(L, n=-64) == _lib.ERR_ARG
    for name in ("x", "packed", "a1", "code2", "a2", "y"):
        assert _nested(L, **{name: None}) == _lib.ERR_ARG, name
    for name in ("x", "packed", "am", "y"):
        assert _single(L, **{name: None}) == _lib.ERR_ARG, name
    assert _nested(L, offset=None, **BAD) == _lib.ERR_ARG  # a null offset is allowed: ends at the cfg


@pytest.mark.parametrize("bs", [0, 32, 96, 8192, -64])
def test_blocksize_must_be_a_power_of_two_64_to_4096(L, bs):
    assert _nested(L, bs=bs) == _lib.ERR_ARG
    assert _single(L, bs=bs) == _lib.ERR_ARG


@pytest.mark.parametrize("bs2", [0, 1, 2, 3, 48, -256])
def test_blocksize2_must_be_a_power_of_two_from_4(L, bs2):
    assert _nested(L, bs2=bs2) == _lib.ERR_ARG


def test_shape_errors(L):
    assert _nested(L, M=33) == _lib.ERR_SHAPE
    assert _nested(L, n=96, plen=96 * K // 2) == _lib.ERR_SHAPE
    assert _nested(L, k=1088, plen=N * 1088 // 2) == _lib.ERR_SHAPE  # K % 128
    assert _nested(L, plen=N * K // 2 - 1) == _lib.ERR_SHAPE
    assert _single(L, M=33) == _lib.ERR_SHAPE
    assert _single(L, plen=N * K // 2 + 1) == _lib.ERR_SHAPE


def test_statistics_must_cover_the_weight(L):
    assert _nested(L, nb=NBLK - 1) == _lib.ERR_SHAPE
    assert _nested(L, n2=NBLK // 256 - 1) == _lib.ERR_SHAPE
    assert _nested(L, bs2=16, n2=NBLK // 16 - 1) == _lib.ERR_SHAPE
    assert _nested(L, bs2=16, n2=NBLK // 16, **BAD) == _lib.ERR_ARG      # enough: ends at the cfg
    assert _nested(L, bs=4096, nb=31, n2=1) == _lib.ERR_SHAPE            # ceil(131072 / 4096) = 32
    assert _nested(L, bs=4096, nb=32, n2=1, **BAD) == _lib.ERR_ARG
    # ceil: 64 x 128 elements in 4096-blocks = 2; 192 x 128 = 6
    assert _single(L, n=192, k=128, plen=192 * 64, bs=4096, nabs=5) == _lib.ERR_SHAPE
    assert _single(L, nabs=NBLK - 1) == _lib.ERR_SHAPE
    assert _single(L, nabs=NBLK, **BAD) == _lib.ERR_ARG


def test_cfg_of_a_family_without_the_mode_or_invalid(L):
    K128, STREAM, PERSIST, XS, XR, GEMV = (_lib.GEMM_K128, _lib.GEMM_STREAM, _lib.GEMM_PERSIST, _lib.GEMM_XS,
                                          _lib.GEMM_XR, _lib.GEMM_GEMV)
    for cfg in (_lib.GemmCfg(STREAM, 8, 2, 1, 1),          # valid for nf4_gemm_ref_cfg: no bnb mode
                _lib.GemmCfg(XS, 4, 2, K // 128 // 2, 1),   # likewise
                _lib.GemmCfg(_lib.GEMM_SK, 8, 2, 1, 1),     # retired
                _lib.GemmCfg(9, 8, 2, 1, 1),                # unknown
                _lib.GemmCfg(K128, 3, 1, 1, 1),             # invalid waves
                _lib.GemmCfg(PERSIST, 8, 2, 3, 1),          # K slices not dividing K / 256
                _lib.GemmCfg(XR, 8, 2, 2, 2),               # ksplit must be ceil(8 / 16) = 1
                _lib.GemmCfg(GEMV, 16, 1, 1, 0)):           # M = 4 is not the GEMV's
        assert _nested(L, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves)
        assert _single(L, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves)
    # statistics blocks above 64: the 128-deep kernel alone
    for cfg in (_lib.GemmCfg(PERSIST, 8, 2, 1, 1), _lib.GemmCfg(XR, 8, 2, 1, 1)):
        assert _nested(L, bs=128, nb=NBLK // 2, cfg=cfg) == _lib.ERR_ARG
        assert _single(L, bs=128, nabs=NBLK // 2, cfg=cfg) == _lib.ERR_ARG
    assert _nested(L, M=1, k=2048, plen=N * 1024, nb=2 * NBLK, n2=16, bs=128,
                   cfg=_lib.GemmCfg(GEMV, 16, 1, 1, 0)) == _lib.ERR_ARG


def test_workspace_is_checked_before_the_launch(L):
    """Shapes whose library choice splits K need a workspace: a null or short one is
    NF4DQ_ERR_ARG, and the size entry is positive, 16-byte granular and covers every named
    cfg the library could pick (the plan's own check: test_gemm_bnb_plan_cpu.py)."""
    for M, n, k in ((32, 4096, 4096), (12, 4096, 4096)):  # register-resident and persistent, two K slices each
        need = L.nf4_gemm_bnb_workspace_bytes(M, n, k, None)
        assert need > 0, (M, n, k)
        nblk = n * k // 64
        kw = dict(M=M, n=n, k=k, plen=n * k // 2)
        assert _nested(L, nb=nblk, n2=-(-nblk // 256), **kw) == _lib.ERR_ARG               # no workspace
        assert _nested(L, nb=nblk, n2=-(-nblk // 256), ws=FAKE + 8, wsb=need, **kw) == _lib.ERR_ARG  # misaligned
        assert _single(L, nabs=nblk, **kw) == _lib.ERR_ARG
    cfg = _lib.GemmCfg(_lib.GEMM_K128, 8, 1, 4, 1)
    need = L.nf4_gemm_bnb_workspace_bytes(4, N, K, ctypes.byref(cfg))
    assert need == L.nf4_gemm_workspace_bytes_cfg(4, N, K, ctypes.byref(cfg)) > 0
    assert _nested(L, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _single(L, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    # rejected shapes need nothing
    assert L.nf4_gemm_bnb_workspace_bytes(4, 96, K, None) == 0
    assert L.nf4_gemm_bnb_workspace_bytes(0, N, K, None) == 0
