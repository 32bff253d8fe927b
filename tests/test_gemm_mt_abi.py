"""nf4_gemm_bnb_mt / nf4_gemm_bnb_mt_single: every validation rule answers its code before any
device work (no GPU needed; fake pointers as in test_gemm_bnb_abi.py -- every call here fails
validation, so none is ever dereferenced or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
N, K = 128, 1024
NBLK = N * K // 64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _nested(L, *, x=FAKE, M=64, packed=FAKE, plen=N * K // 2, a1=FAKE, nb=NBLK, code2=FAKE, a2=FAKE, n2=NBLK // 256,
            offset=None, bs=64, bs2=256, y=FAKE, dt=_lib.BF16, n=N, k=K, ws=None, wsb=0, cfg=None):
    return L.nf4_gemm_bnb_mt(x, M, packed, plen, a1, nb, code2, a2, n2, offset, bs, bs2, y, dt, n, k, ws, wsb,
                             ctypes.byref(cfg) if cfg is not None else None, None)


def _single(L, *, x=FAKE, M=64, packed=FAKE, plen=N * K // 2, am=FAKE, nabs=NBLK, bs=64, y=FAKE, dt=_lib.BF16, n=N,
            k=K, ws=None, wsb=0, cfg=None):
    return L.nf4_gemm_bnb_mt_single(x, M, packed, plen, am, nabs, bs, y, dt, n, k, ws, wsb,
                                    ctypes.byref(cfg) if cfg is not None else None, None)


# a cfg the family rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the
# workspace check and the launch -- so a rule that must NOT fire shows as ERR_ARG, not a launch
BAD = dict(cfg=_lib.GemmCfg(_lib.GEMM_MT, 3, 1, 1, 2))


def test_symbols_and_constants(L):
    for name in ("nf4_gemm_bnb_mt", "nf4_gemm_bnb_mt_single", "nf4_gemm_bnb_mt_workspace_bytes"):
        assert hasattr(L, name)
    text = open(_lib.HEADER_PATH).read()
    assert f"#define NF4DQ_GEMM_MT_MAX_M {_lib.GEMM_MT_MAX_M}\n" in text and _lib.GEMM_MT_MAX_M == 128
    assert f"#define NF4DQ_GEMM_MT {_lib.GEMM_MT}\n" in text
    assert f"#define NF4DQ_GEMM_MAX_M {_lib.GEMM_MAX_M}\n" in text and _lib.GEMM_MAX_M == 32  # unchanged


def test_argument_errors(L):
    assert _nested(L, dt=_lib.F32) == _lib.ERR_ARG  # 16-bit outputs only
    assert _nested(L, dt=7) == _lib.ERR_ARG
    assert _single(L, dt=_lib.F32) == _lib.ERR_ARG
    assert _nested(L, M=-1) == _lib.ERR_ARG
    for name in ("x", "packed", "a1", "code2", "a2", "y"):
        assert _nested(L, **{name: None}) == _lib.ERR_ARG, name
    for name in ("x", "packed", "am", "y"):
        assert _single(L, **{name: None}) == _lib.ERR_ARG, name
    assert _nested(L, offset=None, **BAD) == _lib.ERR_ARG  # a null offset is allowed: ends at the cfg
    for bs in (0, 32, 96, 8192, -64):                      # no power of two in 64..4096
        assert _nested(L, bs=bs) == _lib.ERR_ARG and _single(L, bs=bs) == _lib.ERR_ARG
    for bs2 in (0, 2, 48):
        assert _nested(L, bs2=bs2) == _lib.ERR_ARG
    # 16-byte loads of x and the packed weight, 8-byte stores of y
    assert _nested(L, x=FAKE + 8) == _lib.ERR_ARG
    assert _nested(L, packed=FAKE + 4) == _lib.ERR_ARG
    assert _single(L, y=FAKE + 2) == _lib.ERR_ARG


def test_shape_errors(L):
    for call in (_nested, _single):
        assert call(L, M=0) == _lib.ERR_SHAPE
        assert call(L, M=129) == _lib.ERR_SHAPE
        assert call(L, n=96, plen=96 * K // 2) == _lib.ERR_SHAPE
        assert call(L, n=0, plen=0) == _lib.ERR_SHAPE
        assert call(L, k=1088, plen=N * 1088 // 2) == _lib.ERR_SHAPE  # K % 128
        assert call(L, plen=N * K // 2 - 1) == _lib.ERR_SHAPE
    assert _nested(L, nb=NBLK - 1) == _lib.ERR_SHAPE
    assert _nested(L, n2=NBLK // 256 - 1) == _lib.ERR_SHAPE
    assert _nested(L, bs2=16, n2=NBLK // 16 - 1) == _lib.ERR_SHAPE
    assert _nested(L, bs2=16, n2=NBLK // 16, **BAD) == _lib.ERR_ARG  # enough: ends at the cfg
    assert _single(L, nabs=NBLK - 1) == _lib.ERR_SHAPE
    assert _single(L, nabs=NBLK, **BAD) == _lib.ERR_ARG
    # a larger statistics block is valid elsewhere and out of this family's domain
    assert _nested(L, bs=128, nb=NBLK // 2) == _lib.ERR_SHAPE
    assert _single(L, bs=128, nabs=NBLK // 2) == _lib.ERR_SHAPE
    # the rows this family adds are still out of the small-M entries' domain
    assert L.nf4_gemm_bnb(FAKE, 33, FAKE, N * K // 2, FAKE, NBLK, FAKE, FAKE, NBLK // 256, None, 64, 256, FAKE,
                          _lib.BF16, N, K, None, 0, None, None) == _lib.ERR_SHAPE


def test_named_cfg_never_falls_back(L):
    MT = _lib.GEMM_MT
    for cfg in (_lib.GemmCfg(MT, 3, 1, 1, 2),               # waves
                _lib.GemmCfg(MT, 8, 1, 1, 2),
                _lib.GemmCfg(MT, 4, 2, 1, 2),               # K stage
                _lib.GemmCfg(MT, 4, 1, 0, 2),               # K slices
                _lib.GemmCfg(MT, 4, 1, K // 128 + 1, 2),    # more slices than chunks
                _lib.GemmCfg(MT, 2, 1, 17, 2),              # more than 16
                _lib.GemmCfg(MT, 4, 1, 1, 1),               # strips per wave
                _lib.GemmCfg(_lib.GEMM_K128, 8, 1, 1, 1),   # another family's cfg
                _lib.GemmCfg(9, 4, 1, 1, 2)):               # unknown
        assert _nested(L, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips)
        assert _single(L, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips)
    # 128-column workgroups need N % 128 == 0
    wide = dict(n=192, plen=192 * K // 2, nb=192 * K // 64, n2=192 * K // 64 // 256)
    assert _nested(L, cfg=_lib.GemmCfg(MT, 4, 1, 1, 2), **wide) == _lib.ERR_ARG
    assert _nested(L, cfg=_lib.GemmCfg(MT, 2, 1, 0, 2), **wide) == _lib.ERR_ARG  # 64-column ones fit: ends at ksplit 0
    # ... and the small-M entries do not take this family's number
    assert L.nf4_gemm_bnb(FAKE, 4, FAKE, N * K // 2, FAKE, NBLK, FAKE, FAKE, NBLK // 256, None, 64, 256, FAKE,
                          _lib.BF16, N, K, None, 0, ctypes.byref(_lib.GemmCfg(MT, 4, 1, 1, 2)), None) == _lib.ERR_ARG


def test_workspace_is_checked_before_the_launch(L):
    """K slices need a workspace: a null, short or misaligned one is NF4DQ_ERR_ARG; the size
    entry answers header + ksplit * M * N * 4 bytes, and 0 for one slice or a rejected shape."""
    cfg = _lib.GemmCfg(_lib.GEMM_MT, 4, 1, 4, 2)
    need = L.nf4_gemm_bnb_mt_workspace_bytes(64, N, K, ctypes.byref(cfg))
    assert need == 64 * 1024 + 256 + 4 * 64 * N * 4
    assert _nested(L, cfg=cfg) == _lib.ERR_ARG
    assert _nested(L, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _single(L, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _nested(L, cfg=cfg, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    # the library's choice for 4096^2 splits K as well (whatever the CU count it finds)
    n = k = 4096
    lib_need = L.nf4_gemm_bnb_mt_workspace_bytes(64, n, k, None)
    assert lib_need > 64 * 1024 + 256 and (lib_need - 64 * 1024 - 256) % (64 * n * 4) == 0
    big = dict(n=n, k=k, plen=n * k // 2)
    assert _nested(L, nb=n * k // 64, n2=n * k // 64 // 256, **big) == _lib.ERR_ARG
    assert _single(L, nabs=n * k // 64, **big) == _lib.ERR_ARG
    one = _lib.GemmCfg(_lib.GEMM_MT, 4, 1, 1, 2)
    assert L.nf4_gemm_bnb_mt_workspace_bytes(64, N, K, ctypes.byref(one)) == 0
    assert L.nf4_gemm_bnb_mt_workspace_bytes(64, 96, K, None) == 0
    assert L.nf4_gemm_bnb_mt_workspace_bytes(0, N, K, None) == 0
    assert L.nf4_gemm_bnb_mt_workspace_bytes(129, N, K, None) == 0
