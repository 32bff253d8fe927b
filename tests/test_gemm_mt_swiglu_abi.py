"""nf4_gemm_bnb_mt_swiglu: symbols and constants against the header text, and every validation
rule answers its code before any device work (no GPU needed; fake pointers and the "bad cfg"
trick of test_gemm_mt_abi.py -- every call here fails validation, so none is ever dereferenced
or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
I, K = 128, 1024
NBLK = I * K // 64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _mat(single, **kw):
    """One weight's descriptor: good for [I, K] unless a field is overridden."""
    f = dict(packed=FAKE, plen=I * K // 2, a1=None if single else FAKE, nb=0 if single else NBLK,
             code2=None if single else FAKE, a2=FAKE, n2=NBLK if single else NBLK // 256, offset=None, bs=64,
             bs2=0 if single else 256, y=None, n=I)
    f.update(kw)
    return _lib.GemmBnbMat(f["packed"], f["plen"], f["a1"], f["nb"], f["code2"], f["a2"], f["n2"], f["offset"], f["bs"],
                           f["bs2"], f["y"], f["n"])


def _call(L, *, single=0, gate=None, up=None, both=None, x=FAKE, M=64, k=K, act=None, h=FAKE, dt=_lib.BF16, ws=None,
          wsb=0, cfg=None, mats="two"):
    """gate / up: overrides of that weight's descriptor; both: of the two."""
    arr = (_lib.GemmBnbMat * 2)(_mat(single, **{**(both or {}), **(gate or {})}),
                                _mat(single, **{**(both or {}), **(up or {})}))
    mp = ctypes.cast(arr, ctypes.c_void_p) if mats == "two" else None
    return L.nf4_gemm_bnb_mt_swiglu(x, M, k, mp, single, _lib.ACT_SILU if act is None else act, h, dt, ws, wsb,
                                    ctypes.byref(cfg) if cfg is not None else None, None)


# a cfg the family rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the
# workspace check and the launch -- so a rule that must NOT fire shows as ERR_ARG, not a launch
BAD = dict(cfg=_lib.GemmCfg(_lib.GEMM_MT_SWIGLU, 3, 1, 1, 2))
# every per-weight rule is tried on the gate weight and on the up weight
WEIGHTS = (("gate",), ("up",))


def test_symbols_and_constants(L):
    for name in ("nf4_gemm_bnb_mt_swiglu", "nf4_gemm_bnb_mt_swiglu_workspace_bytes"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    text = open(_lib.HEADER_PATH).read()
    assert f"#define NF4DQ_GEMM_MT_SWIGLU {_lib.GEMM_MT_SWIGLU}\n" in text and _lib.GEMM_MT_SWIGLU == 10
    assert f"#define NF4DQ_ACT_SILU {_lib.ACT_SILU}\n" in text and _lib.ACT_SILU == 0
    assert f"#define NF4DQ_GEMM_MT_MAX_M {_lib.GEMM_MT_MAX_M}\n" in text and _lib.GEMM_MT_MAX_M == 128  # unchanged
    assert f"#define NF4DQ_GEMM_MT {_lib.GEMM_MT}\n" in text and _lib.GEMM_MT == 8
    # the descriptor is nf4_gemm_bnb_grouped's, as it was
    assert ctypes.sizeof(_lib.GemmBnbMat) == 88


def test_argument_errors(L):
    assert _call(L, dt=_lib.F32) == _lib.ERR_ARG  # 16-bit outputs only
    assert _call(L, dt=7) == _lib.ERR_ARG
    assert _call(L, single=1, dt=_lib.F32) == _lib.ERR_ARG
    for act in (1, -1, 7):                        # NF4DQ_ACT_SILU alone
        assert _call(L, act=act) == _lib.ERR_ARG and _call(L, single=1, act=act) == _lib.ERR_ARG
    assert _call(L, M=-1) == _lib.ERR_ARG
    assert _call(L, x=None) == _lib.ERR_ARG and _call(L, h=None) == _lib.ERR_ARG
    assert _call(L, mats=None) == _lib.ERR_ARG
    for (w,) in WEIGHTS:
        for name in ("packed", "a1", "code2", "a2"):
            assert _call(L, **{w: {name: None}}) == _lib.ERR_ARG, (w, name)
        for name in ("packed", "a2"):
            assert _call(L, single=1, **{w: {name: None}}) == _lib.ERR_ARG, (w, name)
        for bs in (0, 32, 96, 8192, -64):          # no power of two in 64..4096
            assert _call(L, **{w: dict(bs=bs)}) == _lib.ERR_ARG and _call(L, single=1, **{w: dict(bs=bs)}) == _lib.ERR_ARG
        for bs2 in (0, 2, 48):
            assert _call(L, **{w: dict(bs2=bs2)}) == _lib.ERR_ARG
        assert _call(L, single=1, **{w: dict(bs2=3)}, **BAD) == _lib.ERR_ARG  # ignored in single mode: ends at the cfg
        assert _call(L, **{w: dict(packed=FAKE + 4)}) == _lib.ERR_ARG           # 16-byte loads of the packed weights
        assert _call(L, **{w: dict(offset=None)}, **BAD) == _lib.ERR_ARG        # a null offset is allowed
    # 16-byte loads of x, 8-byte stores of h; the y fields are ignored
    assert _call(L, x=FAKE + 8) == _lib.ERR_ARG
    assert _call(L, h=FAKE + 4) == _lib.ERR_ARG and _call(L, single=1, h=FAKE + 2) == _lib.ERR_ARG
    assert _call(L, both=dict(y=FAKE + 1), **BAD) == _lib.ERR_ARG
    # an argument error in front of a shape error answers first
    assert _call(L, M=0, act=1) == _lib.ERR_ARG and _call(L, M=0, x=FAKE + 8) == _lib.ERR_ARG


def test_shape_errors(L):
    for single in (0, 1):
        assert _call(L, single=single, M=0) == _lib.ERR_SHAPE
        assert _call(L, single=single, M=129) == _lib.ERR_SHAPE
        assert _call(L, single=single, M=128, **BAD) == _lib.ERR_ARG and _call(L, single=single, M=1, **BAD) == _lib.ERR_ARG
        assert _call(L, single=single, both=dict(n=96, plen=96 * K // 2)) == _lib.ERR_SHAPE   # I % 64
        assert _call(L, single=single, both=dict(n=0, plen=0)) == _lib.ERR_SHAPE              # I >= 64
        assert _call(L, single=single, k=1088, both=dict(plen=I * 1088 // 2)) == _lib.ERR_SHAPE  # K % 128
        assert _call(L, single=single, k=64, both=dict(plen=I * 64 // 2)) == _lib.ERR_SHAPE      # K >= 128
        for (w,) in WEIGHTS:
            wide = dict(n=2 * I, plen=I * K, nb=0 if single else 2 * NBLK, n2=2 * NBLK)
            assert _call(L, single=single, **{w: wide}) == _lib.ERR_SHAPE                     # the two N differ
            assert _call(L, single=single, **{w: dict(plen=I * K // 2 - 1)}) == _lib.ERR_SHAPE
            # a larger statistics block is valid elsewhere and out of this entry's domain
            assert _call(L, single=single, **{w: dict(bs=128, nb=0 if single else NBLK // 2,
                                                       n2=NBLK // 2 if single else NBLK // 256)}) == _lib.ERR_SHAPE
    for (w,) in WEIGHTS:
        assert _call(L, **{w: dict(nb=NBLK - 1)}) == _lib.ERR_SHAPE
        assert _call(L, **{w: dict(n2=NBLK // 256 - 1)}) == _lib.ERR_SHAPE
        assert _call(L, **{w: dict(bs2=16, n2=NBLK // 16 - 1)}) == _lib.ERR_SHAPE
        assert _call(L, **{w: dict(bs2=16, n2=NBLK // 16)}, **BAD) == _lib.ERR_ARG  # enough: ends at the cfg
        assert _call(L, single=1, **{w: dict(n2=NBLK - 1)}) == _lib.ERR_SHAPE
    assert _call(L, single=1, **BAD) == _lib.ERR_ARG and _call(L, **BAD) == _lib.ERR_ARG


def test_too_large(L):
    big = 1 << 19                                                                       # I > 2^18
    assert _call(L, k=128, both=dict(n=big, plen=big * 64, nb=big * 2, n2=big * 2)) == _lib.ERR_TOO_LARGE
    wide = 1 << 18                                                                      # packed_len = 2^31
    st = dict(n=wide, plen=wide * 8192, nb=wide * 256, n2=wide * 256)
    assert _call(L, k=16384, both=st) == _lib.ERR_TOO_LARGE
    assert _call(L, single=1, k=16384, both={**st, "nb": 0}) == _lib.ERR_TOO_LARGE
    # x beyond 2^31 bytes cannot happen within K <= 2^24 and M <= 128 short of the packed limit; K > 2^24:
    k = (1 << 24) + 128
    assert _call(L, k=k, both=dict(n=64, plen=64 * k // 2, nb=k, n2=k)) == _lib.ERR_TOO_LARGE
    # 16 slices of two planes of 128 x 2^18 floats: the plane index would pass 32 bits
    cfg = _lib.GemmCfg(_lib.GEMM_MT_SWIGLU, 4, 1, 16, 2)
    st = dict(n=wide, plen=wide * 1024, nb=wide * 32, n2=wide * 32)
    assert _call(L, M=128, k=2048, both=st, cfg=cfg, ws=FAKE, wsb=1 << 40) == _lib.ERR_TOO_LARGE


def test_named_cfg_never_falls_back(L):
    SG = _lib.GEMM_MT_SWIGLU
    for cfg in (_lib.GemmCfg(SG, 3, 1, 1, 2),               # waves
                _lib.GemmCfg(SG, 8, 1, 1, 2),
                _lib.GemmCfg(SG, 4, 2, 1, 2),               # K stage
                _lib.GemmCfg(SG, 4, 1, 0, 2),               # K slices
                _lib.GemmCfg(SG, 4, 1, K // 128 + 1, 2),    # more slices than chunks
                _lib.GemmCfg(SG, 2, 1, 17, 2),              # more than 16
                _lib.GemmCfg(SG, 4, 1, 1, 1),               # strips per wave
                _lib.GemmCfg(SG, 4, 1, 1, 4),
                _lib.GemmCfg(_lib.GEMM_MT, 4, 1, 1, 2),     # the parent family's cfg
                _lib.GemmCfg(_lib.GEMM_K128, 8, 1, 1, 1),   # another family's
                _lib.GemmCfg(11, 4, 1, 1, 2)):              # unknown
        assert _call(L, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips)
        assert _call(L, single=1, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips)
    # kernel 0 and strips 0 read as this family's: such a cfg ends at the workspace check
    assert _call(L, cfg=_lib.GemmCfg(0, 2, 1, 2, 0)) == _lib.ERR_ARG
    # ... and the other entries do not take this family's number
    assert L.nf4_gemm_bnb_mt(FAKE, 64, FAKE, I * K // 2, FAKE, NBLK, FAKE, FAKE, NBLK // 256, None, 64, 256, FAKE,
                             _lib.BF16, I, K, None, 0, ctypes.byref(_lib.GemmCfg(SG, 4, 1, 1, 2)), None) == _lib.ERR_ARG
    assert L.nf4_gemm_bnb(FAKE, 4, FAKE, I * K // 2, FAKE, NBLK, FAKE, FAKE, NBLK // 256, None, 64, 256, FAKE,
                          _lib.BF16, I, K, None, 0, ctypes.byref(_lib.GemmCfg(SG, 4, 1, 1, 2)), None) == _lib.ERR_ARG


def test_workspace_is_checked_before_the_launch(L):
    """K slices need a workspace: a null, short or misaligned one is NF4DQ_ERR_ARG; the size entry
    answers header + ksplit * 2 * M * I * 4 bytes, and 0 for one slice or a rejected shape."""
    cfg = _lib.GemmCfg(_lib.GEMM_MT_SWIGLU, 4, 1, 4, 2)
    need = L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(64, I, K, ctypes.byref(cfg))
    assert need == 64 * 1024 + 256 + 4 * 2 * 64 * I * 4
    assert _call(L, cfg=cfg) == _lib.ERR_ARG
    assert _call(L, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, single=1, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, cfg=cfg, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    # twice the row-tiled entry's slabs for the same cfg fields
    mt = _lib.GemmCfg(_lib.GEMM_MT, 4, 1, 4, 2)
    assert need - 65792 == 2 * (L.nf4_gemm_bnb_mt_workspace_bytes(64, I, K, ctypes.byref(mt)) - 65792)
    # the library's choice for 1024 x 8192 splits K (whatever the CU count it finds)
    i, k = 1024, 8192
    lib_need = L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(64, i, k, None)
    assert lib_need > 65792 and (lib_need - 65792) % (2 * 64 * i * 4) == 0
    st = dict(n=i, plen=i * k // 2, nb=i * k // 64, n2=i * k // 64)
    assert _call(L, k=k, both=st) == _lib.ERR_ARG
    assert _call(L, single=1, k=k, both={**st, "nb": 0}) == _lib.ERR_ARG
    one = _lib.GemmCfg(_lib.GEMM_MT_SWIGLU, 4, 1, 1, 2)
    assert L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(64, I, K, ctypes.byref(one)) == 0
    assert L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(64, 96, K, None) == 0
    assert L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(0, I, K, None) == 0
    assert L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(129, I, K, None) == 0
