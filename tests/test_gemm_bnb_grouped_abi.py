"""nf4_gemm_bnb_grouped: every validation rule answers its code before any device work (no GPU
needed; fake pointers as in test_gemm_bnb_abi.py -- every call here either fails validation or
is a zero-size call, so none is ever dereferenced or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
K = 1024
NS = (64, 192, 64)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _mat(N, k=K, single=False, **over):
    nblk = N * k // max(over.get("blocksize", 64), 64)
    bs2 = over.get("blocksize2", 256)
    f = dict(packed=FAKE, packed_len=N * k // 2, absmax_q=None if single else FAKE, nb=0 if single else nblk,
             code2=None if single else FAKE, absmax2=FAKE, n2=nblk if single else -(-nblk // max(bs2, 1)),
             offset=None, blocksize=64, blocksize2=0 if single else 256, y=FAKE, N=N)
    f.update(over)
    return _lib.GemmBnbMat(*[f[n] for n, _ in _lib.GemmBnbMat._fields_])


def _call(L, mats, *, x=FAKE, M=4, k=K, single=0, dt=_lib.BF16, ws=None, wsb=0, cfg=None, count=None):
    arr = (_lib.GemmBnbMat * max(len(mats), 1))(*mats)
    n = len(mats) if count is None else count
    return L.nf4_gemm_bnb_grouped(x, M, k, ctypes.cast(arr, ctypes.c_void_p) if mats else None, n, single, dt, ws, wsb,
                                  ctypes.byref(cfg) if cfg is not None else None, None)


def _group(single=False, **over0):
    """The three-weight group, weight 0 with overrides."""
    return [_mat(NS[0], single=single, **over0)] + [_mat(N, single=single) for N in NS[1:]]


# a cfg no family accepts: whatever else is right, the call ends at NF4DQ_ERR_ARG before the
# workspace check and the launch -- so a rule that must NOT fire shows as ERR_ARG, not a launch
BAD = _lib.GemmCfg(_lib.GEMM_K128, 3, 1, 1, 1)


def test_symbols_and_binding(L):
    for name in ("nf4_gemm_bnb_grouped", "nf4_gemm_bnb_grouped_workspace_bytes"):
        assert hasattr(L, name)
        assert _lib.SIGNATURES[name][1][3 if name == "nf4_gemm_bnb_grouped" else 2] == ctypes.c_void_p  # mats
    assert ctypes.sizeof(_lib.GemmBnbMat) == 88


def test_zero_size_calls_are_ok(L):
    assert _call(L, []) == _lib.OK
    assert _call(L, _group(), M=0) == _lib.OK
    assert _call(L, _group(), M=0, x=None) == _lib.OK
    assert _call(L, [_mat(0), _mat(0)]) == _lib.OK                      # no columns at all
    assert _call(L, _group(single=True), M=0, single=1) == _lib.OK


def test_count_bounds(L):
    assert _call(L, _group(), count=-1) == _lib.ERR_ARG
    assert _call(L, [_mat(64)] * 9) == _lib.ERR_ARG                     # above NF4DQ_GEMM_GROUP_MAX
    assert _call(L, [_mat(64)] * 8, cfg=BAD) == _lib.ERR_ARG            # 8 are allowed: ends at the cfg
    assert L.nf4_gemm_bnb_grouped(FAKE, 4, K, None, 3, 0, _lib.BF16, None, 0, None, None) == _lib.ERR_ARG  # null mats


def test_argument_errors(L):
    assert _call(L, _group(), dt=_lib.F32) == _lib.ERR_ARG
    assert _call(L, _group(), M=-1) == _lib.ERR_ARG
    assert _call(L, _group(), k=-128) == _lib.ERR_ARG
    assert _call(L, _group(), x=None) == _lib.ERR_ARG
    g = _group()
    g[1].N = -64
    assert _call(L, g) == _lib.ERR_ARG


@pytest.mark.parametrize("which", [0, 2])
def test_null_fields_per_mode(L, which):
    for name in ("packed", "absmax_q", "code2", "absmax2", "y"):
        g = _group()
        setattr(g[which], name, None)
        assert _call(L, g) == _lib.ERR_ARG, name
    for name in ("packed", "absmax2", "y"):
        g = _group(single=True)
        setattr(g[which], name, None)
        assert _call(L, g, single=1) == _lib.ERR_ARG, name
    # single mode ignores absmax_q, code2, offset and blocksize2; a null offset is allowed when nested
    assert _call(L, _group(single=True), single=1, cfg=BAD) == _lib.ERR_ARG
    assert _call(L, _group(offset=None), cfg=BAD) == _lib.ERR_ARG


@pytest.mark.parametrize("bs", [0, 32, 96, 8192, -64])
def test_blocksize_must_be_a_power_of_two_64_to_4096(L, bs):
    assert _call(L, _group(blocksize=bs, nb=4096, n2=4096)) == _lib.ERR_ARG
    g = _group(single=True)
    g[2].blocksize = bs
    assert _call(L, g, single=1) == _lib.ERR_ARG


@pytest.mark.parametrize("bs2", [0, 1, 2, 3, 48, -256])
def test_blocksize2_must_be_a_power_of_two_from_4(L, bs2):
    g = _group()
    g[1].blocksize2 = bs2
    assert _call(L, g) == _lib.ERR_ARG


def test_shape_errors(L):
    assert _call(L, _group(), M=33) == _lib.ERR_SHAPE
    assert _call(L, _group(single=True), M=33, single=1) == _lib.ERR_SHAPE
    assert _call(L, [_mat(64), _mat(96)]) == _lib.ERR_SHAPE                         # N % 64
    assert _call(L, [_mat(64, k=1088), _mat(64, k=1088)], k=1088) == _lib.ERR_SHAPE  # K % 128
    assert _call(L, _group(packed_len=NS[0] * K // 2 - 1)) == _lib.ERR_SHAPE


def test_statistics_must_cover_every_weight(L):
    nblk = NS[0] * K // 64
    assert _call(L, _group(nb=nblk - 1)) == _lib.ERR_SHAPE
    assert _call(L, _group(n2=nblk // 256 - 1)) == _lib.ERR_SHAPE
    assert _call(L, _group(blocksize2=16, n2=nblk // 16 - 1)) == _lib.ERR_SHAPE
    assert _call(L, _group(blocksize2=16, n2=nblk // 16), cfg=BAD) == _lib.ERR_ARG   # enough: ends at the cfg
    assert _call(L, _group(blocksize=4096, nb=15, n2=1)) == _lib.ERR_SHAPE           # 64 x 1024 / 4096 = 16
    assert _call(L, _group(blocksize=4096, nb=16, n2=1), cfg=BAD) == _lib.ERR_ARG
    g = _group()
    g[2].nb -= 1                                                                     # the last weight's, too
    assert _call(L, g) == _lib.ERR_SHAPE
    assert _call(L, _group(single=True, n2=nblk - 1), single=1) == _lib.ERR_SHAPE
    assert _call(L, _group(single=True, n2=nblk), single=1, cfg=BAD) == _lib.ERR_ARG


def test_cfg_of_a_family_without_the_grouped_mode_or_invalid(L):
    K128, STREAM, PERSIST, XS, XR, GEMV = (_lib.GEMM_K128, _lib.GEMM_STREAM, _lib.GEMM_PERSIST, _lib.GEMM_XS,
                                          _lib.GEMM_XR, _lib.GEMM_GEMV)
    for cfg in (_lib.GemmCfg(STREAM, 8, 2, 1, 1),          # valid for nf4_gemm_ref_grouped: no bnb mode
                _lib.GemmCfg(XS, 4, 2, K // 128 // 2, 1),   # likewise
                _lib.GemmCfg(_lib.GEMM_SK, 8, 2, 1, 1),     # retired
                _lib.GemmCfg(9, 8, 2, 1, 1),                # unknown
                _lib.GemmCfg(K128, 3, 1, 1, 1),             # invalid waves
                _lib.GemmCfg(PERSIST, 8, 2, 3, 1),          # K slices not dividing K / 256
                _lib.GemmCfg(XR, 8, 2, 2, 2)):              # ksplit must be ceil(8 / 16) = 1
        assert _call(L, _group(), cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves)
        assert _call(L, _group(single=True), single=1, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves)
    # the decode GEMV has no grouped mode, not even at its own M = 1, K % 2048 == 0
    g = [_mat(64, k=2048), _mat(64, k=2048)]
    assert _call(L, g, M=1, k=2048, cfg=_lib.GemmCfg(GEMV, 16, 1, 1, 0)) == _lib.ERR_ARG
    # statistics blocks above 64 in any weight: the 128-deep kernel alone
    for cfg in (_lib.GemmCfg(PERSIST, 8, 2, 1, 1), _lib.GemmCfg(XR, 8, 2, 1, 1)):
        g = _group()
        g[1] = _mat(NS[1], blocksize=128)
        assert _call(L, g, cfg=cfg) == _lib.ERR_ARG
        gs = _group(single=True)
        gs[1] = _mat(NS[1], single=True, blocksize=128)
        assert _call(L, gs, single=1, cfg=cfg) == _lib.ERR_ARG
    # an empty weight under the persistent kernel: it cannot own strip groups
    g = [_mat(64), _mat(0), _mat(64)]
    assert _call(L, g, cfg=_lib.GemmCfg(PERSIST, 4, 2, 1, 2)) == _lib.ERR_SHAPE  # valid for the others at K = 1024
    assert _call(L, g, cfg=BAD) == _lib.ERR_ARG                                  # K128 takes it: ends at the cfg


def test_workspace_is_checked_before_the_launch(L):
    """A cfg with K slices needs a workspace: a null, short or misaligned one is NF4DQ_ERR_ARG;
    the size entry is that of nf4_gemm_ref_grouped for the same cfg and 0 for rejected shapes."""
    cfg = _lib.GemmCfg(_lib.GEMM_K128, 8, 1, 4, 1)
    g = _group()
    arr = (_lib.GemmBnbMat * 3)(*g)
    mp = ctypes.cast(arr, ctypes.c_void_p)
    need = L.nf4_gemm_bnb_grouped_workspace_bytes(4, K, mp, 3, 0, ctypes.byref(cfg))
    assert need == L.nf4_gemm_workspace_bytes_cfg(4, sum(NS), K, ctypes.byref(cfg)) > 0
    assert need == L.nf4_gemm_bnb_grouped_workspace_bytes(4, K, mp, 3, 1, ctypes.byref(cfg))
    assert _call(L, g, cfg=cfg) == _lib.ERR_ARG
    assert _call(L, g, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, g, cfg=cfg, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    assert L.nf4_gemm_bnb_grouped_workspace_bytes(0, K, mp, 3, 0, None) == 0
    assert L.nf4_gemm_bnb_grouped_workspace_bytes(4, 1088, mp, 3, 0, None) == 0
    assert L.nf4_gemm_bnb_grouped_workspace_bytes(4, K, mp, 9, 0, None) == 0
    assert L.nf4_gemm_bnb_grouped_workspace_bytes(4, K, None, 3, 0, None) == 0
    # the library's choice for a wide group at M = 12 splits K: the size entry is positive
    wide = [_mat(4096, k=4096), _mat(1024, k=4096), _mat(1024, k=4096)]
    arr2 = (_lib.GemmBnbMat * 3)(*wide)
    assert L.nf4_gemm_bnb_grouped_workspace_bytes(12, 4096, ctypes.cast(arr2, ctypes.c_void_p), 3, 0, None) > 0
    assert _call(L, wide, M=12, k=4096) == _lib.ERR_ARG  # ... and a call without it ends there
