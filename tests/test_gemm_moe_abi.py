"""nf4_gemm_bnb_moe: every validation rule answers its code before any device work (no GPU
needed; fake pointers as in test_gemm_mt_abi.py -- every call here fails validation or has no
pair, so none is ever dereferenced or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
E, N, K = 8, 128, 1024
NBLK = N * K // 64


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _experts(single=False, **over):
    f = dict(packed=FAKE, packed_stride=N * K // 2, absmax_q=None if single else FAKE, nb_stride=0 if single else NBLK,
             code2=None if single else FAKE, code2_stride=0, absmax2=FAKE, n2_stride=NBLK if single else NBLK // 256,
             offset=None, N=N, K=K, experts=E, single=int(single), blocksize=64, blocksize2=0 if single else 256)
    f.update(over)
    return _lib.MoeExperts(**f)


def _call(L, ex, *, x=FAKE, ids=FAKE, P=64, x_div=2, y=FAKE, dt=_lib.BF16, ws=None, wsb=0, cfg=None):
    ep = ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p) if ex is not None else None
    return L.nf4_gemm_bnb_moe(x, ids, P, x_div, ep, y, dt, ws, wsb, ctypes.byref(cfg) if cfg is not None else None, None)


# a cfg the family rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the
# workspace check and the launch -- so a rule that must NOT fire shows as ERR_ARG, not a launch
BAD = dict(cfg=_lib.GemmCfg(_lib.GEMM_MOE, 3, 1, 1, 2))


def test_symbols_constants_and_struct(L):
    for name in ("nf4_gemm_bnb_moe", "nf4_gemm_bnb_moe_workspace_bytes"):
        assert hasattr(L, name)
    text = open(_lib.HEADER_PATH).read()
    assert f"#define NF4DQ_MOE_MAX_PAIRS {_lib.MOE_MAX_PAIRS}\n" in text and _lib.MOE_MAX_PAIRS == 128
    assert f"#define NF4DQ_MOE_MAX_EXPERTS {_lib.MOE_MAX_EXPERTS}\n" in text and _lib.MOE_MAX_EXPERTS == 256
    assert f"#define NF4DQ_GEMM_MOE {_lib.GEMM_MOE}\n" in text and _lib.GEMM_MOE == _lib.GEMM_MT + 1
    # 9 pointers / 64-bit fields, N and K, four 32-bit fields
    assert ctypes.sizeof(_lib.MoeExperts) == 9 * 8 + 2 * 8 + 4 * 4
    assert _lib.MoeExperts.experts.offset == 88 and _lib.MoeExperts.blocksize2.offset == 100


def test_no_pairs_is_ok_and_launches_nothing(L):
    for single in (False, True):
        assert _call(L, _experts(single), P=0) == _lib.OK
        assert _call(L, _experts(single), P=0, x=None, ids=None, y=None) == _lib.OK
    assert _call(L, _experts(), P=0, dt=7) == _lib.ERR_ARG  # ... but the call is still validated


def test_argument_errors(L):
    for single in (False, True):
        ex = lambda **o: _experts(single, **o)  # noqa: E731
        assert _call(L, ex(), dt=_lib.F32) == _lib.ERR_ARG  # 16-bit outputs only
        assert _call(L, ex(), dt=7) == _lib.ERR_ARG
        assert _call(L, None) == _lib.ERR_ARG
        assert _call(L, ex(), P=-1) == _lib.ERR_ARG
        for name in ("x", "ids", "y"):
            assert _call(L, ex(), **{name: None}) == _lib.ERR_ARG, name
        for name in ("packed", "absmax2"):
            assert _call(L, ex(**{name: None})) == _lib.ERR_ARG, name
        assert _call(L, ex(), x_div=0) == _lib.ERR_ARG
        assert _call(L, ex(), x_div=-2) == _lib.ERR_ARG
        for n in (0, -1, 257):
            assert _call(L, ex(experts=n)) == _lib.ERR_ARG, n
        assert _call(L, ex(experts=256), **BAD) == _lib.ERR_ARG  # 256 experts are allowed: ends at the cfg
        for bs in (0, 32, 96, 8192, -64):                        # no power of two in 64..4096
            assert _call(L, ex(blocksize=bs)) == _lib.ERR_ARG
        # 16-byte loads of x and every expert's packed weight, 8-byte stores of y, 4-byte ids
        assert _call(L, ex(), x=FAKE + 8) == _lib.ERR_ARG
        assert _call(L, ex(packed=FAKE + 4)) == _lib.ERR_ARG
        assert _call(L, ex(packed_stride=N * K // 2 + 8)) == _lib.ERR_ARG
        assert _call(L, ex(), y=FAKE + 2) == _lib.ERR_ARG
        assert _call(L, ex(), ids=FAKE + 2) == _lib.ERR_ARG
        assert _call(L, ex(packed_stride=-16)) == _lib.ERR_ARG
    for name in ("absmax_q", "code2"):
        assert _call(L, _experts(**{name: None})) == _lib.ERR_ARG, name
    assert _call(L, _experts(offset=None), **BAD) == _lib.ERR_ARG  # a null offset is allowed: ends at the cfg
    for bs2 in (0, 2, 48):
        assert _call(L, _experts(blocksize2=bs2)) == _lib.ERR_ARG


def test_shape_errors(L):
    for single in (False, True):
        ex = lambda **o: _experts(single, **o)  # noqa: E731
        assert _call(L, ex(), P=129) == _lib.ERR_SHAPE
        assert _call(L, ex(), P=128, **BAD) == _lib.ERR_ARG
        assert _call(L, ex(N=96, packed_stride=96 * K // 2)) == _lib.ERR_SHAPE
        assert _call(L, ex(N=0)) == _lib.ERR_SHAPE
        assert _call(L, ex(K=1088, packed_stride=N * 1088 // 2, nb_stride=N * 17, n2_stride=N * 17)) == _lib.ERR_SHAPE
        assert _call(L, ex(K=0)) == _lib.ERR_SHAPE
        assert _call(L, ex(packed_stride=N * K // 2 - 16)) == _lib.ERR_SHAPE  # experts would overlap
        assert _call(L, ex(packed_stride=N * K // 2 + 4096), **BAD) == _lib.ERR_ARG  # padding between experts is fine
        # a larger statistics block is valid elsewhere and out of this entry's domain
        assert _call(L, ex(blocksize=128)) == _lib.ERR_SHAPE
        assert _call(L, ex(N=1 << 19, K=128, packed_stride=(1 << 19) * 64, nb_stride=1 << 20, n2_stride=1 << 20)) == \
            _lib.ERR_TOO_LARGE
    assert _call(L, _experts(nb_stride=NBLK - 1)) == _lib.ERR_SHAPE
    assert _call(L, _experts(n2_stride=NBLK // 256 - 1)) == _lib.ERR_SHAPE
    assert _call(L, _experts(blocksize2=16, n2_stride=NBLK // 16 - 1)) == _lib.ERR_SHAPE
    assert _call(L, _experts(blocksize2=16, n2_stride=NBLK // 16), **BAD) == _lib.ERR_ARG  # enough: ends at the cfg
    assert _call(L, _experts(True, n2_stride=NBLK - 1)) == _lib.ERR_SHAPE
    assert _call(L, _experts(code2_stride=255)) == _lib.ERR_SHAPE  # tables would overlap
    assert _call(L, _experts(code2_stride=256), **BAD) == _lib.ERR_ARG
    assert _call(L, _experts(code2_stride=-256)) == _lib.ERR_ARG


def test_named_cfg_never_falls_back(L):
    MOE = _lib.GEMM_MOE
    for cfg in (_lib.GemmCfg(MOE, 3, 1, 1, 2),               # waves
                _lib.GemmCfg(MOE, 8, 1, 1, 2),
                _lib.GemmCfg(MOE, 4, 2, 1, 2),               # K stage
                _lib.GemmCfg(MOE, 4, 1, 0, 2),               # K slices
                _lib.GemmCfg(MOE, 4, 1, K // 128 + 1, 2),    # more slices than chunks
                _lib.GemmCfg(MOE, 2, 1, 17, 2),              # more than 16
                _lib.GemmCfg(MOE, 4, 1, 1, 1),               # strips per wave
                _lib.GemmCfg(_lib.GEMM_MT, 4, 1, 1, 2),      # another family's cfg
                _lib.GemmCfg(10, 4, 1, 1, 2)):               # unknown
        for single in (False, True):
            assert _call(L, _experts(single), cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit)
    # 128-column workgroups need N % 128 == 0
    wide = dict(N=192, packed_stride=192 * K // 2, nb_stride=192 * K // 64, n2_stride=192 * K // 64 // 256)
    assert _call(L, _experts(**wide), cfg=_lib.GemmCfg(MOE, 4, 1, 1, 2)) == _lib.ERR_ARG
    assert _call(L, _experts(**wide), cfg=_lib.GemmCfg(MOE, 2, 1, 0, 2)) == _lib.ERR_ARG  # 64-column ones fit: ends at ksplit 0
    # ... and the other entries do not take this family's number
    assert L.nf4_gemm_bnb_mt(FAKE, 64, FAKE, N * K // 2, FAKE, NBLK, FAKE, FAKE, NBLK // 256, None, 64, 256, FAKE,
                             _lib.BF16, N, K, None, 0, ctypes.byref(_lib.GemmCfg(MOE, 4, 1, 1, 2)), None) == _lib.ERR_ARG


def test_workspace_is_checked_before_the_launch(L):
    """K slices need a workspace: a null, short or misaligned one is NF4DQ_ERR_ARG; the size entry
    answers header + ksplit * P * N * 4 bytes (slabs indexed by pair: the expert count does not
    enter), and 0 for one slice or a rejected shape; more tickets than the header holds is
    NF4DQ_ERR_TOO_LARGE."""
    cfg = _lib.GemmCfg(_lib.GEMM_MOE, 4, 1, 4, 2)
    ex = _experts()
    ep = ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p)
    need = L.nf4_gemm_bnb_moe_workspace_bytes(64, ep, ctypes.byref(cfg))
    assert need == 64 * 1024 + 256 + 4 * 64 * N * 4
    assert _call(L, ex, cfg=cfg) == _lib.ERR_ARG
    assert _call(L, ex, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, _experts(True), cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, ex, cfg=cfg, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    one = _lib.GemmCfg(_lib.GEMM_MOE, 4, 1, 1, 2)
    assert L.nf4_gemm_bnb_moe_workspace_bytes(64, ep, ctypes.byref(one)) == 0
    assert L.nf4_gemm_bnb_moe_workspace_bytes(0, ep, None) == 0
    assert L.nf4_gemm_bnb_moe_workspace_bytes(129, ep, None) == 0
    assert L.nf4_gemm_bnb_moe_workspace_bytes(64, None, None) == 0
    e96 = _experts(N=96)
    assert L.nf4_gemm_bnb_moe_workspace_bytes(64, ctypes.cast(ctypes.pointer(e96), ctypes.c_void_p), None) == 0
    # the library's choice for Mixtral's w2 at one token splits K (whatever the CU count it finds)
    n, k = 4096, 14336
    big = _experts(N=n, K=k, packed_stride=n * k // 2, nb_stride=n * k // 64, n2_stride=n * k // 64 // 256)
    bp = ctypes.cast(ctypes.pointer(big), ctypes.c_void_p)
    lib_need = L.nf4_gemm_bnb_moe_workspace_bytes(2, bp, None)
    assert lib_need > 64 * 1024 + 256 and (lib_need - 64 * 1024 - 256) % (2 * n * 4) == 0
    assert _call(L, big, P=2) == _lib.ERR_ARG  # no workspace given
    # 256 experts x 128 column tiles of 64: 32768 tickets, the header holds 16384
    many = _experts(experts=256, N=8192, K=256, packed_stride=8192 * 128, nb_stride=8192 * 4, n2_stride=128)
    two = _lib.GemmCfg(_lib.GEMM_MOE, 2, 1, 2, 2)
    assert _call(L, many, cfg=two, ws=FAKE, wsb=1 << 30) == _lib.ERR_TOO_LARGE
