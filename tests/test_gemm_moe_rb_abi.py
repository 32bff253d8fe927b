"""nf4_gemm_bnb_moe_rb: the header's defines, the symbols of the built library and every
validation rule answering its code before any device work (no GPU needed; fake pointers as in
test_gemm_moe_abi.py -- every call here fails validation or has no pair, so none is ever
dereferenced or launched).  The existing expert entries keep their 128-pair bound."""
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


def _ptr(ex):
    return ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p) if ex is not None else None


def _call(L, ex, *, x=FAKE, ids=FAKE, P=300, x_div=2, y=FAKE, dt=_lib.BF16, ws=None, wsb=0, cfg=None, entry="nf4_gemm_bnb_moe_rb"):
    return getattr(L, entry)(x, ids, P, x_div, _ptr(ex), y, dt, ws, wsb, ctypes.byref(cfg) if cfg is not None else None, None)


# a cfg the family rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the
# workspace check and the launch -- so a rule that must NOT fire shows as ERR_ARG, not a launch
BAD = dict(cfg=_lib.GemmCfg(_lib.GEMM_MOE_RB, 3, 1, 1, 2))


def test_symbols_and_constants(L):
    for name in ("nf4_gemm_bnb_moe_rb", "nf4_gemm_bnb_moe_rb_workspace_bytes"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["nf4_gemm_bnb_moe_rb"] == _lib.SIGNATURES["nf4_gemm_bnb_moe"]
    assert _lib.SIGNATURES["nf4_gemm_bnb_moe_rb_workspace_bytes"] == _lib.SIGNATURES["nf4_gemm_bnb_moe_workspace_bytes"]
    text = open(_lib.HEADER_PATH).read()
    assert f"#define NF4DQ_MOE_RB_MAX_PAIRS {_lib.MOE_RB_MAX_PAIRS}\n" in text and _lib.MOE_RB_MAX_PAIRS == 1024
    assert f"#define NF4DQ_GEMM_MOE_RB {_lib.GEMM_MOE_RB}\n" in text and _lib.GEMM_MOE_RB == _lib.GEMM_MOE_DOWN + 1
    assert "size_t nf4_gemm_bnb_moe_rb_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg);" in text
    assert "int nf4_gemm_bnb_moe_rb(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts," in text
    # the existing entry's bound is where it was
    assert "#define NF4DQ_MOE_MAX_PAIRS 128\n" in text and _lib.MOE_MAX_PAIRS == 128
    from nf4_triton_dequantization_amd import kernel

    assert (kernel.MOE_RB_ROUTED_MIN_P, kernel.MOE_RB_ROUTED_MAX_P) == (_lib.MOE_MAX_PAIRS + 1, _lib.MOE_RB_MAX_PAIRS)
    assert (kernel.MOE_SWIGLU_ROUTED_MAX_P, kernel.MOE_DOWN_ROUTED_MAX_P) == (128, 0)  # out of this entry's scope


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
        # an argument error comes before the shape: a bad dtype at 1025 pairs is ERR_ARG
        assert _call(L, ex(), P=1025, dt=7) == _lib.ERR_ARG
    for name in ("absmax_q", "code2"):
        assert _call(L, _experts(**{name: None})) == _lib.ERR_ARG, name
    for bs2 in (0, 2, 48):
        assert _call(L, _experts(blocksize2=bs2)) == _lib.ERR_ARG


def test_pair_bound_and_shape_errors(L):
    for single in (False, True):
        ex = lambda **o: _experts(single, **o)  # noqa: E731
        assert _call(L, ex(), P=1025) == _lib.ERR_SHAPE
        assert _call(L, ex(), P=1 << 20) == _lib.ERR_SHAPE
        for P in (1, 128, 129, 1024):                           # in the domain: ends at the cfg
            assert _call(L, ex(), P=P, **BAD) == _lib.ERR_ARG, P
        assert _call(L, ex(N=96, packed_stride=96 * K // 2)) == _lib.ERR_SHAPE
        assert _call(L, ex(N=0)) == _lib.ERR_SHAPE
        assert _call(L, ex(K=1088, packed_stride=N * 1088 // 2, nb_stride=N * 17, n2_stride=N * 17)) == _lib.ERR_SHAPE
        assert _call(L, ex(packed_stride=N * K // 2 - 16)) == _lib.ERR_SHAPE  # experts would overlap
        assert _call(L, ex(blocksize=128)) == _lib.ERR_SHAPE
        assert _call(L, ex(N=1 << 19, K=128, packed_stride=(1 << 19) * 64, nb_stride=1 << 20, n2_stride=1 << 20)) == \
            _lib.ERR_TOO_LARGE
        # the existing entries still end at 128 pairs
        assert _call(L, ex(), P=129, entry="nf4_gemm_bnb_moe") == _lib.ERR_SHAPE
    ex2 = (_lib.MoeExperts * 2)(_experts(), _experts())
    p2 = ctypes.cast(ex2, ctypes.c_void_p)
    assert L.nf4_gemm_bnb_moe_swiglu(FAKE, FAKE, 129, 2, p2, _lib.ACT_SILU, FAKE, _lib.BF16, None, 0, None, None) == _lib.ERR_SHAPE
    assert L.nf4_gemm_bnb_moe_down(FAKE, FAKE, 130, 2, 2, FAKE, 1, _ptr(_experts()), FAKE, _lib.BF16, FAKE, 1 << 30, None,
                                   None) == _lib.ERR_SHAPE
    assert _call(L, _experts(nb_stride=NBLK - 1)) == _lib.ERR_SHAPE
    assert _call(L, _experts(code2_stride=255)) == _lib.ERR_SHAPE


def test_named_cfg_never_falls_back(L):
    RB = _lib.GEMM_MOE_RB
    for cfg in (_lib.GemmCfg(RB, 3, 1, 1, 2),               # waves
                _lib.GemmCfg(RB, 8, 1, 1, 2),
                _lib.GemmCfg(RB, 4, 2, 1, 2),               # K stage
                _lib.GemmCfg(RB, 4, 1, 0, 2),               # K slices
                _lib.GemmCfg(RB, 4, 1, K // 128 + 1, 2),    # more slices than chunks
                _lib.GemmCfg(RB, 2, 1, 17, 2),              # more than 16
                _lib.GemmCfg(RB, 4, 1, 1, 1),               # strips per wave
                _lib.GemmCfg(_lib.GEMM_MOE, 4, 1, 1, 2),    # nf4_gemm_bnb_moe's cfg: another entry's
                _lib.GemmCfg(_lib.GEMM_MT, 4, 1, 1, 2),
                _lib.GemmCfg(14, 4, 1, 1, 2)):              # unknown
        for single in (False, True):
            for P in (64, 300):
                assert _call(L, _experts(single), P=P, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit)
    # ... and nf4_gemm_bnb_moe does not take this entry's number
    assert _call(L, _experts(), P=64, cfg=_lib.GemmCfg(RB, 4, 1, 1, 2), entry="nf4_gemm_bnb_moe") == _lib.ERR_ARG


def test_workspace_is_checked_before_the_launch(L):
    """K slices need a workspace: a null, short or misaligned one is NF4DQ_ERR_ARG; the size entry
    answers header + ksplit * P * N * 4 bytes (slabs indexed by pair: neither the experts nor the
    row blocks enter), and 0 for one slice or a rejected shape; more tickets than the header holds
    is NF4DQ_ERR_TOO_LARGE."""
    cfg = _lib.GemmCfg(_lib.GEMM_MOE_RB, 4, 1, 4, 2)
    ex = _experts()
    ep = _ptr(ex)
    need = L.nf4_gemm_bnb_moe_rb_workspace_bytes(300, ep, ctypes.byref(cfg))
    assert need == 64 * 1024 + 256 + 4 * 300 * N * 4
    assert _call(L, ex, cfg=cfg) == _lib.ERR_ARG
    assert _call(L, ex, cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, _experts(True), cfg=cfg, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _call(L, ex, cfg=cfg, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    one = _lib.GemmCfg(_lib.GEMM_MOE_RB, 4, 1, 1, 2)
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(300, ep, ctypes.byref(one)) == 0
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(0, ep, None) == 0
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(1025, ep, None) == 0
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(1025, ep, ctypes.byref(cfg)) == 0
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(1024, ep, ctypes.byref(cfg)) == 64 * 1024 + 256 + 4 * 1024 * N * 4
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(300, None, None) == 0
    assert L.nf4_gemm_bnb_moe_workspace_bytes(129, ep, None) == 0    # the existing entry's answer stays
    e96 = _experts(N=96)
    assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(300, _ptr(e96), None) == 0
    # Mixtral's shapes at 256 .. 1024 pairs: the library's choice is one K slice whatever the CU
    # count it finds (at most 256 a device): no workspace, no slab of 58 MB a slice
    for n, k in ((14336, 4096), (4096, 14336)):
        big = _experts(N=n, K=k, packed_stride=n * k // 2, nb_stride=n * k // 64, n2_stride=n * k // 64 // 256)
        for P in (256, 512, 1024):
            assert L.nf4_gemm_bnb_moe_rb_workspace_bytes(P, _ptr(big), None) == 0, (n, k, P)
    # 256 experts x 16 column tiles of 64 x 5 row blocks: 20480 tickets, the header holds 16384
    many = _experts(experts=256, N=1024, K=256, packed_stride=1024 * 128, nb_stride=1024 * 4, n2_stride=16)
    two = _lib.GemmCfg(_lib.GEMM_MOE_RB, 2, 1, 2, 2)
    assert _call(L, many, P=513, cfg=two, ws=FAKE, wsb=1 << 30) == _lib.ERR_TOO_LARGE
    assert _call(L, many, P=300, cfg=two, ws=FAKE, wsb=64) == _lib.ERR_ARG  # three row blocks fit: ends at the short workspace
