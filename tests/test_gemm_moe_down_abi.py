"""nf4_gemm_bnb_moe_down: the header against the ctypes signatures, and every validation rule
answering its code before any device work (no GPU needed; fake pointers as in
test_gemm_moe_abi.py -- every call here fails validation or has no pair, so none is ever
dereferenced or launched)."""
import ctypes
import re

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
E, N, K = 8, 128, 1024
NBLK = N * K // 64
HEADER = 64 * 1024 + 256
C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
           "size_t": ctypes.c_size_t, "const nf4_gemm_cfg*": ctypes.POINTER(_lib.GemmCfg), "int": ctypes.c_int}


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _experts(single=False, **over):
    f = dict(packed=FAKE, packed_stride=N * K // 2, absmax_q=None if single else FAKE, nb_stride=0 if single else NBLK,
             code2=None if single else FAKE, code2_stride=0, absmax2=FAKE, n2_stride=NBLK if single else NBLK // 256,
             offset=None, N=N, K=K, experts=E, single=int(single), blocksize=64, blocksize2=0 if single else 256)
    f.update(over)
    return _lib.MoeExperts(**f)


def _call(L, ex, *, x=FAKE, ids=FAKE, P=64, x_div=1, topk=2, rw=FAKE, rw_dt=_lib.F32, y=FAKE, dt=_lib.BF16, ws=FAKE,
          wsb=1 << 30, cfg=None):
    ep = ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p) if ex is not None else None
    return L.nf4_gemm_bnb_moe_down(x, ids, P, x_div, topk, rw, rw_dt, ep, y, dt, ws, wsb,
                                   ctypes.byref(cfg) if cfg is not None else None, None)


# a cfg the family rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the launch
BAD = dict(cfg=_lib.GemmCfg(_lib.GEMM_MOE_DOWN, 3, 1, 1, 2))


def test_header_prototypes_match_the_ctypes_signatures(L):
    text = open(_lib.HEADER_PATH).read()
    assert f"#define NF4DQ_GEMM_MOE_DOWN {_lib.GEMM_MOE_DOWN}\n" in text and _lib.GEMM_MOE_DOWN == _lib.GEMM_MOE_SWIGLU + 1
    for name in ("nf4_gemm_bnb_moe_down", "nf4_gemm_bnb_moe_down_workspace_bytes"):
        assert hasattr(L, name)
        m = re.search(r"^(\w+) " + name + r"\(([^;]*)\);", text, re.M | re.S)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(2).replace("\n", " ").split(",")]
        types = [C_TYPES[re.sub(r"\s*\w+$", "", p).strip()] for p in params]
        restype, argtypes = _lib.SIGNATURES[name]
        assert C_TYPES[m.group(1)] is restype and types == list(argtypes), (name, params)
    names = re.search(r"int nf4_gemm_bnb_moe_down\(([^;]*)\);", text, re.S).group(1)
    order = [re.search(r"(\w+)$", p.strip()).group(1) for p in names.replace("\n", " ").split(",")]
    assert order == ["x", "expert_ids", "P", "x_div", "topk", "routing_weights", "rw_dtype", "experts", "y", "out_dtype",
                     "workspace", "workspace_bytes", "cfg", "hip_stream"]


def test_no_pairs_is_ok_and_launches_nothing(L):
    for single in (False, True):
        assert _call(L, _experts(single), P=0, topk=0) == _lib.OK
        assert _call(L, _experts(single), P=0, x=None, ids=None, y=None, rw=None, ws=None, wsb=0) == _lib.OK
    assert _call(L, _experts(), P=0, dt=7) == _lib.ERR_ARG  # ... but the call is still validated
    assert _call(L, _experts(), P=0, rw_dt=7) == _lib.ERR_ARG


def test_the_combines_own_rules(L):
    for single in (False, True):
        ex = _experts(single)
        for topk in (0, -1, 3, 65, 128):                   # < 1, not dividing 64, beyond P
            assert _call(L, ex, topk=topk) == _lib.ERR_ARG, topk
        for topk in (1, 2, 32, 64):
            assert _call(L, ex, topk=topk, **BAD) == _lib.ERR_ARG  # allowed: ends at the cfg
        assert _call(L, ex, rw=None) == _lib.ERR_ARG
        assert _call(L, ex, rw=FAKE + 2) == _lib.ERR_ARG            # fp32 weights: 4-byte aligned
        assert _call(L, ex, rw=FAKE + 1, rw_dt=_lib.BF16) == _lib.ERR_ARG
        for rw_dt in (_lib.F16, 3, -1):                            # fp32 or the OUTPUT dtype, nothing else
            assert _call(L, ex, rw_dt=rw_dt) == _lib.ERR_ARG, rw_dt
        assert _call(L, ex, dt=_lib.F16, rw_dt=_lib.BF16) == _lib.ERR_ARG
        assert _call(L, ex, y=FAKE + 4) == _lib.ERR_ARG              # 8-byte stores of y


def test_the_expert_gemms_rules_with_its_codes(L):
    for single in (False, True):
        ex = lambda **o: _experts(single, **o)  # noqa: E731
        assert _call(L, ex(), dt=_lib.F32) == _lib.ERR_ARG
        assert _call(L, None) == _lib.ERR_ARG
        assert _call(L, ex(), P=-1) == _lib.ERR_ARG
        for name in ("x", "ids", "y"):
            assert _call(L, ex(), **{name: None}) == _lib.ERR_ARG, name
        assert _call(L, ex(), x_div=0) == _lib.ERR_ARG
        assert _call(L, ex(experts=257)) == _lib.ERR_ARG
        assert _call(L, ex(), x=FAKE + 8) == _lib.ERR_ARG
        assert _call(L, ex(), ids=FAKE + 2) == _lib.ERR_ARG
        assert _call(L, ex(), P=129, topk=1) == _lib.ERR_SHAPE
        assert _call(L, ex(), P=129, topk=0) == _lib.ERR_SHAPE      # the expert GEMM's rule answers first
        assert _call(L, ex(N=96, packed_stride=96 * K // 2)) == _lib.ERR_SHAPE
        assert _call(L, ex(K=1088, packed_stride=N * 1088 // 2, nb_stride=N * 17, n2_stride=N * 17)) == _lib.ERR_SHAPE
        assert _call(L, ex(blocksize=128)) == _lib.ERR_SHAPE
        assert _call(L, ex(packed_stride=N * K // 2 - 16)) == _lib.ERR_SHAPE
        assert _call(L, ex(N=1 << 19, K=128, packed_stride=(1 << 19) * 64, nb_stride=1 << 20, n2_stride=1 << 20)) == \
            _lib.ERR_TOO_LARGE


def test_named_cfg_never_falls_back(L):
    D = _lib.GEMM_MOE_DOWN
    for cfg in (_lib.GemmCfg(D, 3, 1, 1, 2), _lib.GemmCfg(D, 4, 2, 1, 2), _lib.GemmCfg(D, 4, 1, 0, 2),
                _lib.GemmCfg(D, 4, 1, K // 128 + 1, 2), _lib.GemmCfg(D, 2, 1, 17, 2), _lib.GemmCfg(D, 4, 1, 1, 1),
                _lib.GemmCfg(_lib.GEMM_MOE, 4, 1, 1, 2),          # the expert GEMM's own id
                _lib.GemmCfg(_lib.GEMM_MOE_SWIGLU, 4, 1, 1, 2), _lib.GemmCfg(13, 4, 1, 1, 2)):
        for single in (False, True):
            assert _call(L, _experts(single), cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit)
    # ... and the expert GEMM does not take this entry's number
    ex = _experts()
    assert L.nf4_gemm_bnb_moe(FAKE, FAKE, 64, 1, ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p), FAKE, _lib.BF16, None, 0,
                              ctypes.byref(_lib.GemmCfg(D, 4, 1, 1, 2)), None) == _lib.ERR_ARG


def test_workspace_is_never_empty_and_checked_before_the_launch(L):
    ex = _experts()
    ep = ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p)
    P = 64
    for ks in (1, 4):
        cfg = _lib.GemmCfg(_lib.GEMM_MOE_DOWN, 4, 1, ks, 2)
        need = L.nf4_gemm_bnb_moe_down_workspace_bytes(P, ep, ctypes.byref(cfg))
        assert need == HEADER + (ks * P * N * 4 if ks > 1 else 0) + P * N * 2
        assert _call(L, ex, cfg=cfg, ws=None, wsb=0) == _lib.ERR_ARG
        assert _call(L, ex, cfg=cfg, wsb=need - 1) == _lib.ERR_ARG
        assert _call(L, ex, cfg=cfg, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    assert L.nf4_gemm_bnb_moe_down_workspace_bytes(P, ep, None) >= HEADER + P * N * 2
    for bad_p in (0, 129):
        assert L.nf4_gemm_bnb_moe_down_workspace_bytes(bad_p, ep, None) == 0
    assert L.nf4_gemm_bnb_moe_down_workspace_bytes(P, None, None) == 0
    # (experts + 1) x column tiles tickets: 128 experts x 128 tiles of 64 columns do not fit, one slice or not
    many = _experts(experts=128, N=8192, K=256, packed_stride=8192 * 128, nb_stride=8192 * 4, n2_stride=128)
    for ks in (1, 2):
        assert _call(L, many, cfg=_lib.GemmCfg(_lib.GEMM_MOE_DOWN, 2, 1, ks, 2)) == _lib.ERR_TOO_LARGE
    fits = _experts(experts=127, N=8192, K=256, packed_stride=8192 * 128, nb_stride=8192 * 4, n2_stride=128)
    assert _call(L, fits, cfg=_lib.GemmCfg(_lib.GEMM_MOE_DOWN, 2, 1, 1, 2), wsb=16) == _lib.ERR_ARG  # ends at the workspace
