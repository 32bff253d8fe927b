"""nf4_lora_add: the header against the ctypes binding (symbol, constants, struct sizes), and every
validation rule answering its documented code before any device work (no GPU needed; fake
pointers as in test_gemm_moe_down_abi.py -- every call here fails validation, so none is ever
dereferenced or launched)."""
import ctypes
import re

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
           "int": ctypes.c_int}


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _mat(**over):
    f = dict(A=FAKE, B=FAKE, base=FAKE, y=FAKE, N=128, r=16, scale=0.5)
    f.update(over)
    return _lib.LoraMat(**f)


def _call(L, mats, *, x=FAKE, M=8, K=256, count=None, dt=_lib.BF16, cfg=None, null_mats=False):
    arr = (_lib.LoraMat * max(len(mats), 1))(*mats)
    mp = None if null_mats else ctypes.cast(arr, ctypes.c_void_p)
    cp = ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p) if cfg is not None else None
    return L.nf4_lora_add(x, M, K, mp, len(mats) if count is None else count, dt, cp, None)


# a cfg the plan rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the launch
BAD = dict(cfg=_lib.LoraCfg(48, 4))


def test_header_prototype_constants_and_structs(L):
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("NF4DQ_LORA_MAX_M", _lib.LORA_MAX_M), ("NF4DQ_LORA_MAX_R", _lib.LORA_MAX_R),
                        ("NF4DQ_LORA_GROUP_MAX", _lib.LORA_GROUP_MAX)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert (_lib.LORA_MAX_M, _lib.LORA_MAX_R, _lib.LORA_GROUP_MAX) == (128, 128, 8) and _lib.LORA_GROUP_MAX == _lib.GEMM_GROUP_MAX
    assert hasattr(L, "nf4_lora_add")
    m = re.search(r"^(\w+) nf4_lora_add\(([^;]*)\);", text, re.M | re.S)
    params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
    types = [C_TYPES[re.sub(r"\s*\w+$", "", p).strip()] for p in params]
    restype, argtypes = _lib.SIGNATURES["nf4_lora_add"]
    assert C_TYPES[m.group(1)] is restype and types == list(argtypes)
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == ["x", "M", "K", "mats", "count", "dtype", "cfg", "hip_stream"]
    # the descriptor: four pointers, N, r and the scale INSIDE the struct, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} nf4_lora_mat;", text, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.LoraMat._fields_] == ["A", "B", "base", "y", "N", "r", "scale"]
    assert ctypes.sizeof(_lib.LoraMat) == 48 and _lib.LoraMat.scale.offset == 44 and _lib.LoraMat.r.offset == 40
    body = re.search(r"typedef struct \{([^}]*)\} nf4_lora_cfg;", text, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in _lib.LoraCfg._fields_]
    assert ctypes.sizeof(_lib.LoraCfg) == 8


def test_arg_rules(L):
    good = [_mat()]
    assert _call(L, good, **BAD) == _lib.ERR_ARG                       # everything else right: ends at the cfg
    assert _call(L, good, x=None) == _lib.ERR_ARG
    assert _call(L, good, null_mats=True) == _lib.ERR_ARG
    for dt in (_lib.F32, 3, -1):
        assert _call(L, good, dt=dt) == _lib.ERR_ARG, dt
    for count in (0, -1, 9):
        assert _call(L, [_mat()] * 9, count=count) == _lib.ERR_ARG, count
    for name in ("A", "B", "y"):
        assert _call(L, [_mat(), _mat(**{name: None})]) == _lib.ERR_ARG, name
    for r in (0, 4, 7, 129, 136, -8):
        assert _call(L, [_mat(r=r)]) == _lib.ERR_ARG, r
    for cfg in ((0, 4), (8, 4), (48, 4), (512, 4), (64, 0), (64, 3), (64, 8)):
        assert _call(L, good, cfg=_lib.LoraCfg(*cfg)) == _lib.ERR_ARG, cfg
    # ARG answers before SHAPE
    assert _call(L, [_mat(N=120, r=4)], M=0, K=48) == _lib.ERR_ARG
    assert _call(L, good, M=129, **BAD) == _lib.ERR_ARG


def test_shape_and_alignment_rules(L):
    good = [_mat()]
    for M in (0, -1, 129, 1 << 20):
        assert _call(L, good, M=M) == _lib.ERR_SHAPE, M
    for K in (0, 16, 48, 100, -32):
        assert _call(L, good, K=K) == _lib.ERR_SHAPE, K
    for N in (0, 8, 24, 120, -16):
        assert _call(L, [_mat(), _mat(N=N)]) == _lib.ERR_SHAPE, N
    for r in (12, 20, 100):
        assert _call(L, [_mat(r=r)]) == _lib.ERR_SHAPE, r
    assert _call(L, good, x=FAKE + 8) == _lib.ERR_SHAPE
    for name in ("A", "B", "base", "y"):
        for off in (2, 4, 8):
            assert _call(L, [_mat(**{name: FAKE + off})]) == _lib.ERR_SHAPE, (name, off)
    assert _call(L, good, K=1 << 23) == _lib.ERR_TOO_LARGE
    assert _call(L, [_mat(N=1 << 23)]) == _lib.ERR_TOO_LARGE
    assert _call(L, [_mat(N=(1 << 23) + 8)]) == _lib.ERR_SHAPE


def test_the_edges_of_the_domain_pass_validation(L):
    """Calls that are valid but for a cfg the plan rejects: each reaches the cfg rule's code, which
    is checked AFTER every other ARG rule, so the rest of the call passed them; the SHAPE rules are
    then pinned from the other side in tests/test_lora_plan_cpu.py (ok_* lines)."""
    for kw in (dict(M=1), dict(M=128), dict(K=32), dict(dt=_lib.F16)):
        assert _call(L, [_mat()], **kw, **BAD) == _lib.ERR_ARG
    for m in (_mat(r=8), _mat(r=128), _mat(N=16), _mat(base=None), _mat(scale=float("nan"))):
        assert _call(L, [m] * 8, **BAD) == _lib.ERR_ARG
