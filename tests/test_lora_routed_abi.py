"""nf4_lora_add_routed: the header against the ctypes binding (symbol, constants, struct field order
and size), and every validation rule answering its documented code before any device work (no GPU
needed; fake pointers as in test_lora_abi.py -- every call here fails validation, so none is ever
dereferenced or launched)."""
import ctypes
import re

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
           "int": ctypes.c_int}
K0, N0, R0 = 256, 128, 16


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _stack(**over):
    f = dict(A=FAKE, B=FAKE, scale=FAKE, base=FAKE, y=FAKE, N=N0, a_stride=R0 * K0, b_stride=N0 * R0, r=R0)
    f.update(over)
    return _lib.LoraStack(**f)


def _call(L, stacks, *, x=FAKE, ids=FAKE, M=8, K=K0, S=4, count=None, dt=_lib.BF16, cfg=None, null_stacks=False):
    arr = (_lib.LoraStack * max(len(stacks), 1))(*stacks)
    sp = None if null_stacks else ctypes.cast(arr, ctypes.c_void_p)
    cp = ctypes.cast(ctypes.pointer(cfg), ctypes.c_void_p) if cfg is not None else None
    return L.nf4_lora_add_routed(x, ids, M, K, S, sp, len(stacks) if count is None else count, dt, cp, None)


# a cfg the plan rejects: whatever else is right, the call ends at NF4DQ_ERR_ARG before the launch
BAD = dict(cfg=_lib.LoraCfg(48, 4))


def test_header_prototype_constants_and_struct(L):
    text = open(_lib.HEADER_PATH).read()
    assert re.search(rf"#define NF4DQ_LORA_MAX_ADAPTERS {_lib.LORA_MAX_ADAPTERS}\b", text) and _lib.LORA_MAX_ADAPTERS == 64
    assert hasattr(L, "nf4_lora_add_routed")
    m = re.search(r"^(\w+) nf4_lora_add_routed\(([^;]*)\);", text, re.M | re.S)
    params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
    types = [C_TYPES[re.sub(r"\s*\w+$", "", p).strip()] for p in params]
    restype, argtypes = _lib.SIGNATURES["nf4_lora_add_routed"]
    assert C_TYPES[m.group(1)] is restype and types == list(argtypes)
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == ["x", "adapter_ids", "M", "K", "adapters", "stacks", "count",
                                                                  "dtype", "cfg", "hip_stream"]
    # the descriptor: five pointers, N, the two strides and r, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} nf4_lora_stack;", text, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.LoraStack._fields_] == ["A", "B", "scale", "base", "y", "N", "a_stride", "b_stride", "r"]
    assert ctypes.sizeof(_lib.LoraStack) == 72 and _lib.LoraStack.r.offset == 64 and _lib.LoraStack.N.offset == 40
    assert _lib.LoraStack.a_stride.offset == 48 and _lib.LoraStack.b_stride.offset == 56


def test_arg_rules(L):
    good = [_stack()]
    assert _call(L, good, **BAD) == _lib.ERR_ARG                       # everything else right: ends at the cfg
    assert _call(L, good, x=None) == _lib.ERR_ARG
    assert _call(L, good, ids=None) == _lib.ERR_ARG
    assert _call(L, good, null_stacks=True) == _lib.ERR_ARG
    for dt in (_lib.F32, 3, -1):
        assert _call(L, good, dt=dt) == _lib.ERR_ARG, dt
    for count in (0, -1, 9):
        assert _call(L, [_stack()] * 9, count=count) == _lib.ERR_ARG, count
    for S in (0, -1, 65, 1 << 20):
        assert _call(L, good, S=S) == _lib.ERR_ARG, S
    for name in ("A", "B", "scale", "y"):
        assert _call(L, [_stack(), _stack(**{name: None})]) == _lib.ERR_ARG, name
    for r in (0, 4, 7, 129, 136, -8):
        assert _call(L, [_stack(r=r)]) == _lib.ERR_ARG, r
    for cfg in ((0, 4), (8, 4), (48, 4), (512, 4), (64, 0), (64, 3), (64, 8)):
        assert _call(L, good, cfg=_lib.LoraCfg(*cfg)) == _lib.ERR_ARG, cfg
    # ARG answers before SHAPE
    assert _call(L, [_stack(N=120, r=4)], M=0, K=48) == _lib.ERR_ARG
    assert _call(L, [_stack(a_stride=4)], S=65) == _lib.ERR_ARG
    assert _call(L, good, M=129, **BAD) == _lib.ERR_ARG


def test_shape_and_alignment_rules(L):
    good = [_stack()]
    for M in (0, -1, 129, 1 << 20):
        assert _call(L, good, M=M) == _lib.ERR_SHAPE, M
    for K in (0, 16, 48, 100, -32):
        assert _call(L, good, K=K) == _lib.ERR_SHAPE, K
    for N in (0, 8, 24, 120, -16):
        assert _call(L, [_stack(), _stack(N=N)]) == _lib.ERR_SHAPE, N
    for r in (12, 20, 100):
        assert _call(L, [_stack(r=r, a_stride=128 * K0, b_stride=N0 * 128)]) == _lib.ERR_SHAPE, r
    assert _call(L, good, x=FAKE + 8) == _lib.ERR_SHAPE
    for off in (1, 2, 3):
        assert _call(L, good, ids=FAKE + off) == _lib.ERR_SHAPE, off
    for name in ("A", "B", "base", "y"):
        for off in (2, 4, 8):
            assert _call(L, [_stack(**{name: FAKE + off})]) == _lib.ERR_SHAPE, (name, off)
    assert _call(L, [_stack(scale=FAKE + 2)]) == _lib.ERR_SHAPE
    for name, least in (("a_stride", R0 * K0), ("b_stride", N0 * R0)):
        for v in (least + 4, least + 1, least - 8, 0, -least):
            assert _call(L, [_stack(**{name: v})]) == _lib.ERR_SHAPE, (name, v)
    assert _call(L, good, K=2 * K0) == _lib.ERR_SHAPE                  # K beyond what a_stride holds
    assert _call(L, [_stack(a_stride=R0 << 23)], K=1 << 23) == _lib.ERR_TOO_LARGE
    assert _call(L, [_stack(N=1 << 23, b_stride=R0 << 23)]) == _lib.ERR_TOO_LARGE
    assert _call(L, [_stack(N=(1 << 23) + 8, b_stride=R0 << 24)]) == _lib.ERR_SHAPE
    for name in ("a_stride", "b_stride"):
        assert _call(L, [_stack(**{name: (1 << 40) + 8})]) == _lib.ERR_TOO_LARGE, name


def test_the_edges_of_the_domain_pass_validation(L):
    """Calls that are valid but for a cfg the plan rejects: each reaches the cfg rule's code, which
    is checked AFTER every other ARG rule, so the rest of the call passed them; the SHAPE rules are
    then pinned from the other side in tests/test_lora_routed_plan_cpu.py (ok_* lines)."""
    for kw in (dict(M=1), dict(M=128), dict(K=32), dict(dt=_lib.F16), dict(S=1), dict(S=64), dict(ids=FAKE + 4)):
        assert _call(L, [_stack()], **kw, **BAD) == _lib.ERR_ARG
    for s in (_stack(r=8), _stack(r=128), _stack(N=16), _stack(base=None), _stack(a_stride=R0 * K0 + 8)):
        assert _call(L, [s] * 8, **BAD) == _lib.ERR_ARG
