"""C ABI of the NF4 embedding gather: the four entries are exported with the ctypes
signatures the header declares, and bad arguments are rejected on the host before any
device work (fake non-null pointers, never dereferenced; no GPU needed)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x10000  # aligned, never dereferenced: every call below ends in validation
ENTRIES = ("nf4_embedding_bnb", "nf4_embedding_bnb_single", "nf4_embedding_bnb_cpu", "nf4_embedding_bnb_single_cpu")
P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


def test_symbols_and_signatures():
    L = _lib.lib()
    nested = [P, I32, I64, P, P, I64, P, P, I64, P, I32, I32, P, I32, I64, I64]
    single = [P, I32, I64, P, P, I64, I32, P, I32, I64, I64]
    want = {"nf4_embedding_bnb": nested + [P], "nf4_embedding_bnb_single": single + [P],
            "nf4_embedding_bnb_cpu": nested + [I32], "nf4_embedding_bnb_single_cpu": single + [I32]}
    for name in ENTRIES:
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        assert res == ctypes.c_int and args == want[name], name
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == want[name], name
    assert (_lib.IDS_I32, _lib.IDS_I64) == (0, 1)
    text = open(_lib.HEADER_PATH).read()
    assert "#define NF4DQ_IDS_I32 0" in text and "#define NF4DQ_IDS_I64 1" in text


def _nested(L, host, **kw):
    """nf4_embedding_bnb(_cpu) on a valid 10 x 128 call (20 blocks of 64, one absmax2), with overrides."""
    a = dict(ids=FAKE, ids_dtype=_lib.IDS_I64, count=4, packed=FAKE, absmax_q=FAKE, nb=20, code2=FAKE, absmax2=FAKE,
             n2=1, offset=None, blocksize=64, blocksize2=256, out=FAKE, out_dtype=_lib.BF16, rows=10, dim=128)
    a.update(kw)
    fn = L.nf4_embedding_bnb_cpu if host else L.nf4_embedding_bnb
    return fn(a["ids"], a["ids_dtype"], a["count"], a["packed"], a["absmax_q"], a["nb"], a["code2"], a["absmax2"],
              a["n2"], a["offset"], a["blocksize"], a["blocksize2"], a["out"], a["out_dtype"], a["rows"], a["dim"],
              1 if host else None)


def _single(L, host, **kw):
    a = dict(ids=FAKE, ids_dtype=_lib.IDS_I32, count=4, packed=FAKE, absmax=FAKE, nabs=20, blocksize=64, out=FAKE,
             out_dtype=_lib.F16, rows=10, dim=128)
    a.update(kw)
    fn = L.nf4_embedding_bnb_single_cpu if host else L.nf4_embedding_bnb_single
    return fn(a["ids"], a["ids_dtype"], a["count"], a["packed"], a["absmax"], a["nabs"], a["blocksize"], a["out"],
              a["out_dtype"], a["rows"], a["dim"], 1 if host else None)


NESTED_CASES = [
    (dict(count=0), _lib.OK),
    (dict(count=0, ids=None, packed=None, absmax_q=None, code2=None, absmax2=None, out=None), _lib.OK),
    (dict(ids=None), _lib.ERR_ARG),
    (dict(out=None), _lib.ERR_ARG),
    (dict(packed=None), _lib.ERR_ARG),
    (dict(absmax_q=None), _lib.ERR_ARG),
    (dict(absmax2=None), _lib.ERR_ARG),
    (dict(code2=None), _lib.ERR_ARG),
    (dict(ids_dtype=2), _lib.ERR_ARG),
    (dict(out_dtype=3), _lib.ERR_ARG),
    (dict(blocksize=32), _lib.ERR_ARG),
    (dict(blocksize=96), _lib.ERR_ARG),
    (dict(blocksize=8192), _lib.ERR_ARG),
    (dict(blocksize2=0), _lib.ERR_ARG),
    (dict(blocksize2=3), _lib.ERR_ARG),
    (dict(nb=19), _lib.ERR_SHAPE),
    (dict(n2=0), _lib.ERR_SHAPE),
    (dict(count=-1), _lib.ERR_SHAPE),
    (dict(rows=-1), _lib.ERR_SHAPE),
    (dict(dim=-1), _lib.ERR_SHAPE),
    (dict(dim=0), _lib.ERR_SHAPE),
    (dict(count=2 ** 24, nb=2 ** 40), _lib.ERR_TOO_LARGE),  # count * dim = 2^31
]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kw,want", NESTED_CASES, ids=[",".join(f"{k}={v}" for k, v in c[0].items())
                                                        for c in NESTED_CASES])
def test_nested_validation(host, kw, want):
    assert _nested(_lib.lib(), host, **kw) == want


SINGLE_CASES = [
    (dict(count=0), _lib.OK),
    (dict(ids=None), _lib.ERR_ARG),
    (dict(out=None), _lib.ERR_ARG),
    (dict(absmax=None), _lib.ERR_ARG),
    (dict(ids_dtype=2), _lib.ERR_ARG),
    (dict(out_dtype=3), _lib.ERR_ARG),
    (dict(blocksize=32), _lib.ERR_ARG),
    (dict(blocksize=96), _lib.ERR_ARG),
    (dict(blocksize=8192), _lib.ERR_ARG),
    (dict(nabs=19), _lib.ERR_SHAPE),
    (dict(count=-1), _lib.ERR_SHAPE),
    (dict(rows=-1), _lib.ERR_SHAPE),
    (dict(dim=-1), _lib.ERR_SHAPE),
]


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kw,want", SINGLE_CASES, ids=[",".join(f"{k}={v}" for k, v in c[0].items())
                                                        for c in SINGLE_CASES])
def test_single_validation(host, kw, want):
    assert _single(_lib.lib(), host, **kw) == want
