"""nf4_gemm_bnb_moe_dec: the symbols and bindings, the empty routed range and the host-side rejections, without a GPU (fake pointers as in test_abi.py: every call here fails
validation or has no pair, so none is dereferenced or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
E, N, K = 8, 256, 2560  # 20 chunks: 16 waves of one chunk make two K slices


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _experts(**over):
    n, k = over.get("N", N), over.get("K", K)
    f = dict(packed=FAKE, packed_stride=n * k // 2, absmax_q=FAKE, nb_stride=n * k // 64, code2=FAKE, code2_stride=0,
             absmax2=FAKE, n2_stride=n * k // 64 // 256 + 1, offset=None, N=N, K=K, experts=E, single=0, blocksize=64,
             blocksize2=256)
    f.update(over)
    return _lib.MoeExperts(**f)


def _ptr(ex):
    return ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p)


def _cfg(waves, depth, strips, ksplit, kernel=17):
    return _lib.GemmCfg(kernel, waves, depth, ksplit, strips)


def test_symbols_constants_and_the_empty_routed_range(L):
    for name in ("nf4_gemm_bnb_moe_dec", "nf4_gemm_bnb_moe_dec_workspace_bytes"):
        assert hasattr(L, name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_dec", "")]
    assert f"#define NF4DQ_GEMM_MOE_DEC {_lib.GEMM_MOE_DEC}\n" in open(_lib.HEADER_PATH).read() and _lib.GEMM_MOE_DEC == 17
    from nf4_triton_dequantization_amd import kernel, nf4_moe_linear_bnb_decode  # noqa: F401

    assert (kernel.MOE_DEC_ROUTED_MIN_P, kernel.MOE_DEC_ROUTED_MAX_P) == (1, 0)


@pytest.mark.parametrize("what,over,kw,expect", [
    ("P = 0", {}, dict(P=0, x=None, ids=None, y=None), "OK"),
    ("an argument error comes before the shape", {}, dict(P=129, dt=7), "ERR_ARG"),
    ("P = 129", {}, dict(P=129), "ERR_SHAPE"),
    ("blocksize 128", dict(blocksize=128), {}, "ERR_SHAPE"),
    ("null ids", {}, dict(ids=None), "ERR_ARG"),
    ("more than 16 slices under every cfg", dict(K=128 * 513), {}, "ERR_TOO_LARGE"),
    ("cfg of nf4_gemm_bnb_moe", {}, dict(cfg=_lib.GemmCfg(_lib.GEMM_MOE, 4, 1, 1, 2)), "ERR_ARG"),
    ("ksplit off the rule", {}, dict(cfg=_cfg(16, 4, 1, 3)), "ERR_ARG"),
    ("four chunks per wave", {}, dict(cfg=_cfg(16, 2, 4, 1)), "ERR_ARG"),
    ("workspace 16 short", {}, dict(cfg=_cfg(16, 4, 1, 2), wsb=65792 + 2 * 100 * N * 4 - 16), "ERR_ARG"),
    ("tickets beyond the header", dict(experts=256, N=1 << 14), dict(P=128, cfg=_cfg(16, 4, 1, 2)), "ERR_TOO_LARGE"),
])
def test_host_side_rejections(L, what, over, kw, expect):
    a = dict(P=100, x=FAKE, ids=FAKE, y=FAKE, x_div=2, dt=_lib.BF16, ws=FAKE, wsb=1 << 40, cfg=None)
    a.update(kw)
    rc = L.nf4_gemm_bnb_moe_dec(a["x"], a["ids"], a["P"], a["x_div"], _ptr(_experts(**over)), a["y"], a["dt"], a["ws"], a["wsb"],
                                ctypes.byref(a["cfg"]) if a["cfg"] is not None else None, None)
    assert rc == getattr(_lib, expect), (what, _lib.strerror(rc))
