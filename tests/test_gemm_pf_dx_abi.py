"""nf4_gemm_bnb_pf_dx / nf4_gemm_bnb_pf_dx_single: the exported symbols, the header's constant and
signatures, and every validation rule answering its code before any device work (no GPU needed;
fake pointers as in test_gemm_mt_abi.py -- every call here fails validation or has no rows, so
none is ever dereferenced or launched)."""
import ctypes
import re

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
N, K = 448, 384
NBLK = N * K // 64
N2 = -(-NBLK // 256)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _nested(L, *, g=FAKE, M=129, packed=FAKE, plen=None, a1=FAKE, nb=None, a2=FAKE, n2=None, bs=64, bs2=256, dx=FAKE,
            dt=_lib.BF16, n=N, k=K, ws=None, wsb=0, cfg=None):
    blocks = n * k // 64
    return L.nf4_gemm_bnb_pf_dx(g, M, packed, n * k // 2 if plen is None else plen, a1, blocks if nb is None else nb,
                                FAKE, a2, -(-blocks // bs2) if n2 is None else n2, None, bs, bs2, dx, dt, n, k, ws, wsb,
                                ctypes.byref(cfg) if cfg is not None else None, None)


def _single(L, *, g=FAKE, M=129, packed=FAKE, am=FAKE, nabs=None, bs=64, dx=FAKE, dt=_lib.BF16, n=N, k=K, ws=None,
            wsb=0, cfg=None):
    return L.nf4_gemm_bnb_pf_dx_single(g, M, packed, n * k // 2, am, n * k // 64 if nabs is None else nabs, bs, dx, dt, n,
                                       k, ws, wsb, ctypes.byref(cfg) if cfg is not None else None, None)


def test_symbols_constant_and_signatures(L):
    text = re.sub(r"\s+", " ", open(_lib.HEADER_PATH).read())
    assert f"#define NF4DQ_GEMM_PF_DX {_lib.GEMM_PF_DX} " in text and _lib.GEMM_PF_DX == 15
    tail = "void* workspace, size_t workspace_bytes, const nf4_gemm_cfg* cfg, void* hip_stream);"
    for name, proto in (
            ("nf4_gemm_bnb_pf_dx_workspace_bytes", "size_t nf4_gemm_bnb_pf_dx_workspace_bytes(int64_t M, int64_t N, int64_t K, "
                                                   "const nf4_gemm_cfg* cfg);"),
            ("nf4_gemm_bnb_pf_dx", "int nf4_gemm_bnb_pf_dx(const void* g, int64_t M, const uint8_t* packed, int64_t packed_len, "
                                   "const uint8_t* absmax_q, int64_t nb, const float* code2, const float* absmax2, int64_t n2, "
                                   "const float* offset, int32_t blocksize, int32_t blocksize2, void* dx, int32_t out_dtype, "
                                   "int64_t N, int64_t K, " + tail),
            ("nf4_gemm_bnb_pf_dx_single", "int nf4_gemm_bnb_pf_dx_single(const void* g, int64_t M, const uint8_t* packed, "
                                          "int64_t packed_len, const float* absmax, int64_t nabs, int32_t blocksize, void* dx, "
                                          "int32_t out_dtype, int64_t N, int64_t K, " + tail)):
        assert hasattr(L, name) and proto in text, name


def test_codes_in_pf_checks_order(L):
    bad = _lib.GemmCfg(_lib.GEMM_PF_DX, 3, 1, 1, 0)  # ends a call that passed every shape rule at NF4DQ_ERR_ARG
    for call in (_nested, _single):
        assert call(L, dt=_lib.F32) == _lib.ERR_ARG and call(L, M=-1) == _lib.ERR_ARG
        assert call(L, g=None) == _lib.ERR_ARG and call(L, dx=None) == _lib.ERR_ARG
        assert call(L, g=FAKE + 8) == _lib.ERR_ARG and call(L, packed=FAKE + 8) == _lib.ERR_ARG and call(L, dx=FAKE + 4) == _lib.ERR_ARG
        assert call(L, bs=96) == _lib.ERR_ARG and call(L, bs=128) == _lib.ERR_SHAPE
        assert call(L, M=8193) == _lib.ERR_SHAPE
        assert call(L, k=320) == _lib.ERR_SHAPE and call(L, k=64) == _lib.ERR_SHAPE   # K in 128s
        assert call(L, n=416) == _lib.ERR_SHAPE and call(L, n=32) == _lib.ERR_SHAPE   # N in 64s
        assert call(L, n=64, k=128, cfg=bad) == _lib.ERR_ARG                          # the smallest shape passes
        assert call(L, n=1 << 19, k=128) == _lib.ERR_TOO_LARGE
        assert call(L, M=8192, n=1 << 17, k=128) == _lib.ERR_TOO_LARGE                # g of 2 GiB
        assert call(L, M=0) == _lib.OK and call(L, M=0, k=320) == _lib.ERR_SHAPE      # no rows: nothing launched
    assert _nested(L, plen=N * K // 2 - 1) == _lib.ERR_SHAPE
    assert _nested(L, nb=NBLK - 1) == _lib.ERR_SHAPE and _nested(L, n2=N2 - 1) == _lib.ERR_SHAPE
    assert _nested(L, n2=N2, cfg=bad) == _lib.ERR_ARG and _single(L, nabs=NBLK - 1) == _lib.ERR_SHAPE


def test_named_cfg_and_workspace(L):
    DX = _lib.GEMM_PF_DX
    for cfg in (_lib.GemmCfg(DX, 2, 1, 1, 0), _lib.GemmCfg(DX, 4, 2, 1, 0), _lib.GemmCfg(DX, 4, 1, 0, 0),
                _lib.GemmCfg(DX, 4, 1, N // 64 + 1, 0),  # more slices than steps of N
                _lib.GemmCfg(DX, 8, 1, 1, 2), _lib.GemmCfg(_lib.GEMM_PF, 4, 1, 1, 0)):
        assert _nested(L, cfg=cfg) == _lib.ERR_ARG and _single(L, cfg=cfg) == _lib.ERR_ARG, (cfg.kernel, cfg.waves, cfg.ksplit)
        assert L.nf4_gemm_bnb_pf_dx_workspace_bytes(129, N, K, ctypes.byref(cfg)) == 0
    three = _lib.GemmCfg(0, 4, 1, 3, 0)  # kernel 0 = the entry's own
    need = L.nf4_gemm_bnb_pf_dx_workspace_bytes(129, N, K, ctypes.byref(three))
    assert need == 64 * 1024 + 256 + 3 * 129 * K * 4
    assert _nested(L, cfg=three) == _lib.ERR_ARG and _nested(L, cfg=three, ws=FAKE, wsb=need - 1) == _lib.ERR_ARG
    assert _single(L, cfg=three, ws=FAKE + 8, wsb=need) == _lib.ERR_ARG
    one = _lib.GemmCfg(DX, 8, 1, 1, 0)
    assert L.nf4_gemm_bnb_pf_dx_workspace_bytes(129, N, K, ctypes.byref(one)) == 0
    for shape in ((129, N, 320), (129, 416, K), (0, N, K), (8193, N, K)):
        assert L.nf4_gemm_bnb_pf_dx_workspace_bytes(*shape, None) == 0
