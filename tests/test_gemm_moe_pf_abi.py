"""nf4_gemm_bnb_moe_pf: the header's defines and prototypes, the bindings, the routed range and the
workspace formula, without a GPU (fake pointers as in test_gemm_moe_rb_abi.py: every call here
fails validation or has no pair, so none is dereferenced or launched)."""
import ctypes

import pytest

from nf4_triton_dequantization_amd import _lib

FAKE = 0x1000
E, N, K = 8, 256, 1024
PF = _lib.GEMM_MOE_PF if hasattr(_lib, "GEMM_MOE_PF") else 16


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _experts(**over):
    nblk = over.get("N", N) * over.get("K", K) // 64
    f = dict(packed=FAKE, packed_stride=over.get("N", N) * over.get("K", K) // 2, absmax_q=FAKE, nb_stride=nblk, code2=FAKE,
             code2_stride=0, absmax2=FAKE, n2_stride=nblk // 256 + 1, offset=None, N=N, K=K, experts=E, single=0,
             blocksize=64, blocksize2=256)
    f.update(over)
    return _lib.MoeExperts(**f)


def _ptr(ex):
    return ctypes.cast(ctypes.pointer(ex), ctypes.c_void_p)


def _need(P, experts, n, waves, ksplit):
    """The header comment's formula."""
    slots = -(-P // (32 * waves)) + min(experts + 1, P)
    tables = -(-(16 * slots + 4 * P + 4 * (experts + 1)) // 16) * 16
    return 65792 + (ksplit * P * n * 4 if ksplit > 1 else 0) + tables


def test_symbols_constants_and_the_empty_routed_range(L):
    for name in ("nf4_gemm_bnb_moe_pf", "nf4_gemm_bnb_moe_pf_workspace_bytes"):
        assert hasattr(L, name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_pf", "_rb")]
    text = open(_lib.HEADER_PATH).read()
    assert f"#define NF4DQ_MOE_PF_MAX_PAIRS {_lib.MOE_PF_MAX_PAIRS}\n" in text and _lib.MOE_PF_MAX_PAIRS == 16384
    assert f"#define NF4DQ_GEMM_MOE_PF {_lib.GEMM_MOE_PF}\n" in text and _lib.GEMM_MOE_PF == 16
    assert "size_t nf4_gemm_bnb_moe_pf_workspace_bytes(int64_t P, const void* experts, const nf4_gemm_cfg* cfg);" in text
    assert "int nf4_gemm_bnb_moe_pf(const void* x, const void* expert_ids, int64_t P, int32_t x_div, const void* experts," in text
    from nf4_triton_dequantization_amd import kernel, nf4_moe_linear_bnb_prefill  # noqa: F401

    assert (kernel.MOE_PF_ROUTED_MIN_P, kernel.MOE_PF_ROUTED_MAX_P) == (1, 0)
    assert (kernel.MOE_RB_ROUTED_MIN_P, kernel.MOE_RB_ROUTED_MAX_P) == (129, 1024)


@pytest.mark.parametrize("P,experts,waves,ksplit", [(1, 8, 4, 1), (300, 8, 4, 3), (300, 256, 8, 2), (16384, 8, 8, 1),
                                                     (16384, 256, 4, 16), (257, 1, 8, 16)])
def test_workspace_bytes_is_header_slabs_and_tables(L, P, experts, waves, ksplit):
    ex = _experts(experts=experts)
    cfg = _lib.GemmCfg(PF, waves, 1, ksplit, 0)
    assert L.nf4_gemm_bnb_moe_pf_workspace_bytes(P, _ptr(ex), ctypes.byref(cfg)) == _need(P, experts, N, waves, ksplit)
    got = L.nf4_gemm_bnb_moe_pf_workspace_bytes(P, _ptr(ex), None)  # the library's choice: never 0 for P >= 1
    assert got in {_need(P, experts, N, w, s) for w in (4, 8) for s in range(1, 17)}


def test_workspace_bytes_is_zero_for_what_the_entry_rejects(L):
    ok = _lib.GemmCfg(PF, 4, 1, 1, 0)
    size = L.nf4_gemm_bnb_moe_pf_workspace_bytes
    assert size(300, None, None) == 0
    for P in (0, -1, 16385):
        assert size(P, _ptr(_experts()), None) == 0 and size(P, _ptr(_experts()), ctypes.byref(ok)) == 0
    for over in (dict(N=192), dict(N=64), dict(K=192), dict(experts=0), dict(experts=257)):
        assert size(300, _ptr(_experts(**over)), None) == 0, over
    for cfg in (_lib.GemmCfg(PF, 2, 1, 1, 0), _lib.GemmCfg(PF, 4, 1, 17, 0), _lib.GemmCfg(PF, 4, 1, 1, 2),
                _lib.GemmCfg(_lib.GEMM_MOE_RB, 4, 1, 1, 0), _lib.GemmCfg(_lib.GEMM_PF, 4, 1, 1, 0)):
        assert size(300, _ptr(_experts()), ctypes.byref(cfg)) == 0, (cfg.kernel, cfg.waves, cfg.ksplit, cfg.strips)


def test_status_codes_in_moe_rb_checks_order(L):
    def call(ex, P=300, x=FAKE, ids=FAKE, y=FAKE, x_div=2, dt=_lib.BF16, ws=FAKE, wsb=1 << 40, cfg=None):
        return L.nf4_gemm_bnb_moe_pf(x, ids, P, x_div, _ptr(ex), y, dt, ws, wsb, ctypes.byref(cfg) if cfg is not None else None, None)

    bad = _lib.GemmCfg(PF, 3, 1, 1, 0)  # ends a call the rules accept at ERR_ARG, before any launch
    assert call(_experts(), P=0) == _lib.OK and call(_experts(), P=0, x=None, ids=None, y=None, ws=None, wsb=0) == _lib.OK
    assert call(_experts(), P=16385, dt=7) == _lib.ERR_ARG       # an argument error comes before the shape
    assert call(_experts(), ids=FAKE + 2) == _lib.ERR_ARG and call(_experts(), x_div=0) == _lib.ERR_ARG
    assert call(_experts(), P=16385) == _lib.ERR_SHAPE and call(_experts(), P=16384, cfg=bad) == _lib.ERR_ARG
    assert call(_experts(N=192)) == _lib.ERR_SHAPE and call(_experts(blocksize=128)) == _lib.ERR_SHAPE
    assert call(_experts(packed_stride=N * K // 2 - 16)) == _lib.ERR_SHAPE
    # P * N * 2 reaches 2^31 at N = 2^16 and 16384 pairs; x alone at K = 2^16 with a row per pair
    assert call(_experts(N=1 << 16, K=128), P=16384) == _lib.ERR_TOO_LARGE
    assert call(_experts(N=128, K=1 << 16), P=16384, x_div=1) == _lib.ERR_TOO_LARGE
    assert call(_experts(N=128, K=1 << 16), P=16384, x_div=2, cfg=bad) == _lib.ERR_ARG
    # 256 experts, 112 column tiles: (128 + 257) slots x 112 tickets do not fit the header under two slices ...
    many = _experts(experts=256, N=14336, K=4096)
    assert call(many, P=16384, cfg=_lib.GemmCfg(PF, 4, 1, 2, 0)) == _lib.ERR_TOO_LARGE
    # ... and the library's choice is never TOO_LARGE: it ends at the short workspace
    assert call(many, P=16384, wsb=64) == _lib.ERR_ARG
    assert call(_experts(N=14336, K=4096), P=16384, cfg=_lib.GemmCfg(PF, 8, 1, 5, 0)) == _lib.ERR_TOO_LARGE  # 4.7 GB of slabs
    assert call(_experts(N=14336, K=4096), P=16384, wsb=64) == _lib.ERR_ARG
    need = _need(300, E, N, 4, 1)
    assert call(_experts(), ws=None) == _lib.ERR_ARG and call(_experts(), wsb=need - 16, cfg=_lib.GemmCfg(PF, 4, 1, 1, 0)) == _lib.ERR_ARG
