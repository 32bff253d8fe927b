"""The fused expert GEMM for decode in 16-row slots (nf4_gemm_bnb_moe_dec: 1..128 pairs, routed on
the device) through the C ABI on the GPU (``-m gpu``).

Judged as test_gpu_gemm_moe.py judges nf4_gemm_bnb_moe (its stacks, its float64 oracle of the pair's expert,
zero bits for invalid ids), y NaN-prefilled between sentinel bands, the whole workspace 0 after every call.
K = 512: four chunks, so every cfg leaves waves without one; once K = 2560: two slices of 16 chunks, the second with four.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_gemm_moe as MOE
from test_gpu_gemm_moe_pf import _drawn

pytestmark = pytest.mark.gpu

DEC, K, BAND = 17, 512, 8  # NF4DQ_GEMM_MOE_DEC


def _cfg(waves, depth, strips, k=K, kernel=DEC, ksplit=None):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(kernel, waves, depth, -(-(k // 128) // (waves * strips)) if ksplit is None else ksplit, strips)


CFGS = [(8, 2, 1), (8, 4, 2), (16, 4, 1), (16, 2, 2), None]  # both wave counts, depths and chunk counts; the library's choice


def _run(S, xd, ids_np, x_div, cfg=None, ws=None, expect=0, ids_ptr=True, short=0):
    """One call into a NaN-filled y between two sentinel bands, on a fresh zeroed workspace unless one is given."""
    _lib, L = MOE._lib_and_L()
    P = len(ids_np)
    ids = torch.from_numpy(np.asarray(ids_np, np.int32)).to(S.gpu)
    buf = torch.full((BAND + P + BAND, S.N), 0x5A5B, dtype=torch.int16, device=S.gpu)
    y = buf[BAND:BAND + P].view(MOE._tdt(S.dt))
    y.fill_(float("nan"))
    cp = ctypes.byref(cfg) if cfg is not None else None
    d = S.desc()
    dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_moe_dec_workspace_bytes(P, dp, cp)
    if ws is None:
        ws = torch.zeros(max(wsz, 65536 + 256), dtype=torch.uint8, device=S.gpu)
    sp = torch.cuda.current_stream().cuda_stream
    rc = L.nf4_gemm_bnb_moe_dec(xd.data_ptr(), ids.data_ptr() if ids_ptr and P else None, P, x_div, dp, y.data_ptr(),
                                _lib.BF16 if S.dt == "bf16" else _lib.F16, ws.data_ptr(), max(wsz - short, 0), cp, sp)
    what = cfg and (cfg.waves, cfg.depth, cfg.strips, cfg.ksplit)
    assert rc == expect, (what, _lib.strerror(rc))
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), sp) == 0
    assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {what}"
    assert bool((buf[:BAND] == 0x5A5B).all()) and bool((buf[BAND + P:] == 0x5A5B).all()), "band written"
    return y


def _x(P, x_div, dt, gpu, k=K):
    xt, xb = MOE._x(-(-P // x_div), k, dt)
    return xt.to(gpu), xb


@pytest.mark.parametrize("P", [1, 15, 16, 17, 33, 128, "bound"])
def test_slot_edges_all_pairs_on_one_expert(coracle, gpu, P):
    """Every pair on expert 2: one row, a slot less one, full, plus one, two full slots plus one, eight slots;
    "bound": experts 0..2 with one pair each and expert 3 with 125, all 3 + 8 = 11 launched slots in use."""
    S = MOE._stack(coracle, gpu, "nested", "drawn", 4, 128, K, "bf16")
    ids = np.full(128 if P == "bound" else P, 3 if P == "bound" else 2)
    if P == "bound":
        P, ids[[5, 64, 127]] = 128, (0, 1, 2)
    xd, xb = _x(P, 2, "bf16", gpu)
    for c in CFGS:
        MOE._check(S, _run(S, xd, ids, 2, c and _cfg(*c)), xb, ids, 2, f"one expert P={P} cfg {c}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("P", [2, 40, 128])
def test_drawn_routings(coracle, gpu, dt, mode, P):
    """E = 4 with expert 2 idle, uneven drawn shares; x per pair and shared by a token's two pairs."""
    S = MOE._stack(coracle, gpu, mode, "drawn", 4, 128, K, dt)
    ids = _drawn(P, 4, seed=P, idle=(2,))
    for x_div in (1, 2):
        xd, xb = _x(P, x_div, dt, gpu)
        for c in (None, (8, 2, 2), (16, 4, 1)):
            MOE._check(S, _run(S, xd, ids, x_div, c and _cfg(*c)), xb, ids, x_div, f"drawn P={P} x_div={x_div} cfg {c}")


def test_256_experts(coracle, gpu):
    """128 pairs on 128 distinct experts of 256 (128 slots, all used, in expert order, not pair order); 3 pairs."""
    S = MOE._stack(coracle, gpu, "nested", "drawn", 256, 64, K, "bf16")
    ids = np.random.default_rng(3).permutation(256)[:128]
    xd, xb = _x(128, 2, "bf16", gpu)
    for c in (None, (8, 4, 1), (16, 2, 2)):
        MOE._check(S, _run(S, xd, ids, 2, c and _cfg(*c)), xb, ids, 2, f"256 experts cfg {c}")
    few = np.array([255, 0, 255])
    MOE._check(S, _run(S, xd, few, 2), xb, few, 2, "3 pairs on 256 experts")


@pytest.mark.parametrize("c", [None, (8, 2, 1), (16, 4, 2)])
def test_invalid_ids(coracle, gpu, c):
    """Ids outside 0..E-1 at pairs 0, 63, 64 (the two halves of the id read) and P - 1: zero bits there, the
    neighbours pass; and one call whose every id is invalid."""
    E, P = 4, 128
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, 128, K, "bf16")
    ids = _drawn(P, E, seed=5)
    at = [0, 63, 64, P - 1]
    ids[at] = [-1, E, 2 ** 31 - 1, -2 ** 31]
    xd, xb = _x(P, 2, "bf16", gpu)
    cfg = c and _cfg(*c)
    y = _run(S, xd, ids, 2, cfg)
    assert bool((y[at].view(torch.int16) == 0).all())
    MOE._check(S, y, xb, ids, 2, f"invalid ids cfg {c}")
    none = np.array([-1, E, 77, -5])[np.arange(100) % 4]
    assert int(_run(S, xd, none, 2, cfg).view(torch.int16).count_nonzero()) == 0


@pytest.mark.parametrize("c,k", [((8, 4, 1), K), ((16, 2, 2), K), ((16, 4, 1), 2560), ((8, 2, 2), 2560), ((8, 4, 1), 2560)])
def test_a_rows_bits_do_not_depend_on_the_batch(coracle, gpu, c, k):
    """y[p] of a drawn 128-pair batch equals, as int16 with no tolerance, the one-pair call on p's row of x and
    its id under the same cfg; and the same call twice on one workspace gives equal bits.  K = 2560: 16 + 4
    chunks in two slices under 16 waves x 1 and 8 waves x 2, 8 + 8 + 4 in three under 8 waves x 1."""
    _, L = MOE._lib_and_L()
    S = MOE._stack(coracle, gpu, "nested", "drawn", 4, 64 if k != K else 128, k, "bf16")
    ids = _drawn(128, 4, seed=9)
    xd, xb = _x(128, 1, "bf16", gpu, k)
    cfg = _cfg(*c, k=k)
    d = S.desc()
    ws = torch.zeros(max(L.nf4_gemm_bnb_moe_dec_workspace_bytes(128, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), ctypes.byref(cfg)),
                         65536 + 256), dtype=torch.uint8, device=gpu)
    y = _run(S, xd, ids, 1, cfg, ws=ws).clone()
    assert torch.equal(_run(S, xd, ids, 1, cfg, ws=ws).view(torch.int16), y.view(torch.int16))
    MOE._check(S, y, xb, ids, 1, f"128 pairs cfg {c}")
    for p in (0, 17, 63, 64, 127):
        one = _run(S, xd[p:p + 1].contiguous(), ids[p:p + 1], 1, cfg)
        assert torch.equal(one.view(torch.int16)[0], y.view(torch.int16)[p]), f"pair {p}, cfg {c}"


@pytest.mark.parametrize("what,expect", [("P=129", "ERR_SHAPE"), ("blocksize=128", "ERR_SHAPE"), ("null ids", "ERR_ARG"),
                                         ("cfg of moe", "ERR_ARG"), ("ksplit off the rule", "ERR_ARG"),
                                         ("workspace 16 short", "ERR_ARG"), ("P=0", "OK")])
def test_status_codes_before_any_launch(coracle, gpu, what, expect):
    """Every rejected call leaves y NaN (and P = 0 has no y to touch)."""
    import copy

    _lib, _ = MOE._lib_and_L()
    k = 2560 if what == "workspace 16 short" else K
    S = MOE._stack(coracle, gpu, "nested", "drawn", 4, 64 if k != K else 128, k, "bf16")
    P = {"P=129": 129, "P=0": 0}.get(what, 40)
    xd, _ = _x(max(P, 2), 2, "bf16", gpu, k)
    if what == "blocksize=128":
        S, real = copy.copy(S), S.desc

        def desc():
            d = real()
            d.blocksize = 128
            return d
        S.desc = desc
    cfg = {"cfg of moe": _lib.GemmCfg(_lib.GEMM_MOE, 4, 1, 1, 2), "ksplit off the rule": _cfg(8, 2, 1, ksplit=2),
           "workspace 16 short": _cfg(16, 4, 1, k=2560)}.get(what)
    y = _run(S, xd, np.zeros(P, np.int64), 2, cfg, expect=getattr(_lib, expect), ids_ptr=what != "null ids",
             short=16 if what == "workspace 16 short" else 0)
    assert bool(torch.isnan(y.float()).all())
