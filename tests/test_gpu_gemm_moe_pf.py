"""The fused expert GEMM for prompts (nf4_gemm_bnb_moe_pf: 1..16384 pairs, routed on the device)
through the C ABI on the GPU (``-m gpu``).

Every product is judged as test_gpu_gemm_moe.py judges nf4_gemm_bnb_moe's, with its stacks and its
check: the float64 oracle of the exact 16-bit weights OF THE PAIR'S EXPERT under the suite's GEMM
bound; a pair whose id is outside 0..E-1 must read as zero bits.  y is NaN-prefilled with a
sentinel band on either side.  After every call the WHOLE workspace -- tickets, slabs, routing
tables -- reads 0 and nf4_gemm_check_workspace is clean.

Shapes: E = 4 (once 256), N = 128 or 256, K = 256: four 64-deep steps, so 1, 2 and 3 K slices exist
and 3 leaves the last slice empty.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_gemm_moe as MOE

pytestmark = pytest.mark.gpu

PF, K, BAND = 16, 256, 8  # NF4DQ_GEMM_MOE_PF


def _cfg(waves, ksplit, kernel=PF):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(kernel, waves, 1, ksplit, 0)


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
    wsz = L.nf4_gemm_bnb_moe_pf_workspace_bytes(P, dp, cp)
    if ws is None:
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=S.gpu)
    sp = torch.cuda.current_stream().cuda_stream
    rc = L.nf4_gemm_bnb_moe_pf(xd.data_ptr(), ids.data_ptr() if ids_ptr and P else None, P, x_div, dp, y.data_ptr(),
                               _lib.BF16 if S.dt == "bf16" else _lib.F16, ws.data_ptr(), max(wsz - short, 0), cp, sp)
    assert rc == expect, (cfg and (cfg.waves, cfg.ksplit), _lib.strerror(rc))
    assert not wsz or L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), sp) == 0  # (0: a call the entry rejects)
    assert int(ws.count_nonzero()) == 0, f"tickets, slab entries or routing tables left set, cfg {cfg and (cfg.waves, cfg.ksplit)}"
    assert bool((buf[:BAND] == 0x5A5B).all()) and bool((buf[BAND + P:] == 0x5A5B).all()), "band written"
    return y


def _x(P, x_div, dt, gpu):
    xt, xb = MOE._x(-(-P // x_div), K, dt)
    return xt.to(gpu), xb


def _drawn(P, E, seed, idle=()):
    rng = np.random.default_rng(seed)
    live = [e for e in range(E) if e not in idle]
    w = rng.random(len(live)) + 0.2
    return np.asarray(live)[rng.choice(len(live), size=P, p=w / w.sum())]


@pytest.mark.parametrize("P", [1, 255, 256, 257, 513])
def test_block_edges_all_pairs_on_one_expert(coracle, gpu, P):
    """Every pair on expert 2: one row, a 256-row slot less one, full, plus one, and two full slots
    plus one; 128- and 256-row slots, one and three K slices (the third empty), and the library's choice."""
    S = MOE._stack(coracle, gpu, "nested", "drawn", 4, 256, K, "bf16")
    xd, xb = _x(P, 2, "bf16", gpu)
    ids = np.full(P, 2)
    for cfg in (_cfg(4, 1), _cfg(4, 3), _cfg(8, 1), _cfg(8, 3), None):
        MOE._check(S, _run(S, xd, ids, 2, cfg), xb, ids, 2, f"one expert P={P} cfg {cfg and (cfg.waves, cfg.ksplit)}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("P", [130, 1025, 16384])
def test_drawn_routings(coracle, gpu, dt, mode, P):
    """E = 4 with expert 2 idle, uneven drawn shares: at 16384 pairs the busiest expert fills many
    slots and its last one partly.  x per pair and shared by a token's two pairs."""
    S = MOE._stack(coracle, gpu, mode, "drawn", 4, 128, K, dt)
    ids = _drawn(P, 4, seed=P, idle=(2,))
    counts = np.bincount(ids, minlength=4)
    assert counts[2] == 0 and (counts[[0, 1, 3]] > 0).all() and (P < 16384 or (counts.max() > 2048 and counts.max() % 256))
    for x_div in (1, 2):
        xd, xb = _x(P, x_div, dt, gpu)
        for cfg in (None, _cfg(8, 2)):
            MOE._check(S, _run(S, xd, ids, x_div, cfg), xb, ids, x_div, f"drawn P={P} x_div={x_div} cfg {cfg and (8, 2)}")


def test_256_experts_at_300_pairs(coracle, gpu):
    """Most experts idle or holding one pair: ceil(300 / BM) + 257 slots launched, about 180 used."""
    S = MOE._stack(coracle, gpu, "nested", "drawn", 256, 128, K, "bf16")
    ids = _drawn(300, 256, seed=256, idle=(77,))
    ids[:40] = 5  # one expert with rows enough to matter beside the singles
    xd, xb = _x(300, 2, "bf16", gpu)
    for cfg in (None, _cfg(4, 2), _cfg(8, 1)):
        MOE._check(S, _run(S, xd, ids, 2, cfg), xb, ids, 2, f"256 experts cfg {cfg and (cfg.waves, cfg.ksplit)}")
    few = np.array([255, 0, 255])  # P below E + 1: the bound's other term
    MOE._check(S, _run(S, xd, few, 2), xb, few, 2, "3 pairs on 256 experts")


@pytest.mark.parametrize("cfg", [None, (4, 2), (8, 1)])
def test_invalid_ids_at_round_and_chunk_edges(coracle, gpu, cfg):
    """Ids outside 0..E-1 at pairs 63, 64 (a ballot round's edge), 1023, 1024 (a wave's chunk of 128
    ids ends at a multiple of it) and P - 1 of 1500: zero bits there, the neighbours pass; and one
    call whose every id is invalid."""
    E, P = 4, 1500
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, 128, K, "bf16")
    ids = _drawn(P, E, seed=5)
    at = [63, 64, 1023, 1024, P - 1]
    ids[at] = [-1, E, 2 ** 31 - 1, -2 ** 31, E + 1]
    xd, xb = _x(P, 2, "bf16", gpu)
    c = cfg and _cfg(*cfg)
    y = _run(S, xd, ids, 2, c)
    assert bool((y[at].view(torch.int16) == 0).all())
    MOE._check(S, y, xb, ids, 2, f"invalid ids cfg {cfg}")
    none = np.array([-1, E, 77, -5])[np.arange(200) % 4]
    assert int(_run(S, xd, none, 2, c).view(torch.int16).count_nonzero()) == 0


@pytest.mark.parametrize("waves,ksplit", [(4, 1), (8, 3)])
def test_a_rows_bits_are_the_prefill_kernels(coracle, gpu, waves, ksplit):
    """y[ids == e] equals nf4_gemm_bnb_pf on expert e's operands and the gathered rows of x at the
    same waves and ksplit, as int16 with no tolerance: the staging layout, the gather / scatter and
    the slice order in one comparison.  Twice on one workspace: equal bits."""
    _lib, L = MOE._lib_and_L()
    E, N, P = 4, 128, 700
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, N, K, "bf16")
    ids = _drawn(P, E, seed=9)
    ids[[3, 600]] = (-1, E)
    xd, xb = _x(P, 2, "bf16", gpu)
    cfg = _cfg(waves, ksplit)
    d = S.desc()
    ws = torch.zeros(L.nf4_gemm_bnb_moe_pf_workspace_bytes(P, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), ctypes.byref(cfg)),
                     dtype=torch.uint8, device=gpu)
    y = _run(S, xd, ids, 2, cfg, ws=ws).clone()
    assert torch.equal(_run(S, xd, ids, 2, cfg, ws=ws).view(torch.int16), y.view(torch.int16))
    MOE._check(S, y, xb, ids, 2, f"700 pairs cfg {(waves, ksplit)}")
    q, a1, c2, a2, off = S.t
    nblk, sp = N * K // 64, torch.cuda.current_stream().cuda_stream
    pcfg = _cfg(waves, ksplit, _lib.GEMM_PF)
    for e in range(E):
        sel = torch.from_numpy(np.nonzero(ids == e)[0]).to(gpu)
        M = int(sel.numel())
        xs = xd[sel // 2].contiguous()
        need = L.nf4_gemm_bnb_pf_workspace_bytes(M, N, K, ctypes.byref(pcfg))
        pws = torch.zeros(max(need, 16), dtype=torch.uint8, device=gpu)
        ref = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
        rc = L.nf4_gemm_bnb_pf(xs.data_ptr(), M, q[e].data_ptr(), N * K // 2, a1[e].data_ptr(), nblk, c2[e].data_ptr(),
                               a2[e].data_ptr(), -(-nblk // S.bs2), off[e:].data_ptr(), 64, S.bs2, ref.data_ptr(), _lib.BF16,
                               N, K, pws.data_ptr() if need else None, need, ctypes.byref(pcfg), sp)
        assert rc == 0, _lib.strerror(rc)
        same = ref.view(torch.int16) == y[sel].view(torch.int16)
        assert bool(same.all()), f"expert {e}, cfg {(waves, ksplit)}: {int((~same).sum())} of {same.numel()} outputs differ"


@pytest.mark.parametrize("what,expect", [("P=16385", "ERR_SHAPE"), ("N=192", "ERR_SHAPE"), ("blocksize=128", "ERR_SHAPE"),
                                         ("null ids", "ERR_ARG"), ("waves=2", "ERR_ARG"), ("ksplit=5", "ERR_ARG"),
                                         ("cfg of moe_rb", "ERR_ARG"), ("workspace 16 short", "ERR_ARG"), ("P=0", "OK")])
def test_status_codes_before_any_launch(coracle, gpu, what, expect):
    """Every rejected call leaves y NaN (and P = 0 has no y to touch)."""
    import copy

    _lib, _ = MOE._lib_and_L()
    S = MOE._stack(coracle, gpu, "nested", "drawn", 4, 128, K, "bf16")
    P = {"P=16385": 16385, "P=0": 0}.get(what, 300)
    xd, _ = _x(max(P, 2), 2, "bf16", gpu)
    if what in ("N=192", "blocksize=128"):
        S, real = copy.copy(S), S.desc

        def desc():
            d = real()
            d.N, d.blocksize = (192, 64) if what == "N=192" else (128, 128)
            return d
        S.desc, S.N = desc, 128  # (y keeps 128 columns: nothing may be stored)
    cfg = {"waves=2": _cfg(2, 1), "ksplit=5": _cfg(4, 5), "cfg of moe_rb": _cfg(4, 1, _lib.GEMM_MOE_RB)}.get(what)
    y = _run(S, xd, np.zeros(P, np.int64), 2, cfg, expect=getattr(_lib, expect), ids_ptr=what != "null ids",
             short=16 if what == "workspace 16 short" else 0)
    assert bool(torch.isnan(y.float()).all())
