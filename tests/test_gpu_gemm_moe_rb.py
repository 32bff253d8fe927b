"""The fused expert GEMM in row blocks of 128 listed rows (nf4_gemm_bnb_moe_rb: up to 1024 pairs
in one launch) through the C ABI on the GPU (``-m gpu``).

Every product is judged as test_gpu_gemm_moe.py judges nf4_gemm_bnb_moe's, with its stacks and
its check: against the float64 oracle of the C oracle's exact 16-bit weights OF THE PAIR'S EXPERT
with the suite's GEMM bound (``_gemm_cases.gemm_oracle`` / ``check_close``); a pair whose id is
outside 0..E-1 must read as zero bits.  Outputs are NaN-prefilled, so a row never stored fails.
After every call that had a workspace the whole workspace reads 0 again (tickets and slabs) and
nf4_gemm_check_workspace is clean.

Shapes: E = 4 (once 256), N = 64 or 128, K = 256 -- two 128-deep chunks, so one and two K slices
both exist; the pair counts sit on the edges of the 128-row blocks and of the 64-id ballot rounds.
The exact-weight test walks the identity at 1024 pairs; every other shape, stack form, K-slice count
and routing is drawn: test_gpu_gemm_moe_rb_drawn.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_gemm_moe as MOE

pytestmark = pytest.mark.gpu

RB = 13  # NF4DQ_GEMM_MOE_RB
K = 256


def _cfg(waves, ksplit, kernel=RB):
    from nf4_triton_dequantization_amd import _lib

    return _lib.GemmCfg(kernel, waves, 1, ksplit, 2)


def _tag(cfg):
    return cfg and (cfg.waves, cfg.ksplit)


def _call(S, x_ptr, ids, P, x_div, y_ptr, cfg=None, ws=None, expect=0):
    """One call of nf4_gemm_bnb_moe_rb; with ws None a fresh zeroed workspace, checked clean and zero afterwards."""
    _lib, L = MOE._lib_and_L()
    cp = ctypes.byref(cfg) if cfg is not None else None
    d = S.desc()
    dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_moe_rb_workspace_bytes(P, dp, cp)
    if cfg is not None:
        assert wsz == (64 * 1024 + 256 + cfg.ksplit * P * S.N * 4 if cfg.ksplit > 1 else 0)
    own = ws is None
    if own:
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=S.gpu)
    assert ws.numel() >= wsz
    assert ids.dtype == torch.int32 and ids.numel() == P and ids.is_contiguous()
    sp = torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 if S.dt == "bf16" else _lib.F16
    rc = L.nf4_gemm_bnb_moe_rb(x_ptr, ids.data_ptr(), P, x_div, dp, y_ptr, code, ws.data_ptr() if wsz else None, wsz, cp, sp)
    assert rc == expect, (_tag(cfg), _lib.strerror(rc))
    if own and wsz:
        assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {_tag(cfg)}"
    return wsz


def _rb(S, xd, ids_np, x_div, cfg=None, ws=None):
    P = len(ids_np)
    ids = torch.from_numpy(np.asarray(ids_np, np.int32)).to(S.gpu)
    y = torch.full((P, S.N), float("nan"), dtype=MOE._tdt(S.dt), device=S.gpu)
    _call(S, xd.data_ptr(), ids, P, x_div, y.data_ptr(), cfg, ws)
    return y


def _x(P, x_div, dt, gpu):
    xt, xb = MOE._x(-(-P // x_div), K, dt)
    return xt.to(gpu), xb


def _drawn(P, E, seed, idle=()):
    """A drawn routing with uneven shares; the experts of ``idle`` get no pair."""
    rng = np.random.default_rng(seed)
    live = [e for e in range(E) if e not in idle]
    w = rng.random(len(live)) + 0.2
    return np.asarray(live)[rng.choice(len(live), size=P, p=w / w.sum())]


# ---- block edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [129, 256, 257, 300])
def test_block_edges_all_pairs_on_one_expert(coracle, gpu, P):
    """Every pair on expert 2, the others idle: 128 + 1 rows, exactly two blocks, two blocks + 1 and
    a last block of 44 rows.  64- and 128-column workgroups, one and two K slices, and the
    library's choice; x shared by a token's two pairs."""
    S = MOE._stack(coracle, gpu, "nested", "drawn", 4, 128, K, "bf16")
    xd, xb = _x(P, 2, "bf16", gpu)
    ids = np.full(P, 2)
    for cfg in (_cfg(2, 1), _cfg(2, 2), _cfg(4, 1), _cfg(4, 2), None):
        MOE._check(S, _rb(S, xd, ids, 2, cfg), xb, ids, 2, f"one expert P={P} cfg {_tag(cfg)}")


# ---- drawn routings --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("P", [130, 300, 1024])
def test_drawn_routings(coracle, gpu, dt, mode, P):
    """E = 4, N = 64, uneven drawn shares with expert 2 idle: at 1024 pairs the busiest expert fills
    several row blocks and the last of them partly.  x per pair (x_div 1) and shared by a token's
    two pairs (x_div 2); the library's choice and two K slices."""
    S = MOE._stack(coracle, gpu, mode, "drawn", 4, 64, K, dt)
    ids = _drawn(P, 4, seed=P, idle=(2,))
    counts = np.bincount(ids, minlength=4)
    assert counts[2] == 0 and (counts[[0, 1, 3]] > 0).all() and (P < 1024 or counts.max() > 256)
    for x_div in (1, 2):
        xd, xb = _x(P, x_div, dt, gpu)
        for cfg in (None, _cfg(2, 2)):
            MOE._check(S, _rb(S, xd, ids, x_div, cfg), xb, ids, x_div, f"drawn P={P} x_div={x_div} {mode} {dt} cfg {_tag(cfg)}")


# ---- invalid ids -----------------------------------------------------------------------------------
@pytest.mark.parametrize("idle0", [False, True])
def test_invalid_ids_across_the_ballot_rounds(coracle, gpu, idle0):
    """Ids outside 0..E-1 at pairs 63, 64, 127, 128, 191, 192 and P - 1 of 300: the last lane of a
    ballot round and the first of the next, beyond nf4_gemm_bnb_moe's two rounds.  Their rows are
    zero bits -- also with expert 0 idle, whose workgroups do the zeroing -- and every other row,
    their neighbours included, passes the oracle.  y sits between two sentinel bands."""
    E, N, P, band = 4, 128, 300, 16
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, N, K, "bf16")
    ids = _drawn(P, E, seed=5, idle=(0,) if idle0 else ())
    at = [63, 64, 127, 128, 191, 192, P - 1]
    ids[at] = [-1, E, 2 ** 31 - 1, -2 ** 31, E + 1, -7, E]
    idt = torch.from_numpy(ids.astype(np.int32)).to(gpu)
    xd, xb = _x(P, 2, "bf16", gpu)
    for cfg in (None, _cfg(2, 2), _cfg(4, 1)):
        buf = torch.full((band + P + band, N), 0x5A5B, dtype=torch.int16, device=gpu)
        buf[band:band + P] = torch.full((P, N), float("nan"), dtype=torch.bfloat16, device=gpu).view(torch.int16)
        y = buf[band:band + P].view(torch.bfloat16)
        _call(S, xd.data_ptr(), idt, P, 2, y.data_ptr(), cfg)
        what = f"invalid ids, expert 0 {'idle' if idle0 else 'busy'}, cfg {_tag(cfg)}"
        assert bool((buf[:band] == 0x5A5B).all()) and bool((buf[band + P:] == 0x5A5B).all()), f"band written: {what}"
        assert bool((y[at].view(torch.int16) == 0).all()), what
        MOE._check(S, y, xb, ids, 2, what)


# ---- row independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("waves,ksplit", [(2, 1), (2, 2), (4, 2)])
def test_every_row_has_the_bits_of_the_128_pair_entry(coracle, gpu, waves, ksplit):
    """A row's fp32 sum depends on the chunk order and the K slices alone -- not on the row block,
    the row tile or the other rows of the launch.  So at 300 pairs under an explicit cfg every
    row's bits equal those nf4_gemm_bnb_moe stores for that row within ANY subset of at most 128
    pairs at the NF4DQ_GEMM_MOE cfg of the same waves and ksplit: the three consecutive blocks of
    the pairs, and every third pair.  And up to 128 pairs the two entries' outputs are equal bit
    for bit, under the explicit cfg and under each library's own choice."""
    E, N, P = 4, 128, 300
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, N, K, "bf16")
    ids = _drawn(P, E, seed=11)
    ids[[5, 200]] = (-1, E)
    xd, xb = _x(P, 2, "bf16", gpu)
    y = _rb(S, xd, ids, 2, _cfg(waves, ksplit))
    MOE._check(S, y, xb, ids, 2, f"300 pairs cfg {(waves, ksplit)}")
    for name, sel in (("pairs 0..127", np.arange(0, 128)), ("pairs 128..255", np.arange(128, 256)),
                      ("pairs 256..299", np.arange(256, 300)), ("every third pair", np.arange(0, P, 3))):
        xs = xd[torch.from_numpy(sel // 2).to(gpu)].contiguous()      # the subset's rows of x, one per pair
        sub = MOE._moe(S, xs, ids[sel], 1, _cfg(waves, ksplit, MOE.MOE))
        same = sub.view(torch.int16) == y[torch.from_numpy(sel).to(gpu)].view(torch.int16)
        assert bool(same.all()), f"{name}, cfg {(waves, ksplit)}: {int((~same).sum())} of {same.numel()} outputs differ"
    for Q in (17, 100, 128):
        small = ids[:Q]
        xq, _ = _x(Q, 2, "bf16", gpu)
        for rb_cfg, moe_cfg in ((_cfg(waves, ksplit), _cfg(waves, ksplit, MOE.MOE)), (None, None)):
            a, b = _rb(S, xq, small, 2, rb_cfg), MOE._moe(S, xq, small, 2, moe_cfg)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{Q} pairs, cfg {_tag(rb_cfg)}"


# ---- exact weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_exact_walk_at_1024_pairs_recovers_every_experts_weights(coracle, gpu, dt):
    """E = 4 weights of 128 x 256 (sensitive nested, blocksize2 16; drawn single) and P = 1024:
    every (expert, k) exactly once in ONE launch.  x_div 1: a drawn permutation of the (e, k) with
    x[p] = eye[k_p]; x_div 4: x = eye(256) and each token's four ids a drawn permutation of
    0 .. 3.  y[p] is W_{e_p}[:, k_p] plus exact zeros and must equal the oracle's 16-bit weight by
    value, with no tolerance -- a slice that sums an exact value and exact zeros stays exact, so
    also under two K slices.  Each expert holds 256 rows: two full row blocks, and row blocks 2 .. 7
    of every expert return without a row.  A swapped expert, row block, list entry, column or k
    shows, and so does a fused multiply-add in the scale."""
    E, N, P = 4, 128, 1024
    tdt = MOE._tdt(dt)
    rng = np.random.default_rng(1024)
    eye = torch.eye(K, dtype=tdt, device=gpu)
    perm = rng.permutation(P)
    forms = [(1, perm // K, perm % K), (4, np.concatenate([rng.permutation(E) for _ in range(K)]), np.arange(P) // 4)]
    for x_div, ids, ks in forms:
        assert sorted(zip(ids.tolist(), ks.tolist())) == [(e, k) for e in range(E) for k in range(K)]
    edge = [int(np.nonzero(forms[0][1] == e)[0][127]) % 64 for e in range(E)]
    assert any(lane != 63 for lane in edge), "no block edge inside a ballot round"
    for S in (MOE._stack(coracle, gpu, "nested", "sensitive", E, N, K, dt), MOE._stack(coracle, gpu, "single", "drawn", E, N, K, dt)):
        want = torch.stack([torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).to(gpu).view(tdt) for b in S.bits])  # [E, N, K]
        for x_div, ids, ks in forms:
            kt = torch.from_numpy(ks).to(gpu)
            x = (eye[kt] if x_div == 1 else eye).contiguous()
            expect = want[torch.from_numpy(ids).to(gpu), :, kt]                                                           # [P, N]
            for cfg in (None, _cfg(2, 1), _cfg(2, 2), _cfg(4, 2)):
                ok = _rb(S, x, ids, x_div, cfg) == expect
                assert bool(ok.all()), (f"{S.mode} {dt} x_div {x_div} cfg {_tag(cfg)}: {int((~ok).sum())} of {ok.numel()} weights "
                                        f"differ, first at (pair, n) {(~ok).nonzero()[0].tolist()}")


# ---- reproducible and re-entrant -------------------------------------------------------------------
def test_same_call_twice_on_one_workspace_gives_the_same_bits(coracle, gpu):
    """300 pairs, two K slices: twice on one workspace with another routing (two experts idle,
    invalid ids) in between: identical bits, the second routing right, the workspace all zero
    after each call, nf4_gemm_check_workspace clean."""
    _lib, L = MOE._lib_and_L()
    E, N, P = 4, 128, 300
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, N, K, "bf16")
    cfg = _cfg(4, 2)
    d = S.desc()
    need = L.nf4_gemm_bnb_moe_rb_workspace_bytes(P, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), ctypes.byref(cfg))
    assert need == 64 * 1024 + 256 + 2 * P * N * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    sp = torch.cuda.current_stream().cuda_stream
    xd, xb = _x(P, 2, "bf16", gpu)
    a = _drawn(P, E, seed=3)
    b = np.array([1, 3, -1, 3, E])[np.arange(P) % 5]
    ys = []
    for ids in (a, b, a):
        ys.append(_rb(S, xd, ids, 2, cfg, ws=ws))
        assert int(ws.count_nonzero()) == 0, "tickets or slab entries left set"
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), sp) == 0
    MOE._check(S, ys[0], xb, a, 2, "first call")
    MOE._check(S, ys[1], xb, b, 2, "other routing")
    assert torch.equal(ys[0].view(torch.int16), ys[2].view(torch.int16))


# ---- many experts ----------------------------------------------------------------------------------
def test_256_experts_at_1024_pairs(coracle, gpu):
    """E = 256, N = 64, 1024 drawn pairs: every expert gets a few rows, so of each expert's eight
    row blocks at most one works and the others return at once; one expert is left idle."""
    E, N, P = 256, 64, 1024
    S = MOE._stack(coracle, gpu, "nested", "drawn", E, N, K, "bf16")
    ids = _drawn(P, E, seed=256, idle=(77,))
    counts = np.bincount(ids, minlength=E)
    assert counts[77] == 0 and (counts > 0).sum() > 200 and counts.max() <= 128
    xd, xb = _x(P, 8, "bf16", gpu)
    for cfg in (None, _cfg(2, 2)):
        MOE._check(S, _rb(S, xd, ids, 8, cfg), xb, ids, 8, f"256 experts cfg {_tag(cfg)}")
    # the bounds: one pair more is the caller's error, and so is nf4_gemm_bnb_moe's own cfg
    _lib, L = MOE._lib_and_L()
    y = torch.empty((P, N), dtype=torch.bfloat16, device=gpu)
    idt = torch.zeros(P + 1, dtype=torch.int32, device=gpu)
    _call(S, xd.data_ptr(), idt[:P], P, 8, y.data_ptr(), _cfg(2, 1, MOE.MOE), expect=_lib.ERR_ARG)
    rc = L.nf4_gemm_bnb_moe_rb(xd.data_ptr(), idt.data_ptr(), P + 1, 8, ctypes.cast(ctypes.pointer(S.desc()), ctypes.c_void_p),
                               y.data_ptr(), _lib.BF16, None, 0, None, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_SHAPE
