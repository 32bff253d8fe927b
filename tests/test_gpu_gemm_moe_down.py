"""The fused expert down projection with the routed weighted sum (nf4_gemm_bnb_moe_down) through
the C ABI on the GPU (``-m gpu``).

The reference is the EXISTING expert GEMM: ``nf4_gemm_bnb_moe`` with the same (waves, ksplit) on the
same inputs gives the 16-bit products d (it is judged against the float64 oracle in
test_gpu_gemm_moe.py), the documented chain is applied to d on the host in numpy fp32
(_moe_down_cases.chain), and y must equal it BIT FOR BIT -- no tolerance anywhere in this file.

Every call: y is NaN-prefilled between two sentinel bands, the 16-bit scratch of the workspace is
filled with NaN bits BEFORE the call (a stale or unwritten element that is read shows as NaN),
and afterwards the tickets and slabs read 0 and nf4_gemm_check_workspace is clean.  The stacks are
test_gpu_gemm_moe.py's: padded strides, per-expert offsets and code2 tables."""
import ctypes

import numpy as np
import pytest
import torch

from _moe_down_cases import chain, rn16
from test_gpu_gemm_moe import _cfg as _moe_cfg
from test_gpu_gemm_moe import _lib_and_L, _moe, _Stack, _stack, _tdt, _x

pytestmark = pytest.mark.gpu

MOE_DOWN = 12  # NF4DQ_GEMM_MOE_DOWN
E, N = 4, 128  # one column tile at 4 waves, two at 2
HEADER = 64 * 1024 + 256
BAND = 8
# (P, k): row tiles 2 / 4 / 8 of the kernel's instantiations, k from 1 to 8; (96, 2) with every pair
# on one expert is the instantiation for 6
PAIRS = [(2, 2), (16, 2), (34, 2), (128, 2), (12, 1), (12, 3), (32, 4), (128, 8), (96, 2)]


def _cfgs(K):
    """waves {2, 4} x every ksplit in {1, 2, 3} that K admits, and the library's choice (None)."""
    return [None] + [(w, ks) for w in (2, 4) for ks in (1, 2, 3) if ks <= K // 128]


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _routings(P, k, seed):
    """name -> ids[P]."""
    rng = np.random.default_rng(seed)
    p = np.arange(P)
    pats = {"drawn": rng.integers(0, E, P),
            "one expert, three idle": np.full(P, 2),
            "one expert idle": np.array([0, 2, 3])[rng.integers(0, 3, P)],   # never expert 1
            "-1 and E among valid ids": np.array([-1, 0, E, 1, 2, E - 1])[p % 6]}
    if k >= 2:
        same = rng.integers(0, E, P)
        same[1] = same[0]                      # token 0 names one expert twice
        pats["the same expert twice in a token"] = same
    dead = rng.integers(0, E, P)
    dead[:k] = [-1, E, -7, 2 ** 31 - 1, -2 ** 31, E + 1, -1, E][:k]   # token 0: every id invalid
    pats["a token without a valid id"] = dead
    return pats


def _down(S, xd, ids_np, x_div, k, rw, cfg=None, ws=None, fill=True, slabs_zero=True):
    """One call of the entry.  rw: np.float32 values or np.uint16 patterns of the output dtype.
    Returns y's bits [P / k, N].  slabs_zero False: only the header is checked to read 0 afterwards
    (a workspace that an earlier call of another layout left its products in)."""
    _lib, L = _lib_and_L()
    P, T = len(ids_np), len(ids_np) // k
    c = None if cfg is None else _lib.GemmCfg(MOE_DOWN, cfg[0], 1, cfg[1], 2)
    cp = ctypes.byref(c) if c is not None else None
    d = S.desc()
    dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_moe_down_workspace_bytes(P, dp, cp)
    assert wsz >= HEADER + P * S.N * 2, "the workspace is never empty for a valid call"
    scratch_at = wsz - P * S.N * 2
    assert scratch_at % 16 == 0 and (scratch_at - HEADER) % (P * S.N * 4) == 0
    if ws is None:
        ws = torch.zeros(wsz, dtype=torch.uint8, device=S.gpu)
    assert ws.numel() == wsz
    if fill:
        ws[scratch_at:] = 0xFF   # 0xFFFF is a NaN in bf16 and in fp16
    ids = torch.from_numpy(np.asarray(ids_np, np.int32)).to(S.gpu)
    rw = np.ascontiguousarray(rw)
    code = _lib.BF16 if S.dt == "bf16" else _lib.F16
    rwt = torch.from_numpy(rw.view(np.int16) if rw.dtype == np.uint16 else rw).to(S.gpu)
    buf = torch.full((BAND + T + BAND, S.N), 0x5A5B, dtype=torch.int16, device=S.gpu)
    buf[BAND:BAND + T] = torch.full((T, S.N), float("nan"), dtype=_tdt(S.dt), device=S.gpu).view(torch.int16)
    y = buf[BAND:BAND + T]
    sp = torch.cuda.current_stream().cuda_stream
    rc = L.nf4_gemm_bnb_moe_down(xd.data_ptr(), ids.data_ptr(), P, x_div, k, rwt.data_ptr(),
                                 _lib.F32 if rw.dtype == np.float32 else code, dp, y.data_ptr(), code, ws.data_ptr(), wsz,
                                 cp, sp)
    assert rc == 0, (cfg, _lib.strerror(rc))
    assert L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp) == 0
    assert int(ws[:scratch_at if slabs_zero else HEADER].count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg}"
    assert bool((buf[:BAND] == 0x5A5B).all()) and bool((buf[BAND + T:] == 0x5A5B).all()), f"band written, cfg {cfg}"
    return _bits(y)


def _want(S, xd, ids_np, x_div, k, rw, cfg):
    """The host chain over what nf4_gemm_bnb_moe stores under the same (waves, ksplit)."""
    d = _bits(_moe(S, xd, ids_np, x_div, None if cfg is None else _moe_cfg(*cfg)))
    return chain(d, ids_np, S.E, rw, k, S.dt)


def _same(got, want, what):
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                           f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]:#06x} != {want[bad][0]:#06x}")


def _weights(P, seed):
    """fp32 routing weights in (0, 1) with all their mantissa bits: none is a 16-bit value."""
    w = np.random.default_rng(seed).random(P, dtype=np.float32) * np.float32(0.96) + np.float32(0.02)
    assert ((w.view(np.uint32) & 0xFFFF) != 0).all()
    return w


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("P,k", PAIRS)
def test_every_routing_and_cfg_is_the_chain_of_the_expert_gemm(coracle, gpu, dt, K, P, k):
    """Nested statistics, per-pair activations (x_div 1), fp32 routing weights rounded on the device.
    K = 256: ksplit 1 takes no slab, ksplit 2 even slices; K = 384: ksplit 2 uneven slices, ksplit 3."""
    S = _stack(coracle, gpu, "nested", "drawn", E, N, K, dt)
    xd = _x(P, K, dt)[0].to(gpu)
    rw = _weights(P, seed=P + k)
    routings = _routings(P, k, seed=7 * P + k)
    if (P, k) == (96, 2):
        routings = {"one expert, three idle": routings["one expert, three idle"]}
    for name, ids in routings.items():
        for cfg in _cfgs(K):
            got = _down(S, xd, ids, 1, k, rw, cfg)
            _same(got, _want(S, xd, ids, 1, k, rw, cfg), f"{name} P={P} k={k} K={K} {dt} cfg {cfg}")
            if name == "a token without a valid id":
                assert (got[0] == 0).all(), "a token whose ids are all invalid must be a row of +0 bits"


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("P", [16, 48, 80, 128])
@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_instantiation(coracle, gpu, dt, mode, waves, P, ksplit):
    """K = 640 (five chunks: one slice wraps the weight ring, two get 3 + 2), 2 / 4 / 6 / 8 row tiles,
    k = 2, fp32 routing weights.  All pairs go to expert 1 but the last, which goes to expert 0: one
    workgroup runs the instantiation with all its row tiles live, another with one, and two experts
    arrive idle at every tile's ticket."""
    K, k = 640, 2
    S = _stack(coracle, gpu, mode, "drawn", E, N, K, dt)
    ids = np.ones(P, np.int32)
    ids[-1] = 0
    xd = _x(P, K, dt)[0].to(gpu)
    rw = _weights(P, seed=P)
    cfg = (waves, ksplit)
    _same(_down(S, xd, ids, 1, k, rw, cfg), _want(S, xd, ids, 1, k, rw, cfg), f"{dt} {mode} waves={waves} P={P} ksplit={ksplit}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["nested", "single"])
def test_weight_dtypes_special_values_statistics_and_shared_rows(coracle, gpu, dt, mode):
    """16 pairs, k = 2, K = 384; nested and single statistics; weights in fp32 (none representable in
    16 bits: the device rounds) and in the output dtype; x [P, K] and x [P / k, K] (x_div = k).  One
    NaN weight on a pair with an invalid id (0 * NaN is NaN, as in the torch expression), one +Inf
    weight on a valid pair, a token of two invalid ids with weights -0.0 (both products -0: the sum
    from +0 gives +0 bits), a token of two valid ids with weights -0.0."""
    P, k, K = 16, 2, 384
    S = _stack(coracle, gpu, mode, "drawn", E, N, K, dt)
    ids = np.random.default_rng(3).integers(0, E, P)
    ids[2:4] = (-1, E)          # token 1: no valid id, weights -0.0
    ids[6] = E + 2              # token 3: pair 6 invalid with a NaN weight
    rw = _weights(P, seed=5)
    rw[2:4] = -0.0
    rw[6] = np.nan
    rw[9] = np.inf              # token 4, a valid pair
    rw[12:14] = -0.0            # token 6, two valid pairs
    assert 0 <= ids[9] < E and 0 <= ids[12] < E and 0 <= ids[13] < E
    for x_div in (1, k):
        xd = _x(P // x_div, K, dt)[0].to(gpu)
        for weights in (rw, rn16(rw, dt)):
            for cfg in (None, (2, 3), (4, 1)):
                got = _down(S, xd, ids, x_div, k, weights, cfg)
                what = f"{mode} {dt} x_div={x_div} rw {weights.dtype} cfg {cfg}"
                _same(got, _want(S, xd, ids, x_div, k, weights, cfg), what)
                nan = np.isnan(_f32(got, dt))
                assert (got[1] == 0).all(), f"{what}: -0 + -0 from +0 must be +0 bits"
                assert nan[3].all() and not nan[[0, 1, 2, 5, 6, 7]].any(), f"{what}: the NaN weight's token alone is NaN"
                assert np.isinf(_f32(got, dt)[4]).all(), f"{what}: the Inf weight's token"
                assert ((got[6] & 0x7FFF) == 0).all(), f"{what}: products of -0.0 weights are zeros"


def _f32(bits, dt):
    from _moe_down_cases import widen

    return widen(bits, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_two_calls_on_one_workspace_without_a_memset(coracle, gpu, dt):
    """34 pairs, k = 2, K = 384, waves 2 (two column tiles) x three K slices, then the library's
    choice: two routings back to back on ONE workspace, nothing cleared or refilled in between --
    the second result is right only if every ticket of the first call was put back."""
    P, k, K = 34, 2, 384
    S = _stack(coracle, gpu, "nested", "drawn", E, N, K, dt)
    xd = _x(P, K, dt)[0].to(gpu)
    rw = _weights(P, seed=9)
    r = _routings(P, k, seed=11)
    a, b = r["drawn"], r["one expert, three idle"]
    for cfg in ((2, 3), None):
        _lib, L = _lib_and_L()
        d = S.desc()
        c = None if cfg is None else _lib.GemmCfg(MOE_DOWN, cfg[0], 1, cfg[1], 2)
        wsz = L.nf4_gemm_bnb_moe_down_workspace_bytes(P, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p),
                                                      ctypes.byref(c) if c is not None else None)
        ws = torch.zeros(wsz, dtype=torch.uint8, device=gpu)
        first = _down(S, xd, a, 1, k, rw, cfg, ws=ws)
        second = _down(S, xd, b, 1, k, rw, cfg, ws=ws, fill=False)
        third = _down(S, xd, a, 1, k, rw, cfg, ws=ws, fill=False)
        _same(first, _want(S, xd, a, 1, k, rw, cfg), f"first call {dt} cfg {cfg}")
        _same(second, _want(S, xd, b, 1, k, rw, cfg), f"second call on the same workspace {dt} cfg {cfg}")
        _same(third, first, f"the first routing again {dt} cfg {cfg}")


def test_an_earlier_layouts_products_in_a_later_calls_slabs(coracle, gpu):
    """Found by the drawn sequence of test_gpu_gemm_family_drawn.py (seed 20260, moe_down / bf16, cases
    0 and 3) and pinned here by its fields: ONE workspace, nothing cleared in between.
    First 256 single-statistics experts of 64 x 128, 97 pairs, one K slice: the 16-bit products lie
    right behind the header.  Then 17 nested experts of 64 x 1152 (one shared code2 table), 67 pairs,
    2 waves x 8 K slices, ids outside 0..16 among valid ones: slab 0 begins where those products lie.
    Every slab element the reducer reads was stored by a slice of the same call, so the second result
    is the chain bit for bit; afterwards the header and the slab rows of valid pairs read 0, and the
    rows of pairs without a valid id hold what lay there (include/nf4_dequant.h) -- in slab 0, rows
    0 .. 47, the first call's products.  The first layout again, on the same workspace, gives its
    first result."""
    _lib, L = _lib_and_L()
    dt, n = "bf16", 64
    A = _Stack(coracle, gpu, "single", "drawn", 256, n, 128, dt, pads=(704, 2, 2))
    B = _Stack(coracle, gpu, "nested", "drawn", 17, n, 1152, dt, bs2=256, shared_code2=True, pads=(2112, 6, 0))
    (Pa, cfga), (Pb, cfgb) = (97, (2, 1)), (67, (2, 8))

    def need(S, P, cfg):
        d, c = S.desc(), _lib.GemmCfg(MOE_DOWN, cfg[0], 1, cfg[1], 2)
        return L.nf4_gemm_bnb_moe_down_workspace_bytes(P, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), ctypes.byref(c))

    wa, wb = need(A, Pa, cfga), need(B, Pb, cfgb)
    assert wa == HEADER + Pa * n * 2 and wb == HEADER + 8 * Pb * n * 4 + Pb * n * 2
    ws = torch.zeros(max(wa, wb), dtype=torch.uint8, device=gpu)
    ids_a = np.arange(Pa) * 37 % 256                                  # every id valid: every product row is stored
    ids_b = np.array([3, -1, 0, 17, 16, 5, 2 ** 31 - 1, 1, -2 ** 31, 18])[np.arange(Pb) % 10]
    valid = (ids_b >= 0) & (ids_b < 17)
    xa, xb = _x(Pa, 128, dt)[0].to(gpu), _x(Pb, 1152, dt)[0].to(gpu)
    rwa, rwb = _weights(Pa, seed=21), _weights(Pb, seed=22)

    first = _down(A, xa, ids_a, 1, 1, rwa, cfga, ws=ws[:wa])
    _same(first, _want(A, xa, ids_a, 1, 1, rwa, cfga), "first layout")
    slabs = ws[HEADER:wb - Pb * n * 2].view(torch.int32).view(8, Pb, n)   # the second call's slabs
    before = slabs.clone()
    stale = Pa * n * 2 // (n * 4)                                     # rows of slab 0 the products cover: 48 (and half of row 48)
    assert stale == 48 and bool((before[0, :stale] != 0).any(dim=1).all()), "the first call's products are not where slab 0 begins"
    assert int(before[1:].count_nonzero()) == 0

    second = _down(B, xb, ids_b, 1, 1, rwb, cfgb, ws=ws[:wb], fill=False, slabs_zero=False)
    _same(second, _want(B, xb, ids_b, 1, 1, rwb, cfgb), "second layout over the first one's products")
    vt = torch.from_numpy(valid).to(gpu)
    assert int(slabs[:, vt].count_nonzero()) == 0, "slab rows of valid pairs left set"
    assert torch.equal(slabs[:, ~vt], before[:, ~vt]), "slab rows of pairs without a valid id were written"
    assert (~valid[:stale]).sum() == 23 and bool((slabs[0, :stale][~vt[:stale]] != 0).any(dim=1).all()), \
        "no stale products left in the rows of invalid ids: the case no longer has the property it pins"

    third = _down(A, xa, ids_a, 1, 1, rwa, cfga, ws=ws[:wa], fill=False)
    _same(third, first, "the first layout again")


def test_argument_errors_launch_nothing(coracle, gpu):
    """topk 0 and topk not dividing P, a workspace one byte short, a misaligned y, an rw_dtype that is
    neither fp32 nor the output dtype, the expert GEMM's kernel id in the cfg: each its status code,
    with y and the workspace untouched."""
    _lib, L = _lib_and_L()
    P, k, K, dt = 16, 2, 256, "bf16"
    S = _stack(coracle, gpu, "nested", "drawn", E, N, K, dt)
    xd = _x(P, K, dt)[0].to(gpu)
    ids = torch.zeros(P, dtype=torch.int32, device=gpu)
    rw = torch.ones(P, dtype=torch.float32, device=gpu)
    y = torch.full((P // k + 1, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    d = S.desc()
    dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_moe_down_workspace_bytes(P, dp, None)
    assert wsz > 0 and L.nf4_gemm_bnb_moe_down_workspace_bytes(P, dp, ctypes.byref(_lib.GemmCfg(MOE_DOWN, 4, 1, 1, 2))) == \
        HEADER + P * N * 2
    ws = torch.zeros(wsz, dtype=torch.uint8, device=gpu)
    sp = torch.cuda.current_stream().cuda_stream

    def call(topk=k, rw_dtype=_lib.F32, yp=y.data_ptr(), wsb=wsz, cfg=None, pairs=P):
        return L.nf4_gemm_bnb_moe_down(xd.data_ptr(), ids.data_ptr(), pairs, 1, topk, rw.data_ptr(), rw_dtype, dp, yp,
                                       _lib.BF16, ws.data_ptr(), wsb, ctypes.byref(cfg) if cfg is not None else None, sp)

    assert call(topk=0) == _lib.ERR_ARG
    assert call(topk=3) == _lib.ERR_ARG            # 16 % 3 != 0
    assert call(topk=32) == _lib.ERR_ARG           # more than P
    assert call(wsb=wsz - 1) == _lib.ERR_ARG
    assert call(yp=y.data_ptr() + 2) == _lib.ERR_ARG
    assert call(rw_dtype=_lib.F16) == _lib.ERR_ARG  # a 16-bit dtype that is not the output's
    assert call(rw_dtype=5) == _lib.ERR_ARG
    assert call(cfg=_lib.GemmCfg(9, 4, 1, 1, 2)) == _lib.ERR_ARG
    assert call(pairs=0, topk=0) == _lib.OK        # no pairs: nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()) and int(ws.count_nonzero()) == 0, "a rejected call launched"
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y[:P // k].float()).all()) and bool(torch.isnan(y[P // k:].float()).all())
