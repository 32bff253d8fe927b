"""tests/_activation_cases.py checked on the host (no GPU): ``judge`` and ``isolated`` accept an
honest fp32 emulation of a fused GEMM -- numpy float32 products accumulated in float32, in one
pass and in 2 and 3 K slices summed in slice order, rounded to nearest even to 16 bits with
overflow to infinity -- and reject each mutant of it; every activation matrix the GPU tests build
passes the builder's own assertions and keeps its borderline share within the cap."""
import numpy as np
import pytest

import _activation_cases as A
from _gemm_cases import bits_to_f64, cfg_tuple, gemm_cfgs


def _f32(bits, dt):
    bits = np.asarray(bits, np.uint16)
    if dt == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _round16(v32, dt, clamp=False):
    """fp32 -> 16 bits, ties to even, overflow to infinity (``clamp``: to the format's max)."""
    v32 = np.asarray(v32, np.float32)
    if dt == "f16":
        with np.errstate(over="ignore"):
            out = v32.astype(np.float16).view(np.uint16)
    else:
        b = v32.view(np.uint32)
        out = ((b + (((b >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)
        out = np.where(np.isnan(v32), np.uint16(0x7FC0), out)
    if clamp:
        inf = 0x7C00 if dt == "f16" else 0x7F80
        was_inf = np.isinf(v32)
        out = np.where(((out & 0x7FFF) == inf) & ~was_inf, (out & 0x8000) | (inf - 1), out).astype(np.uint16)
    return out


def emulate(x_bits, w_bits, dt, slices=1, flush_x=False, nan_as_zero=False, clamp=False, inf_times_zero_is_zero=False):
    x, w = _f32(x_bits, dt).copy(), _f32(w_bits, dt)
    if flush_x:
        x[np.abs(x) < (2.0 ** -14 if dt == "f16" else 2.0 ** -126)] = 0
    if nan_as_zero:
        x[np.isnan(x)] = 0
    M, K = x.shape
    edges = [K * i // slices // 128 * 128 for i in range(slices)] + [K]
    y = np.empty((M, w.shape[0]), np.uint16)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(M):
            p = x[m][None, :] * w                               # fp32 products
            if inf_times_zero_is_zero:
                p[:, np.isinf(x[m])] = np.where(w[:, np.isinf(x[m])] == 0, np.float32(0), p[:, np.isinf(x[m])])
            acc = np.zeros(w.shape[0], np.float32)
            for a, b in zip(edges[:-1], edges[1:]):
                acc = (acc + p[:, a:b].sum(axis=1, dtype=np.float32)).astype(np.float32)
            y[m] = _round16(acc, dt, clamp)
    return y


@pytest.fixture(scope="module")
def weights(coracle):
    N, K = A.GEMM_N, 1024
    return {dt: A.bits_of(coracle, A.decode_weight("nested", N, K), N, K, dt) for dt in ("bf16", "f16")}


def _cases(dt, w, Ms=(1, 8, 32)):
    """(x, base, rows) for every kind set of both groups at each M."""
    for M in Ms:
        for which in ("finite", "nonfinite"):
            for kinds in A.kind_sets(M, dt, which):
                yield A.special_x(M, 1024, dt, A.x_seed(M, 1024), kinds, w)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("slices", [1, 2, 3])
def test_judge_accepts_an_honest_fp32_emulation(weights, dt, slices):
    w = weights[dt]
    seen = set()
    for x, base, rows in _cases(dt, w):
        y = emulate(x, w, dt, slices)
        A.judge(y, x, w, dt, f"{dt} {slices} slices {rows}", rows=rows)
        A.isolated(y, emulate(base, w, dt, slices), rows, f"{dt} {slices} slices {rows}")
        seen |= set(rows.values())
        yf = bits_to_f64(y, dt)
        for r, kind in rows.items():  # the rows do what their names say
            if kind == "nan":
                assert np.isnan(yf[r]).all()
            if kind in ("pinf", "ninf"):
                assert np.isnan(yf[r]).any() and np.isinf(yf[r]).any() and not np.isfinite(yf[r]).any()
            if kind == "huge" and dt == "f16":
                assert np.isinf(yf[r]).mean() >= 0.25 and np.isfinite(yf[r]).mean() >= 0.25
            if kind in ("tiny", "small"):
                assert (yf[r] != 0).mean() > 0.9
    assert seen == set(A.FINITE[dt]) | set(A.NONFINITE)


def _row_of(rows, kind):
    return next(r for r, k in rows.items() if k == kind)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 32])
def test_judge_rejects_every_mutant(weights, dt, M):
    w = weights[dt]
    fin = {k: c for c in _cases(dt, w, (M,)) for k in c[2].values()}   # kind -> the case that holds it

    def rejected(y, case, what, by_isolated=None):
        x, base, rows = case
        with pytest.raises(AssertionError):
            A.judge(y, x, w, dt, what, rows=rows)
        if by_isolated is not None:
            with pytest.raises(AssertionError):
                A.isolated(y, by_isolated, rows, what)

    if dt == "f16":
        x, base, rows = fin["tiny"]
        rejected(emulate(x, w, dt, flush_x=True), fin["tiny"], "subnormal x flushed to zero")
        x, base, rows = fin["huge"]
        y = emulate(x, w, dt, clamp=True)
        assert (y[_row_of(rows, "huge")] & 0x7FFF == 0x7BFF).any()
        rejected(y, fin["huge"], "overflow clamped to the format's max")
    x, base, rows = fin["nan"]
    rejected(emulate(x, w, dt, nan_as_zero=True), fin["nan"], "a NaN row computed as if the NaN were 0")
    if M > 1:
        r = _row_of(rows, "nan")
        y, yb = emulate(x, w, dt), emulate(base, w, dt)
        n = r - 1 if r > 0 and r - 1 not in rows else next(m for m in range(M) if m not in rows)
        y[n, 5] = 0x7FC0 if dt == "bf16" else 0x7E00
        rejected(y, fin["nan"], "a NaN copied into a neighbouring row", by_isolated=yb)
        y = emulate(x, w, dt)
        y[n, 5] ^= 1                                           # one ulp in a plain row: not isolated
        with pytest.raises(AssertionError):
            A.isolated(y, yb, rows)
    for kind in ("zero", "negzero"):
        x, base, rows = fin[kind]
        y = emulate(x, w, dt)
        assert (y[_row_of(rows, kind)] & 0x7FFF == 0).all()
        y[_row_of(rows, kind), 3] = 0x0001                      # the smallest subnormal
        rejected(y, fin[kind], f"a {kind} row returning a small non-zero value")
    for kind in ("pinf", "ninf"):
        x, base, rows = fin[kind]
        y = emulate(x, w, dt, inf_times_zero_is_zero=True)
        assert not np.isnan(bits_to_f64(y[_row_of(rows, kind)], dt)).any()
        rejected(y, fin[kind], "an infinity times a zero weight giving 0")
        y = emulate(x, w, dt)
        r = _row_of(rows, kind)
        y[r] = np.where((y[r] & 0x7FFF) == (0x7C00 if dt == "f16" else 0x7F80), y[r] ^ 0x8000, y[r])
        rejected(y, fin[kind], "the other infinity")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_gpu_case_builds_and_keeps_its_borderline_share(coracle, dt):
    """special_x's own assertions (a column with zero and non-zero weights in every weight, a
    subnormal majority in the tiny row, the fp16 power of two of the huge row, no fp32 overflow in
    bf16) at every (M, K, weights) of the GPU tests, and the reference's borderline share."""
    import torch

    from test_gpu_gemm_moe import _Stack

    cases = list(A.host_cases(coracle, dt))
    S = _Stack(coracle, torch.device("cpu"), "nested", "sensitive", A.MOE["E"], A.MOE["N"], A.MOE["K"], dt)
    cases.append(("moe", -(-A.MOE["P"] // A.MOE["x_div"]), A.MOE["K"], S.bits))
    shares, huge = [], []
    for label, M, K, ws in cases:
        for which in ("finite", "nonfinite"):
            for kinds in A.kind_sets(M, dt, which):
                x, base, rows = A.special_x(M, K, dt, A.x_seed(M, K), kinds, ws)
                assert (x != base).any(axis=1).sum() == len(rows) == len(kinds)
                assert sorted(rows) == sorted(A.positions(M, len(kinds)))
                for w in ws:
                    s = A.borderline_share(x, w, dt)
                    assert s <= A.BORDERLINE_CAP, (label, M, K, kinds, s)
                    shares.append(s)
                    if "huge" in kinds and dt == "f16":
                        huge.append(s)
                    assert A.borderline_share(base, w, dt) == 0.0
    print(f"borderline share {dt}: max {max(shares):.4%}, mean over fp16 huge cases "
          f"{(np.mean(huge) if huge else 0.0):.4%}, {len(shares)} (case, weight) pairs")
    if dt == "bf16":
        assert max(shares) == 0.0
    for M in A.GEMM_MS:  # the explicit decompositions are members of the shared list
        for K, cfg in A.decode_cfgs(M, True):
            assert cfg is None or cfg in {cfg_tuple(c) for c in gemm_cfgs(K, M)}, (M, K, cfg)
    assert A.positions(32, 4) == [0, 31, 15, 16] and A.positions(17, 3) == [0, 16, 15] and A.positions(8, 4) == [0, 7, 1, 6]


def test_the_row_block_routing_is_what_it_says():
    """moe_rb_routing: the special tokens sit on entries 127 / 128 and on the last entry of expert
    1's ascending pair list, on pair 0 and on pair P - 1; the block edge lies inside a ballot round;
    one special token owns an invalid id; every expert's subset holds at least 20 rows per pair of
    any one special token (the condition under which the borderline cap cannot be exceeded)."""
    E, P, x_div = A.MOE["E"], A.MOE_RB["P"], A.MOE_RB["x_div"]
    ids, tokens = A.moe_rb_routing()
    assert ids.shape == (P,) and P == 300 and x_div == 2 and len(set(tokens)) == len(tokens) == 4
    tok = np.arange(P) // x_div
    valid = (ids >= 0) & (ids < E)
    assert set(ids[~valid].tolist()) == {-1, E}
    mine = np.nonzero(ids == 1)[0]                             # expert 1's ascending list
    assert mine.size >= 140 and 128 < mine.size < 256 and mine.size % 16, "two row blocks, the last row tile partly filled"
    assert [int(tok[mine[127]]), int(tok[mine[128]]), int(tok[mine[-1]]), int(tok[0])] == tokens
    assert tok[mine[127]] != tok[mine[128]] and mine[-1] == P - 1 and tok[P - 1] in tokens
    assert mine[127] % 64 != 63 and mine[127] // 64 == mine[128] // 64, "the block edge in the middle of a ballot round"
    assert any(not valid[p] for p in range(P) if tok[p] in tokens), "no invalid id on a special token"
    assert any(not valid[p] for p in range(P) if tok[p] not in tokens), "no invalid id on a plain token"
    counts = np.bincount(ids[valid], minlength=E)
    assert (counts > 0).all()
    for e in range(E):
        for t in tokens:  # whichever special token is the huge one
            assert counts[e] >= 20 * max(1, int(((ids == e) & (tok == t)).sum())), (e, t, counts)
    kinds4, kinds3 = A.FINITE["f16"], A.NONFINITE
    assert A.moe_rb_passes(kinds4, tokens) == [tokens]
    assert {t for at in A.moe_rb_passes(kinds3, tokens) for t in at[:3]} == set(tokens)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_the_row_block_case_builds_and_keeps_its_borderline_share(coracle, dt):
    """The reference alone, per expert subset as test_gpu_gemm_moe_rb_activations.py judges it:
    special_x's own assertions hold on the named rows and the borderline share stays under the cap."""
    import torch

    from test_gpu_gemm_moe import _Stack

    E, N, K, P, x_div = A.MOE["E"], A.MOE["N"], A.MOE["K"], A.MOE_RB["P"], A.MOE_RB["x_div"]
    S = _Stack(coracle, torch.device("cpu"), "nested", "sensitive", E, N, K, dt)
    ids, tokens = A.moe_rb_routing()
    T = P // x_div
    tok = np.arange(P) // x_div
    shares = []
    for which in ("finite", "nonfinite"):
        for kinds in A.kind_sets(T, dt, which):
            for at in A.moe_rb_passes(kinds, tokens):
                x, base, rows = A.special_x(T, K, dt, A.x_seed(T, K), kinds, S.bits, at=at)
                assert list(rows) == at[:len(kinds)] and (x != base).any(axis=1).sum() == len(kinds)
                for e in range(E):
                    sel = np.nonzero(ids == e)[0]
                    s = A.borderline_share(x[tok[sel]], S.bits[e], dt)
                    assert s <= A.BORDERLINE_CAP, (dt, kinds, e, s)
                    shares.append(s)
                    assert A.borderline_share(base[tok[sel]], S.bits[e], dt) == 0.0
    print(f"row-block case {dt}: borderline share at most {max(shares):.4%} over {len(shares)} (pass, expert) subsets")
    if dt == "bf16":
        assert max(shares) == 0.0
