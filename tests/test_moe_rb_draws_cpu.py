"""The drawn calls of the expert GEMM in row blocks (_moe_rb_draws.py) are what they claim:
deterministic (a digest per dtype is pinned here, so a change of the generator shows in review),
covering (every item of the list below on the generated cases), legal by the rules of
include/nf4_dequant.h -- restated here from the header's text, not imported from the generator --,
routed as their names say, and small.  CPU only; test_gpu_gemm_moe_rb_drawn.py runs the same draw
on the device."""
import numpy as np
import pytest

import _family_draws as F
import _moe_rb_draws as D

SEED = D.TEST_SEED  # the seed test_gpu_gemm_moe_rb_drawn.py runs
OTHER_SEEDS = (1, 2, 77)
HEADER = 64 * 1024 + 256  # the ticket header of a split-K workspace

DIGESTS = {
    "bf16": "d41690ef7c523027ee28cd9aeb068005c354c7e91ba0a693f11b12929ac886b5",
    "f16": "30d5d599cc48dff7e41eb21ed99fc415076b8d721ed07bc1a8f8175cad45ec82",
}


def _all(seed=SEED, cases=D.DEFAULT_CASES):
    return {dt: D.draws(dt, seed, cases) for dt in D.DTYPES}


@pytest.fixture(scope="module")
def drawn():
    return _all()


# ---- determinism ------------------------------------------------------------------------------------
def test_two_draws_with_one_seed_are_equal_and_the_digest_is_pinned(drawn):
    again = _all()
    got = {}
    for dt, cases in drawn.items():
        assert cases == again[dt] and len(cases) == D.DEFAULT_CASES == 48
        assert [c.index for c in cases] == list(range(len(cases)))
        for a, b in zip(cases, again[dt]):
            assert np.array_equal(D.ids(a), D.ids(b))
        got[dt] = D.digest(cases)
    assert got == DIGESTS, "the generator changed: review the draw, then pin\n" + "\n".join(
        f'    "{k}": "{v}",' for k, v in got.items())
    assert D.digest(D.draws("bf16", SEED + 1)) != got["bf16"]
    assert SEED != F.TEST_SEED and D.MIN_CASES <= 44


# ---- coverage -----------------------------------------------------------------------------------------
def _counts(c):
    ids = D.ids(c)
    valid = (ids >= 0) & (ids < c.stack.E)
    return ids, valid, np.bincount(ids[valid], minlength=c.stack.E)


def _empty_last_slice(c):
    chunks = c.stack.K // 128
    return c.cfg is not None and (c.cfg[1] - 1) * -(-chunks // c.cfg[1]) >= chunks


def _covers(cases):
    """Every item of the MUST list, or an AssertionError naming it."""
    named = [c for c in cases if c.cfg is not None]
    big = [c for c in named if c.P > 128]
    small = [c for c in cases if c.P <= 128]
    assert {1, 17, 128} <= {c.P for c in small} and any(c.cfg is None for c in small if c.P in (1, 17, 128)), "P <= 128 at 1, 17, 128"
    assert {c.cfg[0] for c in named} == {2, 4}, "both wave counts"
    for pick, what in ((named, "at any P"), (big, "at P > 128")):
        assert any(c.cfg[1] == 1 for c in pick), f"ksplit 1, named, {what}"
        assert any(c.cfg[1] == c.stack.K // 128 > 1 for c in pick), f"ksplit = K / 128 > 1, {what}"
        assert any(c.stack.K == 1152 and c.stack.E == 17 and c.cfg == (2, 7) for c in pick), f"(2, 7) on K = 1152 / E = 17, {what}"
        assert any(c.stack.K == 640 and c.cfg[1] == 4 and _empty_last_slice(c) for c in pick), f"four slices on K = 640, {what}"
    top = [c for c in cases if c.P == 1024]
    assert any(c.routing == "one" for c in top), "1024 pairs on one expert"
    assert any(c.routing == "uniform" and c.stack.E == 256 for c in top), "1024 pairs, uniform, E = 256"
    assert any(c.routing == "none_valid" for c in top), "1024 pairs, every id invalid"
    assert any(c.x_div == 8 for c in top), "1024 pairs with x_div 8"
    fb = [c for c in cases if c.routing == "full_blocks"]
    assert any(c.P == 257 for c in fb), "full_blocks at 257 pairs"
    assert any(c.P >= 385 and c.j_min >= 2 and ((_counts(c)[2] >= 256) & (_counts(c)[2] % 128 == 0)).any() for c in fb), "full_blocks, j >= 2"
    bp = [c for c in cases if c.routing == "block_plus_one" and c.tail]
    assert {130, 385} <= {c.P for c in bp}, "block_plus_one at 130 and 385 pairs, the expert's last pair the last pair"
    assert any(c.routing == "sorted" for c in cases), "sorted"
    assert any(c.routing == "late" and c.P % 64 for c in cases), "late at a P that is no multiple of 64"
    assert any(c.routing == "invalid_share" and c.P == 1023 and c.stack.E == 256 for c in cases), "invalid_share, 1023 pairs, E = 256"
    assert any(c.invalid_edges and c.P > 128 for c in cases), "invalid ids forced at the ballot-round edges"
    for name in ("high", "distinct", "last"):
        assert any(c.routing == name and c.stack.E == 256 and c.P > 128 for c in cases), f"{name} at E = 256, P > 128"
    assert {(129, 3), (257, 5), (385, 7)} <= {(c.P, c.x_div) for c in cases}, "odd x_div against a block edge"
    assert any(c.stack.N == 256 and c.cfg[0] == 2 and c.P == 129 for c in named), "two waves on N = 256 with 129 pairs"
    assert 4 * sum(c.cfg is None for c in cases) >= len(cases), "the library's choice in a quarter of the cases"
    assert {c.routing for c in cases} == set(D.ROUTINGS), "each routing name"
    assert any(c.P % c.x_div for c in cases), "x_div beyond the divisors of P"
    assert any(c.cfg[1] > 1 and _counts(c)[2].max() > 128 for c in big), "several K slices with two row blocks of one expert"


def test_coverage_of_the_seed_the_gpu_test_runs(drawn):
    for dt in D.DTYPES:
        _covers(drawn[dt])
        stacks = [c.stack for c in drawn[dt]]
        nested = [s for s in stacks if s.mode == "nested"]
        assert {s.N for s in stacks} == set(F.N_POOL) and {s.K for s in stacks} == set(F.K_POOL) and {s.E for s in stacks} == set(F.E_POOL)
        assert {s.bs2 for s in nested} == {16, 64, 256} and {s.code2_stride for s in nested} == {0, 256}
        assert {s.offset for s in nested} == {False, True} and {s.mode for s in stacks} == {"nested", "single"}
        assert len({c.stack_index for c in drawn[dt]}) == len(F.pool("moe", SEED)), "every stack of the pool is used"


@pytest.mark.parametrize("seed", OTHER_SEEDS)
def test_coverage_holds_for_other_seeds_and_for_the_smallest_draw(seed):
    """The MUST list carries the coverage, not the luck of one seed: the tool's seeds cover too."""
    for cases in _all(seed, D.MIN_CASES).values():
        assert len(cases) == D.MIN_CASES
        _covers(cases)


def test_the_free_cases_spread_as_the_text_says():
    """Over many seeds: about 15 % of the free cases up to 128 pairs, about 60 % of the others on the edge list."""
    free = [c for seed in range(100, 140) for c in D.draws("bf16", seed, 2 * D.MIN_CASES)]
    assert len(free) == 40 * 2 * D.MIN_CASES
    Ps = np.array([c.P for c in free])
    small = (Ps <= 128).mean()
    # (the MUST half pins 3 of 30 cases to P <= 128 and draws 13 more from 129 .. 1024)
    assert 0.08 < small < 0.16, small
    assert {c.x_div for c in free} == set(range(1, 9)) and Ps.min() >= 1 and Ps.max() == 1024
    assert set(D.EDGES) <= set(Ps.tolist())


# ---- legality: the header's rules, restated -------------------------------------------------------------
def _legal(c):
    S = c.stack
    assert c.dt in ("bf16", "f16")
    assert 1 <= c.P <= 1024                                   # NF4DQ_MOE_RB_MAX_PAIRS
    assert S.N >= 64 and S.N % 64 == 0 and S.K >= 128 and S.K % 128 == 0
    assert 1 <= S.E <= 256                                    # NF4DQ_MOE_MAX_EXPERTS
    assert S.mode in ("nested", "single") and S.up is None
    assert S.pads[0] % 16 == 0 and min(S.pads) >= 0           # packed_stride % 16 == 0, every stride >= its data
    if S.mode == "nested":
        assert S.bs2 >= 4 and S.bs2 & (S.bs2 - 1) == 0         # a power of two
        assert S.code2_stride == 0 or S.code2_stride >= 256
    assert c.x_div >= 1
    if c.cfg is not None:
        waves, ksplit = c.cfg
        assert waves in (2, 4)
        assert S.N % (32 * waves) == 0                         # "owns 32 * waves columns"
        assert 1 <= ksplit <= min(S.K // 128, 16)
        tiles, blocks = S.N // (32 * waves), -(-c.P // 128)
        if ksplit > 1:                                         # "experts * column tiles * row blocks" tickets in the header
            assert S.E * tiles * blocks * 4 <= 64 * 1024
            assert HEADER + ksplit * c.P * S.N * 4 < 2 ** 32
    ids = D.ids(c)
    assert ids.shape == (c.P,) and ids.dtype == np.int64 and ids.min() >= -2 ** 31 and ids.max() <= 2 ** 31 - 1


@pytest.mark.parametrize("seed", (SEED,) + OTHER_SEEDS)
def test_every_case_is_legal_by_the_headers_rules(seed):
    for cases in _all(seed).values():
        for c in cases:
            _legal(c)


# ---- the routings are what their names say --------------------------------------------------------------
def _is_block_expert(c, ids, counts, e):
    """Expert e is what full_blocks / block_plus_one promise of one expert."""
    E, P, plus = c.stack.E, c.P, c.routing == "block_plus_one"
    n = int(counts[e])
    j = n // 128
    if n % 128 != plus or not max(1, c.j_min) <= j <= (P - 1) // 128:
        return False
    at = np.nonzero(ids == e)[0]
    if n < P:  # drawn positions: not one run, and every 128th pair of the expert inside a ballot round:
        if at[-1] - at[0] < n or any(at[128 * i - 1] % 64 == 63 for i in range(1, j + 1)):
            return False  # (lanes of the same round follow the block's last row)
    elif not (plus and P % 128 == 1):
        return False
    blocks = -(-P // 128)  # row blocks of the grid
    if plus:   # the expert's last block, j, holds one row
        ok = j < blocks and n - 128 * j == 1
    else:      # row block j is in the grid and gets no row: there `seen == lo`
        ok = j < blocks and n - 128 * j == 0 and n < P
    if c.tail:
        ok = ok and at[-1] == P - 1
    rest = np.delete(ids, at)
    inside = (rest >= 0) & (rest < E)
    return bool(ok and (not inside.any() if E == 1 else inside.all()))


def _check_routing(c):
    ids, valid, counts = _counts(c)
    E, P = c.stack.E, c.P
    bad = {-1, E, E + 1, -2 ** 31, 2 ** 31 - 1}
    assert set(ids[~valid].tolist()) <= bad, c
    if c.invalid_edges:
        at = D.edge_pairs(P)
        assert not valid[at].any() and {63, 64, 64 * ((P - 1) // 64) - 1, P - 1} == set(at), c
        return
    name = c.routing
    if name in ("uniform", "zipf", "last", "first", "high", "twice", "one", "sorted"):
        assert valid.all(), c
    if name == "last":
        assert (ids == E - 1).all(), c
    if name == "first":
        assert (ids == 0).all(), c
    if name == "zipf":
        assert counts.max() >= P // 2, c
    if name == "distinct":
        assert valid.sum() == min(P, E) and counts.max() == 1 and (ids[~valid] == -1).all(), c
    if name == "high":
        assert E == 256 and ids.min() >= 128, c
    if name == "invalid_share":
        assert (~valid).any(), c
    if name == "dead_token":
        assert not valid[:min(P, c.x_div)].any(), c
    if name == "twice":
        assert c.x_div >= 2 and ids[0] == ids[1], c
    if name == "one":
        assert counts.max() == P and (counts > 0).sum() == 1, c
    if name in ("full_blocks", "block_plus_one"):
        assert P >= 129 and any(_is_block_expert(c, ids, counts, e) for e in range(E)), c
    if name == "none_valid":
        assert not valid.any() and set(ids.tolist()) <= bad, c
        if P >= 64:
            assert set(ids.tolist()) == bad, c
    if name == "sorted":
        assert (np.diff(ids) >= 0).all(), c
        if E >= 3:
            assert (counts == 0).any(), c
        live = counts[counts > 0]
        if E >= 2 and P >= 129:
            assert live.size >= 2 and live.max() > live.min(), c    # uneven shares
    if name == "late":
        lo = 64 * ((P - 1) // 64)
        mine = [e for e in range(E) if counts[e] and np.nonzero(ids == e)[0].min() >= lo]
        assert mine, c                                              # an expert whose pairs all lie in the last ballot round
        if E == 1:
            assert not valid[:lo].any(), c


def test_the_routings_are_what_their_names_say(drawn):
    seen = set()
    for seed in (SEED,) + OTHER_SEEDS:
        for cases in (drawn if seed == SEED else _all(seed)).values():
            for c in cases:
                _check_routing(c)
                seen.add(c.routing)
    assert seen == set(D.ROUTINGS) and len(D.ROUTINGS) == 15 and D.ROUTINGS[:9] == F.ROUTINGS
    for c in drawn["bf16"]:
        if c.routing == "invalid_share" and c.stack.E == 256 and c.P == 1023:
            assert (D.ids(c) == 256).any(), "the id E itself as an invalid id at E = 256"
        if c.routing in F.ROUTINGS and not c.invalid_edges:  # the nine old names: _family_draws.routing_ids itself
            f = F.Case("moe", c.dt, c.seed, c.index, c.stack_index, c.stack, c.P, c.x_div, c.cfg, c.routing, c.case_seed)
            assert np.array_equal(D.ids(c), F.routing_ids(f))


# ---- size ---------------------------------------------------------------------------------------------
def test_pool_and_calls_are_small():
    for seed in (SEED,) + OTHER_SEEDS:
        stacks = F.pool("moe", seed)
        assert len(stacks) <= 12 and sum(s.nbytes() for s in stacks) < 64 * 2 ** 20  # the family test's byte bound
        for dt in D.DTYPES:
            need = HEADER
            for c in D.draws(dt, seed):
                assert c.stack == stacks[c.stack_index]
                ks = c.cfg[1] if c.cfg is not None else min(c.stack.K // 128, 16)  # None: whatever the library may choose
                if ks > 1:
                    need = max(need, HEADER + ks * c.P * c.stack.N * 4)
            assert need < 16 * 2 ** 20
