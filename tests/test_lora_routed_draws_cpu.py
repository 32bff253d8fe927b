"""The drawn calls of nf4_lora_add_routed (_lora_routed_draws.py) are what they claim: deterministic (a
digest per dtype is pinned here, so a change of the generator shows in review), covering (every
item of the list below on the generated cases), legal by the rules of include/nf4_dequant.h --
restated here from the header's text, not imported from the plan or the generator -- and small.  CPU
only; test_gpu_lora_routed_drawn.py runs the same draw on the device."""
import numpy as np
import pytest

import _lora_draws as L
import _lora_routed_draws as D
from _family_draws import EDGES

SEED = D.TEST_SEED
OTHER_SEEDS = (1, 77)

DIGESTS = {
    "bf16": "9c2e2e5c5ffb80f5101d4f48669718df82423bfa74681960e0ac3f908dccde42",
    "f16": "c0c4c37805fa78aa493301c771ad51ae4636ad483ed99afdca9114d081eedc22",
}


def _all(seed=SEED, cases=D.DEFAULT_CASES):
    return {dt: D.draws(dt, seed, cases) for dt in D.DTYPES}


@pytest.fixture(scope="module")
def drawn():
    return _all()


def test_two_draws_with_one_seed_are_equal_and_the_digest_is_pinned(drawn):
    again = _all()
    got = {}
    for dt, cases in drawn.items():
        assert cases == again[dt] and len(cases) == D.DEFAULT_CASES == 48 and D.MIN_CASES == 44
        assert [c.index for c in cases] == list(range(len(cases)))
        assert all(np.array_equal(D.ids(p), D.ids(q)) for p, q in zip(cases, again[dt]))
        got[dt] = D.digest(cases)
    assert got == DIGESTS, "the generator changed: review the draw, then pin\n" + "\n".join(f'    "{k}": "{v}",' for k, v in got.items())
    assert D.digest(D.draws("bf16", SEED + 1)) != got["bf16"]


# ---- coverage: the MUST list -----------------------------------------------------------------------------
def _group_rows(c):
    """adapter -> ascending rows, from the ids alone."""
    out = {}
    for m, a in enumerate(D.ids(c).tolist()):
        if 0 <= a < c.S:
            out.setdefault(a, []).append(m)
    return out


def _covers(cases):
    """Every item of the MUST list, or an AssertionError naming it."""
    rows = {c.index: _group_rows(c) for c in cases}
    at128 = [c for c in cases if c.M == 128]
    for n in D.SIZES:
        assert any(len(g) >= 2 and n in [len(v) for v in g.values()] for g in (rows[c.index] for c in at128)), \
            f"a group of {n} rows beside other adapters within M = 128"
    groups128 = [v for c in at128 if len(rows[c.index]) >= 2 for v in rows[c.index].values()]
    assert any(v[0] >= 64 for v in groups128), "a group entirely in rows 64 .. 127"
    assert any(v[-1] < 64 for v in groups128), "a group entirely in rows 0 .. 63"
    assert any(len(v) > 64 and v[:64] == list(range(64)) for v in groups128), "a group of rows 0 .. 63 and more from 64 on"
    assert any(len(v) == 65 and v[:64] == list(range(64)) for v in groups128), "64 rows in the first mask plus one in the second"
    assert any(c.M > 64 and any(v[0] < 64 <= v[-1] for v in rows[c.index].values()) for c in cases), "a group that straddles row 64"
    for pair in ((31, 32), (0, 63)):
        assert any(set(pair) <= set(rows[c.index]) for c in cases), f"adapters {pair} both present"
    assert any(c.M == 64 and len(rows[c.index]) == 64 for c in cases), "M = 64 with 64 distinct adapters"
    assert any(c.M == 1 and c.S == 64 and len(rows[c.index]) == 1 for c in cases), "M = 1 at S = 64"
    assert any(len(c.stacks) == 8 and {8, 128} <= {s.r for s in c.stacks} for c in cases), "8 stacks with r = 8 and r = 128"
    assert any(72 <= max(s.r for s in c.stacks) <= 96 and len({s.r for s in c.stacks}) >= 2 for c in cases), \
        "a largest r in 72 .. 96 (t rows narrower than the accumulators' columns) over a smaller one"
    stacks = [(c, s) for c in cases for s in c.stacks]
    assert {s.a_pad for _, s in stacks} >= {0, 8, 24} and any(s.a_pad == s.r * c.K for c, s in stacks), "every a_pad"
    assert {s.b_pad for _, s in stacks} == {0, 8, 4096}, "every b_pad"
    assert {s.mode for _, s in stacks} == set(L.MODES), "every base mode"
    assert {c.cfg for c in cases} == set(L.PAIRS) | {None}, "every (tile_n, waves) and the library's choice"
    assert any(c.scales[a] == 0.0 for c in cases for a in rows[c.index]), "scale 0 on a present adapter"
    assert any(not rows[c.index] for c in cases), "a call where every row is without an adapter"
    assert any(c.none_rows() == 0 for c in cases), "a call with no row without an adapter"
    assert {c.S for c in cases} == set(D.S_POOL) and {len(c.stacks) for c in cases} >= {1, 2, 8}, "every S; one, two and eight stacks"
    assert {c.rt() for c in cases} == {1, 2, 4, 8}, "every r-tile instantiation"
    bad = {int(v) for c in cases for v in D.ids(c) if not 0 <= v < c.S}
    assert bad >= {-1, D.INT32_MIN, D.INT32_MAX} and any(c.S in D.ids(c) for c in cases), "every id of a row without an adapter"


def test_coverage_of_the_seed_the_gpu_test_runs(drawn):
    for dt in D.DTYPES:
        _covers(drawn[dt])


@pytest.mark.parametrize("seed", OTHER_SEEDS)
def test_coverage_holds_for_other_seeds_and_for_the_smallest_draw(seed):
    """The MUST list carries the coverage, not the luck of one seed: the tool's seeds cover too."""
    for cases in _all(seed, D.MIN_CASES).values():
        assert len(cases) >= D.MIN_CASES
        _covers(cases)


# ---- legality: the header's rules, restated -------------------------------------------------------------
def _legal(c):
    assert c.dt in ("bf16", "f16")
    assert 1 <= c.M <= 128 and c.M in EDGES                      # NF4DQ_LORA_MAX_M
    assert c.K >= 32 and c.K % 32 == 0 and c.K <= 2 ** 22 and c.K in L.K_POOL
    assert 1 <= len(c.stacks) <= 8                               # NF4DQ_LORA_GROUP_MAX
    assert 1 <= c.S <= 64 and c.S in (1, 2, 3, 8, 33, 64)        # NF4DQ_LORA_MAX_ADAPTERS
    if c.cfg is not None:
        assert c.cfg[0] in (16, 32, 64, 128, 256) and c.cfg[1] in (1, 2, 4)
    for s in c.stacks:
        assert s.N >= 16 and s.N % 16 == 0 and s.N <= 2 ** 22 and s.N in L.N_POOL
        assert 8 <= s.r <= 128 and s.r % 8 == 0                  # NF4DQ_LORA_MAX_R
        assert s.mode in L.MODES
        # "a_stride and b_stride multiples of 8 with a_stride >= r * K and b_stride >= N * r", at most 2^40
        a_stride, b_stride = s.r * c.K + s.a_pad, s.N * s.r + s.b_pad
        assert s.a_pad in (0, 8, 24, s.r * c.K) and s.b_pad in (0, 8, 4096)
        assert a_stride % 8 == 0 and b_stride % 8 == 0 and s.r * c.K <= a_stride <= 2 ** 40 and s.N * s.r <= b_stride <= 2 ** 40
    assert len(c.scales) == c.S
    for v in c.scales:
        assert v in L.SCALES and np.isfinite(v) and float(np.float32(v)) == v
    # the routing: group sizes that sum to at most M, distinct adapters, and ids that say the same
    assert all(0 <= a < c.S and n >= 1 for a, n in c.groups) and len({a for a, _ in c.groups}) == len(c.groups)
    assert sum(n for _, n in c.groups) <= c.M and c.place in D.PLACES
    ids = D.ids(c)
    assert ids.shape == (c.M,) and ids.min() >= -2 ** 31 and ids.max() <= 2 ** 31 - 1     # int32 on the device
    assert {a: len(v) for a, v in _group_rows(c).items()} == dict(c.groups)
    assert int(((ids < 0) | (ids >= c.S)).sum()) == c.none_rows() == c.M - sum(n for _, n in c.groups)
    # "every pointer 16-byte aligned" and "two stacks of one call must not share output elements": the
    # runner carves every y from one 16-byte aligned allocation at these element offsets
    offs, total = D.layout(c)
    spans = [(o, o + c.M * s.N) for o, s in zip(offs, c.stacks)]
    assert all(o % 8 == 0 for o, _ in spans) and spans[0][0] == D.BAND == 4096 and total == spans[-1][1] + D.BAND
    for (_, e0), (b1, _) in zip(spans[:-1], spans[1:]):
        assert b1 - e0 == D.GAP == 64


@pytest.mark.parametrize("seed", (SEED,) + OTHER_SEEDS)
def test_every_case_is_legal_by_the_headers_rules(seed):
    for cases in _all(seed).values():
        for c in cases:
            _legal(c)


@pytest.mark.parametrize("seed", (SEED,) + OTHER_SEEDS)
def test_the_inputs_are_small_and_few_rows_lack_an_adapter(seed):
    for cases in _all(seed).values():
        for c in cases:
            if c.S >= 33:
                assert max(s.r for s in c.stacks) <= 32 and c.K <= 352
            n = 2 * c.M * c.K + 4 * c.M + sum(2 * c.S * (s.r * c.K + s.a_pad + s.N * s.r + s.b_pad) + 4 * c.S +
                                              (0 if s.mode == "null" else 2 * c.M * s.N) for s in c.stacks)
            assert c.input_bytes() == n <= 8 * 2 ** 20
        # at most a quarter of all rows are without an adapter: the draw is not mostly copies of the base
        assert 4 * sum(c.none_rows() for c in cases) <= sum(c.M for c in cases)
