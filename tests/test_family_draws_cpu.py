"""The drawn cases of the row-tiled / expert GEMM family (_family_draws.py) are what they claim:
deterministic (a digest per (entry, dtype) is pinned here, so a change of the generator shows in
review), covering (every item of the list below on the generated cases), legal by the rules of
include/nf4_dequant.h -- restated here from the header's text, not imported from the generator --
and small.  CPU only; test_gpu_gemm_family_drawn.py runs the same draw on the device."""
import numpy as np
import pytest

import _family_draws as D

SEED = D.TEST_SEED  # the seed test_gpu_gemm_family_drawn.py runs
OTHER_SEEDS = (1, 2, 77)

DIGESTS = {
    "mt/bf16": "d06109e3057d9addf3e3337e52926a72fa15e9fef883f3fd4a90067c97797b94",
    "mt/f16": "55419a2d7cb086df6cefec761c917160c46cb928c8a5047392ea65505f577e5a",
    "mt_swiglu/bf16": "5e4da64b903ff6351f93eb7fb4bfc3a22587aed5d37b34ca6dfdeda0657975ce",
    "mt_swiglu/f16": "f9f3d33d26cb0fb87cd20c1161fd922b3f526bbd501cafe997baa45aa8206a47",
    "moe/bf16": "d594bad6821fd564d21b7c90ad63eeafdf70dc9f186e250410badfea056b938c",
    "moe/f16": "2788360f55ed1e366aefdaa579a46854d99c9daf86e7bc8ed3216491df11d7bf",
    "moe_swiglu/bf16": "4cb84843a41d19ee603cb275e96ee5ca0fedcb1dbd447eaaa5227571024a4ac8",
    "moe_swiglu/f16": "fc5754e49eb0583ca623f538da0856dfde228bc998857a84aa453ad0d8446a1f",
    "moe_down/bf16": "00e8b5318c239f7e06850a41be0ca43ca1cb75aeb67d5a75522ac7dea8e2b25d",
    "moe_down/f16": "57440ded35448354ea0e4c723a81f2ae1ea67197fde4bfd338ad95c421a4b801",
}


def _all(seed=SEED, cases=D.DEFAULT_CASES):
    return {(e, dt): D.draws(e, dt, seed, cases) for e in D.ENTRIES for dt in D.DTYPES}


@pytest.fixture(scope="module")
def drawn():
    return _all()


# ---- determinism ------------------------------------------------------------------------------------
def test_two_draws_with_one_seed_are_equal_and_the_digest_is_pinned(drawn):
    again = _all()
    got = {}
    for key, cases in drawn.items():
        assert cases == again[key] and len(cases) == D.DEFAULT_CASES
        assert [c.index for c in cases] == list(range(len(cases)))
        for a, b in zip(cases, again[key]):
            if a.routing is not None:
                assert np.array_equal(D.routing_ids(a), D.routing_ids(b))
        got["%s/%s" % key] = D.digest(cases)
    assert got == DIGESTS, "the generator changed: review the draw, then pin\n" + "\n".join(
        f'    "{k}": "{v}",' for k, v in got.items())
    assert D.digest(D.draws("moe", "bf16", SEED + 1)) != got["moe/bf16"]


# ---- coverage -----------------------------------------------------------------------------------------
def _tiles(P):
    t = (P + 15) // 16
    return t + (t & 1)  # "The row-tile count follows from M": ceil(M / 16) rounded up to even


def _covers(entry, cases):
    """Every item of the coverage list, or an AssertionError naming it."""
    moe = entry in D.MOE_ENTRIES
    Ps = {c.P for c in cases}
    assert {32, 64, 96, 128} <= Ps and {_tiles(c.P) for c in cases} == {2, 4, 6, 8}, "row-tile instantiations and their upper edges"
    named = [c for c in cases if c.cfg is not None]
    assert {c.cfg[0] for c in named} == {2, 4}, "both wave counts"
    assert any(c.cfg[1] == 1 for c in named), "ksplit 1, named"
    assert any(c.cfg[1] == c.stack.K // 128 and c.cfg[1] > 1 for c in named), "ksplit = K / 128"
    empty = [c for c in named if (c.cfg[1] - 1) * -(-(c.stack.K // 128) // c.cfg[1]) >= c.stack.K // 128]
    assert empty, "a case whose last K slice is empty"
    assert any(c.stack.K == 1152 and c.cfg[1] == 7 and (not moe or c.stack.E == 17) for c in named), "K = 1152 in seven slices (E = 17)"
    assert any(c.stack.N == 256 and c.cfg[0] == 2 and c.P == 1 for c in named), "two waves on N = 256 with one pair"
    assert 4 * sum(c.cfg is None for c in cases) >= len(cases), "the library's choice in a quarter of the cases"
    assert {c.stack.N for c in cases} == set(D.N_POOL) and {c.stack.K for c in cases} == set(D.K_POOL), "every N and K"
    assert {c.stack.mode for c in cases} == {"nested", "single"}, "both modes"
    for halves in ([c.stack for c in cases], [c.stack.up for c in cases] if entry in D.SWIGLU_ENTRIES else None):
        if halves is None:
            continue
        nested = [s for s in halves if s.mode == "nested"]
        assert {s.bs2 for s in nested} == {16, 64, 256}, "each blocksize2"
        assert {s.code2_stride for s in nested} == {0, 256}, "code2_stride 0 and 256"
        assert {s.offset for s in nested} == {False, True}, "offset NULL and set"
    assert len({c.stack_index for c in cases}) == len(D.pool(entry, cases[0].seed)), "every stack of the pool is used"
    if not moe:
        assert all(c.routing is None and c.x_div == 1 for c in cases)
        return
    assert {c.stack.E for c in cases} == set(D.E_POOL), "every E of the pool"
    assert 10 * sum(c.stack.E >= 64 for c in cases) >= len(cases), "10 % of the cases at E >= 64"
    assert {c.stack.mode for c in cases if c.stack.E >= 64} == {"nested", "single"}, "both modes at E >= 64"
    assert {c.routing for c in cases} == set(D.ROUTINGS), "each routing name"
    assert any(c.routing == "distinct" and c.P == 128 and c.stack.E == 256 for c in cases), "128 pairs on 128 of 256 experts"
    for name in ("last", "invalid_share", "high"):
        assert any(c.routing == name and c.stack.E == 256 for c in cases), f"{name} at E = 256"
    if entry == "moe_down":
        assert {c.topk for c in cases} == set(range(1, 9)), "every topk"
        assert {c.rw_dtype for c in cases} == {"f32", "out"}, "both rw_dtypes"
        assert any(c.topk in (5, 6) and c.x_div == c.topk for c in cases), "topk 5 or 6 with x_div = topk"
        assert {c.x_div == 1 for c in cases if c.topk > 1} == {False, True}, "x_div 1 and topk"
    else:
        assert {2, 3, 5, 7, 8} <= {c.x_div for c in cases} and any(c.P % c.x_div for c in cases), "x_div beyond the divisors of P"
        assert any(c.x_div % 2 and c.x_div > 1 and c.P % 16 == 1 and c.P > 16 for c in cases), "odd x_div against a row-tile edge"


@pytest.mark.parametrize("entry", D.ENTRIES)
def test_coverage_of_the_seed_the_gpu_test_runs(drawn, entry):
    for dt in D.DTYPES:
        _covers(entry, drawn[entry, dt])


@pytest.mark.parametrize("seed", OTHER_SEEDS)
def test_coverage_holds_for_other_seeds_and_for_the_smallest_draw(seed):
    """The MUST list carries the coverage, not the luck of one seed: the tool's seeds cover too."""
    for (entry, dt), cases in _all(seed, D.MIN_CASES).items():
        _covers(entry, cases)


# ---- legality: the header's rules, restated -------------------------------------------------------------
def _legal(c):
    S = c.stack
    moe, swiglu = c.entry in D.MOE_ENTRIES, c.entry in D.SWIGLU_ENTRIES
    assert c.dt in ("bf16", "f16")
    assert 1 <= c.P <= 128                                    # NF4DQ_GEMM_MT_MAX_M, NF4DQ_MOE_MAX_PAIRS
    assert S.N >= 64 and S.N % 64 == 0 and S.K >= 128 and S.K % 128 == 0
    assert 1 <= S.E <= 256                                    # NF4DQ_MOE_MAX_EXPERTS
    assert S.mode in ("nested", "single")
    stacks = [S] + ([S.up] if swiglu else [])
    assert (S.up is not None) == swiglu
    for s in stacks:
        assert (s.mode, s.E, s.N, s.K) == (S.mode, S.E, S.N, S.K)  # the two stacks agree in N, K, experts, single
        assert s.pads[0] % 16 == 0 and min(s.pads) >= 0          # packed_stride % 16 == 0, every stride >= its data
        if s.mode == "nested":
            assert s.bs2 >= 4 and s.bs2 & (s.bs2 - 1) == 0      # a power of two
            assert s.code2_stride == 0 or s.code2_stride >= 256
    assert c.x_div >= 1
    tiles = None
    if c.cfg is not None:
        waves, ksplit = c.cfg
        assert waves in (2, 4)
        cols = (16 if swiglu else 32) * waves                    # "owns 32 * waves columns" / "16 * waves columns of h"
        assert S.N % cols == 0
        assert 1 <= ksplit <= min(S.K // 128, 16)
        tiles = S.N // cols
        tickets = (S.E * tiles if moe else tiles) + (tiles if c.entry == "moe_down" else 0)
        assert tickets * 4 <= 64 * 1024                          # the tickets the workspace header holds
    if moe:
        assert c.routing in D.ROUTINGS
        ids = D.routing_ids(c)
        assert ids.shape == (c.P,) and ids.min() >= -2 ** 31 and ids.max() <= 2 ** 31 - 1
    else:
        assert c.x_div == 1 and 0 <= c.expert < S.E and c.topk == 1
    if c.entry == "moe_down":
        assert 1 <= c.topk <= 8 and c.topk <= c.P and c.P % c.topk == 0
        assert c.x_div in (1, c.topk) and c.rw_dtype in ("f32", "out")
    elif moe:
        assert 1 <= c.x_div <= 8 and c.topk == 1


@pytest.mark.parametrize("seed", (SEED,) + OTHER_SEEDS)
def test_every_case_is_legal_by_the_headers_rules(seed):
    for cases in _all(seed).values():
        for c in cases:
            _legal(c)


def test_the_routings_are_what_their_names_say(drawn):
    for (entry, dt), cases in drawn.items():
        for c in cases:
            if c.routing is None:
                continue
            ids, E, P = D.routing_ids(c), c.stack.E, c.P
            valid = (ids >= 0) & (ids < E)
            group = max(1, min(P, c.topk if entry == "moe_down" else c.x_div))
            bad = {-1, E, E + 1, -2 ** 31, 2 ** 31 - 1}
            assert set(ids[~valid].tolist()) <= bad, c
            if c.routing in ("uniform", "zipf", "last", "first", "high", "twice"):
                assert valid.all(), c
            if c.routing == "zipf" and P >= 32:
                assert np.bincount(ids, minlength=E).max() >= P // 2, c
            if c.routing == "last":
                assert (ids == E - 1).all(), c
            if c.routing == "first":
                assert (ids == 0).all(), c
            if c.routing == "distinct":
                v = ids[valid]
                assert v.size == min(P, E) and np.unique(v).size == v.size and (ids[~valid] == -1).all(), c
            if c.routing == "high":
                assert E == 256 and ids.min() >= 128, c
            if c.routing == "invalid_share":
                assert (~valid).any(), c
            if c.routing == "dead_token":
                assert not valid[:group].any(), c
            if c.routing == "twice":
                assert group >= 2 and ids[0] == ids[1], c
    big = [c for c in drawn["moe", "bf16"] if c.routing == "distinct" and c.P == 128 and c.stack.E == 256]
    assert big and np.unique(D.routing_ids(big[0])).size == 128  # 128 experts active, 128 idle
    inv = [c for cs in drawn.values() for c in cs if c.routing == "invalid_share" and c.stack.E == 256]
    assert any((D.routing_ids(c) == 256).any() for c in inv), "the id E itself as an invalid id at E = 256"


# ---- size ---------------------------------------------------------------------------------------------
def test_pools_and_calls_are_small():
    for seed in (SEED,) + OTHER_SEEDS:
        for entry in D.ENTRIES:
            stacks = D.pool(entry, seed)
            assert len(stacks) <= 12
            for s in stacks:
                assert s.N in D.N_POOL and s.K in D.K_POOL and s.E in D.E_POOL
                assert s.E < 64 or (s.N == 64 and s.K <= 384)
                assert s.nbytes() < (16 if s.up else 8) * 2 ** 20  # a stack (gate and up: two) stays under 8 MiB
            assert sum(s.nbytes() for s in stacks) < 64 * 2 ** 20
            for dt in D.DTYPES:
                for c in D.draws(entry, dt, seed):
                    assert c.stack == stacks[c.stack_index]
                    assert (c.P // c.topk) * c.stack.N <= c.P * c.stack.N <= 128 * 256
                    if c.entry == "moe_down":
                        w = D.routing_weights(c)
                        assert w.dtype == np.float32 and ((w.view(np.uint32) & 0xFFFF) != 0).all() and (0 < w).all() and (w < 1).all()
