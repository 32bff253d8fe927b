"""The drawn grouped calls of nf4_lora_add (_lora_draws.py) are what they claim: deterministic (a
digest per dtype is pinned here, so a change of the generator shows in review), covering (every
item of the list below on the generated cases), legal by the rules of include/nf4_dequant.h --
restated here from the header's text, not imported from the plan -- and small.  CPU only;
test_gpu_lora_drawn.py runs the same draw on the device."""
import numpy as np
import pytest

import _lora_draws as D
from _family_draws import EDGES

SEED = D.TEST_SEED
OTHER_SEEDS = (1, 2, 77)

DIGESTS = {
    "bf16": "5fdc2bd71cfe6a4ce9091e73937651d407f08f8809835c245c14e287edb62e5b",
    "f16": "73586ae96981e32142e3034f2244d91d8d8b922d0add7d4eba67da1fed7f4b6a",
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
        assert cases == again[dt] and len(cases) == D.DEFAULT_CASES >= 60
        assert [c.index for c in cases] == list(range(len(cases)))
        a, b = D.inputs(cases[5]), D.inputs(again[dt][5])
        assert np.array_equal(a[0], b[0]) and all(np.array_equal(p, q) for p, q in zip(a[1] + a[2], b[1] + b[2]))
        got[dt] = D.digest(cases)
    assert got == DIGESTS, "the generator changed: review the draw, then pin\n" + "\n".join(f'    "{k}": "{v}",' for k, v in got.items())
    assert D.digest(D.draws("bf16", SEED + 1)) != got["bf16"]


# ---- coverage -----------------------------------------------------------------------------------------
def _wave_ranges(K, waves):
    """Chunks per wave: "the K / 32 chunks split into one contiguous range per wave"."""
    chunks = K // 32
    per = -(-chunks // waves)
    return [max(0, min(chunks, (w + 1) * per) - min(chunks, w * per)) for w in range(waves)]


def _covers(cases):
    """Every item of the coverage list, or an AssertionError naming it."""
    assert any(len(c.adapters) == 8 for c in cases), "a group of 8"
    assert {len(c.adapters) for c in cases} >= {1, 2, 3, 8}, "single calls and small groups"
    assert {a.r for c in cases for a in c.adapters} == set(range(8, 129, 8)), "every r"
    for big, small in ((128, 8), (72, 16)):
        for low in (True, False):
            assert any((c.M <= 16) == low and {big, small} <= {a.r for a in c.adapters} and max(a.r for a in c.adapters) == big
                       for c in cases), f"r = {big} beside r = {small} at M {'<=' if low else '>'} 16"
    assert {c.rt() for c in cases} == {1, 2, 4, 8}, "every r-tile instantiation"
    named = [c for c in cases if c.cfg is not None]
    assert any(c.K == 32 and c.cfg[1] == 4 for c in named), "K = 32 with four waves"
    assert any(c.K == 1056 and c.cfg[1] == 1 and c.rt() == 8 for c in named), "K = 1056 with one wave and RT = 8"
    assert any(c.cfg[0] == 256 and any(a.N == 16 for a in c.adapters) for c in named), "N = 16 under tile_n = 256"
    assert any(a.share is not None for c in cases for a in c.adapters), "two adapters that read the same A and B"
    assert {c.cfg for c in named} == set(D.PAIRS), "every (tile_n, waves)"
    assert 5 * sum(c.cfg is None for c in cases) >= len(cases), "the library's choice in a fifth of the cases"
    assert {c.K for c in cases} == set(D.K_POOL) and {a.N for c in cases for a in c.adapters} == set(D.N_POOL), "every K and N"
    assert {a.mode for c in cases for a in c.adapters} == set(D.MODES), "every base mode"
    assert {a.scale for c in cases for a in c.adapters} == set(D.SCALES), "every scale"
    assert any(c.M <= 16 for c in cases) and any(16 < c.M <= 32 for c in cases) and any(c.M > 96 for c in cases), "one and two row tiles, several row blocks"
    # the load step: kU = 2 chunks at RT = 8, else 4; ranges longer than a step with every tail length, and empty ranges
    tails = {2: set(), 4: set()}
    empty = False
    for c in named:
        ku = 2 if c.rt() == 8 else 4
        for n in _wave_ranges(c.K, c.cfg[1]):
            empty |= n == 0
            if n > ku:
                tails[ku].add(n % ku)
    assert empty and tails[2] == {0, 1} and tails[4] == {0, 1, 2, 3}, ("wave ranges", empty, tails)


def test_coverage_of_the_seed_the_gpu_test_runs(drawn):
    for dt in D.DTYPES:
        _covers(drawn[dt])


@pytest.mark.parametrize("seed", OTHER_SEEDS)
def test_coverage_holds_for_other_seeds_and_for_the_smallest_draw(seed):
    """The MUST list carries the coverage, not the luck of one seed: the tool's seeds cover too."""
    for cases in _all(seed, D.MIN_CASES).values():
        _covers(cases)


# ---- legality: the header's rules, restated ----------------------------------------------------------------
def _legal(c):
    assert c.dt in ("bf16", "f16")
    assert 1 <= c.M <= 128 and c.M in EDGES                      # NF4DQ_LORA_MAX_M
    assert c.K >= 32 and c.K % 32 == 0 and c.K <= 2 ** 22
    assert 1 <= len(c.adapters) <= 8                             # NF4DQ_LORA_GROUP_MAX
    if c.cfg is not None:
        assert c.cfg[0] in (16, 32, 64, 128, 256) and c.cfg[1] in (1, 2, 4)
    for i, a in enumerate(c.adapters):
        assert a.N >= 16 and a.N % 16 == 0 and a.N <= 2 ** 22
        assert 8 <= a.r <= 128 and a.r % 8 == 0                  # NF4DQ_LORA_MAX_R
        assert a.mode in D.MODES and np.isfinite(a.scale) and float(np.float32(a.scale)) == a.scale
        if a.share is not None:
            s = c.adapters[a.share]
            assert 0 <= a.share < i and s.share is None and (s.r, s.N) == (a.r, a.N)
    # "every pointer 16-byte aligned" and "two adapters of one call must not share output elements": the
    # runner carves every y from one 16-byte aligned allocation at these element offsets
    offs, total = D.layout(c)
    spans = [(o, o + c.M * a.N) for o, a in zip(offs, c.adapters)]
    assert all(o % 8 == 0 for o, _ in spans) and spans[0][0] == D.BAND and total == spans[-1][1] + D.BAND
    for (_, e0), (b1, _) in zip(spans[:-1], spans[1:]):
        assert b1 - e0 == D.GAP == 64
    x, As, Bs, bases = D.inputs(c)
    assert x.shape == (c.M, c.K) and x.dtype == np.uint16
    for a, A, B, base in zip(c.adapters, As, Bs, bases):
        assert A.shape == (a.r, c.K) and B.shape == (a.N, a.r) and (base is None) == (a.mode == "null")
        assert base is None or base.shape == (c.M, a.N)
        if a.share is not None:
            assert A is As[a.share] and B is Bs[a.share]
    exp = 0x7F80 if c.dt == "bf16" else 0x7C00
    for arr in [x] + As + Bs + [b for b in bases if b is not None]:
        assert ((arr & exp) != exp).all()                          # finite


@pytest.mark.parametrize("seed", (SEED,) + OTHER_SEEDS)
def test_every_case_is_legal_by_the_headers_rules(seed):
    for cases in _all(seed).values():
        for c in cases:
            _legal(c)


def test_inputs_are_of_unit_size_and_small():
    for seed in (SEED,) + OTHER_SEEDS:
        for dt, cases in _all(seed).items():
            assert max(c.input_bytes() for c in cases) <= 4 * 2 ** 20        # one call: 4 MiB
            assert sum(c.input_bytes() for c in cases) <= 48 * 2 ** 20       # one draw: 48 MiB
    c = next(c for c in _all()["f16"] if c.M >= 64 and c.K >= 224)
    x = D.inputs(c)[0].view(np.float16).astype(np.float64)
    assert abs(x.std() - 1.0) < 0.05 and abs(x.mean()) < 0.05
    v = np.array([1.0, 1.00390625, 1.01171875, -2.5, 0.0], np.float32)     # bf16: a tie to even, a tie up
    assert D.to_bits(v, "bf16").tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC020, 0]
