"""Drawn calls of the expert GEMM in row blocks (nf4_gemm_bnb_moe_rb: 1 .. 1024 pairs in one
launch): pure numpy, no torch, no GPU, in the manner of _lora_routed_draws.py.  The stacks, the
drawing helpers and the nine routings up to 128 pairs are _family_draws.py's, unchanged.

``draws(dt, seed)`` is a deterministic list of ``Case``: a weight stack of ``pool("moe", seed)`` and
one call on it.  test_moe_rb_draws_cpu.py checks that the draw is what this text claims (coverage,
legality, the routing names, size, a pinned digest); test_gpu_gemm_moe_rb_drawn.py runs it on the
device and tools/fuzz_gemm.py --semantics moe_rb runs it with other seeds.

A call: P pairs -- about 15 % of the free cases in 1 .. 128 (``_family_draws._draw_P``), where the
entry must equal nf4_gemm_bnb_moe bit for bit; the rest in 129 .. 1024, 60 % of them from EDGES (the
edges of the 128-row blocks and of the 64-id ballot rounds), the others uniform --, x_div in 1 .. 8
(any value, not only divisors of P), cfg None or (waves, ksplit) legal by include/nf4_dequant.h, and
a routing by name (``ids``): the nine of ``_family_draws.ROUTINGS`` with their meaning, and

    one             every pair on one drawn expert
    full_blocks     a drawn expert gets exactly 128 j pairs, j drawn in max(1, j_min) .. (P - 1) // 128,
                    at drawn, non-contiguous positions; none of its 128th, 256th, ... pairs is the
                    last lane of a ballot round (p % 64 == 63).  The other pairs are spread over the
                    other experts; with E = 1 they have invalid ids.  Row block j of that expert is
                    in the grid and gets no row
    block_plus_one  the same with 128 j + 1 pairs: a last block of one row.  (128 j + 1 = P: every pair
                    is that expert's, and there is nothing to draw.)  ``tail``: the expert's last
                    pair is pair P - 1
    none_valid      every id drawn from the five invalid values -1, E, E + 1, INT_MIN, INT_MAX
    sorted          uneven drawn shares, at least one expert idle when E >= 3, ids ascending
    late            one drawn expert's pairs (at least one) all lie at p >= 64 ((P - 1) // 64), the
                    last ballot round, and no other pair is on that expert (E = 1: invalid ids)

each a function of the case's fields and ``case_seed`` alone.  full_blocks and block_plus_one need
P >= 129.  ``invalid_edges`` forces invalid ids at pairs 63, 64, 64 ((P - 1) // 64) - 1 and P - 1 of
whatever the routing gave: the last lane of a ballot round, the first of the next, the last lane
before the last round and the last pair.

The first cases of a draw are the MUST list -- what the coverage check of test_moe_rb_draws_cpu.py
names -- so a draw of at least MIN_CASES cases covers it whatever the seed; the rest are free.  The
order is shuffled at the end.  Only ``Generator.integers`` and ``Generator.random`` are used.
"""
from __future__ import annotations

import hashlib
from dataclasses import asdict, dataclass, replace
from typing import Optional, Tuple

import numpy as np

import _family_draws as F
from _family_draws import DTYPES, Stack, _pick, _rng, _shuffled, ksplit_max, pool, wave_choices

ROUTINGS = F.ROUTINGS + ("one", "full_blocks", "block_plus_one", "none_valid", "sorted", "late")
EDGES = (129, 130, 191, 192, 193, 255, 256, 257, 319, 320, 321, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024)
MAX_P = 1024                # NF4DQ_MOE_RB_MAX_PAIRS
BLOCK = 128                 # listed rows of one row block (NF4DQ_MOE_MAX_PAIRS)
ROUND = 64                  # ids of one ballot round
DEFAULT_CASES = 48
TEST_SEED = 20263           # the seed the suite runs; the tool takes any other


@dataclass(frozen=True)
class Case:
    dt: str
    seed: int                       # the draw's seed
    index: int                      # position in the draw
    stack_index: int
    stack: Stack
    P: int
    x_div: int
    cfg: Optional[Tuple[int, int]]  # None: the library's choice; (waves, ksplit)
    routing: str
    case_seed: int                  # seeds the ids
    j_min: int = 1                  # full_blocks / block_plus_one: the least j
    tail: bool = False              # block_plus_one: the expert's last pair is pair P - 1
    invalid_edges: bool = False     # invalid ids forced at 63, 64, 64 ((P - 1) // 64) - 1 and P - 1

    def fields(self):
        return asdict(self)


def invalid_values(E):
    return np.array([-1, E, E + 1, -2 ** 31, 2 ** 31 - 1], np.int64)


def edge_pairs(P):
    """Where ``invalid_edges`` puts its invalid ids (those of them P admits)."""
    return sorted({p for p in (ROUND - 1, ROUND, ROUND * ((P - 1) // ROUND) - 1, P - 1) if 0 <= p < P})


# ---- one call --------------------------------------------------------------------------------------
def _draw_P(rng, big=False):
    if not big and rng.random() < 0.15:
        return F._draw_P(rng)
    return int(_pick(rng, EDGES)) if rng.random() < 0.6 else int(rng.integers(BLOCK + 1, MAX_P + 1))


def _routings_for(S, P, x_div):
    return [r for r in ROUTINGS if (r != "high" or S.E > 128) and (r != "twice" or (x_div >= 2 and P >= 2))
            and (r not in ("full_blocks", "block_plus_one") or P > BLOCK)]


def _case(rng, dt, seed, stacks, si, must):
    """One case on stack `si` (or the first stack from `si` on that satisfies must["stack"]), with
    the fields of `must` forced and the rest drawn."""
    want = must.get("stack")
    if want is not None:
        si = next(i % len(stacks) for i in range(si, si + len(stacks)) if want(stacks[i % len(stacks)]))
    S = stacks[si]
    P = must["P"] if "P" in must else _draw_P(rng, must.get("big", False))
    if isinstance(P, tuple):
        P = int(_pick(rng, P))
    x_div = must.get("x_div", int(rng.integers(1, 9)))
    if "cfg" in must:
        cfg = must["cfg"]
        if cfg is not None:
            w, ks = cfg
            w = int(_pick(rng, wave_choices("moe", S.N))) if w is None else w
            ks = int(rng.integers(1, ksplit_max(S.K) + 1)) if ks is None else ksplit_max(S.K) if ks == "max" else ks
            cfg = (w, ks)
    else:
        cfg = (int(_pick(rng, wave_choices("moe", S.N))), int(rng.integers(1, ksplit_max(S.K) + 1)))
    ok = _routings_for(S, P, x_div)
    routing = must.get("routing", _pick(rng, ok))
    assert routing in ok, (routing, S.E, x_div, P)
    return Case(dt, seed, -1, si, S, P, x_div, cfg, routing, int(rng.integers(1, 2 ** 31 - 1)),
                must.get("j_min", 1), must.get("tail", False), must.get("invalid_edges", False))


def _musts():
    """The forced fields of the first cases of every draw.  "stack": a predicate on the Stack;
    "big": P drawn from 129 .. 1024; a tuple P: one of its values, drawn."""
    w4 = lambda s: 4 in wave_choices("moe", s.N)  # noqa: E731
    e256 = lambda s: s.E == 256  # noqa: E731
    deep = lambda s: s.K >= 256  # noqa: E731
    return [
        # up to 128 pairs: nf4_gemm_bnb_moe's bits; both wave counts
        {"P": 1, "cfg": (2, None)}, {"P": 17, "cfg": None}, {"P": 128, "cfg": (4, None), "stack": w4},
        # K-slice forms beyond 128 pairs: one slice named, one slice per chunk, empty last slices
        # (K = 1152: 9 chunks in 7 slices of 2; K = 640: 5 in 4 of 2)
        {"big": True, "cfg": (None, 1)}, {"big": True, "cfg": (None, "max"), "stack": lambda s: s.K >= 384},
        {"big": True, "cfg": (2, 7), "stack": lambda s: s.K == 1152 and s.E == 17},
        {"big": True, "cfg": (None, 4), "stack": lambda s: s.K == 640},
        # eight row blocks
        {"P": MAX_P, "routing": "one"}, {"P": MAX_P, "routing": "uniform", "stack": e256},
        {"P": MAX_P, "routing": "none_valid"}, {"P": MAX_P, "x_div": 8},
        # exactly 128 j pairs and 128 j + 1 pairs on one expert, several K slices among them
        {"P": 257, "routing": "full_blocks", "cfg": (None, "max"), "stack": deep},
        {"P": (385, 511, 512, 513, 767, 768, 769, 1023, 1024), "routing": "full_blocks", "j_min": 2},
        {"P": 130, "routing": "block_plus_one", "tail": True},
        {"P": 385, "routing": "block_plus_one", "tail": True, "cfg": (None, 2), "stack": deep},
        {"big": True, "routing": "sorted"},
        {"P": tuple(p for p in EDGES if p % ROUND), "routing": "late"},
        # invalid ids: E itself at E = 256, the ballot-round edges
        {"P": 1023, "routing": "invalid_share", "stack": e256},
        {"big": True, "routing": "uniform", "invalid_edges": True},
        # many experts beyond 128 pairs
        {"big": True, "routing": "high", "stack": e256}, {"big": True, "routing": "distinct", "stack": e256},
        {"big": True, "routing": "last", "stack": e256},
        # odd x_div against a block edge
        {"P": 129, "x_div": 3}, {"P": 257, "x_div": 5}, {"P": 385, "x_div": 7},
        # two waves on N = 256 with a last block of one pair
        {"P": 129, "cfg": (2, None), "stack": lambda s: s.N == 256},
        # the remaining names of _family_draws.ROUTINGS beyond 128 pairs
        {"big": True, "routing": "zipf"}, {"big": True, "routing": "first", "cfg": None},
        {"big": True, "routing": "dead_token", "x_div": 2}, {"big": True, "routing": "twice", "x_div": 2},
    ]


MIN_CASES = len(_musts())
assert MIN_CASES <= 44


def draws(dt, seed, cases=DEFAULT_CASES):
    """The cases of (dt, seed), in the order they are to run."""
    assert dt in DTYPES and cases >= 1
    stacks = pool("moe", seed)
    rng = _rng("moe_rb calls", dt, seed)
    musts = _musts()
    out = []
    for i in range(cases):
        # two of five cases that force no cfg take the library's choice: more than a quarter of any
        # draw of MIN_CASES or more, whatever the MUST list forces
        must = dict(musts[i]) if i < len(musts) else {}
        if i % 5 in (0, 2):
            must.setdefault("cfg", None)
        out.append(_case(rng, dt, seed, stacks, i % len(stacks), must))
    order = _shuffled(rng, range(len(out)))
    return [replace(out[j], index=i) for i, j in enumerate(order)]


# ---- what a case stands for -------------------------------------------------------------------------
def _subset(rng, n, k):
    """k of range(n), ascending, drawn."""
    return np.sort(np.argsort(rng.random(n), kind="stable")[:k])


def _others(rng, E, e, n):
    """n ids for pairs that must not be on expert e: the other experts, or invalid ids when E = 1."""
    if E == 1:
        bad = invalid_values(E)
        return bad[rng.integers(0, bad.size, n)]
    v = rng.integers(0, E - 1, n).astype(np.int64)
    return v + (v >= e)


def ids(case):
    """ids[P] (int64; the device gets them as int32)."""
    P, E, name = case.P, case.stack.E, case.routing
    bad = invalid_values(E)
    if name in F.ROUTINGS:
        out = F.routing_ids(F.Case("moe", case.dt, case.seed, case.index, case.stack_index, case.stack, P, case.x_div,
                                   case.cfg, name, case.case_seed))
    else:
        rng = _rng("moe_rb ids", case.case_seed)
        e = int(rng.integers(E))
        if name == "one":
            out = np.full(P, e, np.int64)
        elif name in ("full_blocks", "block_plus_one"):
            assert P > BLOCK
            j = int(rng.integers(max(1, case.j_min), (P - 1) // BLOCK + 1))
            n = BLOCK * j + (name == "block_plus_one")
            while True:  # drawn positions until they are what the name says (n == P: there is one choice)
                at = _subset(rng, P - 1, n - 1) if case.tail else _subset(rng, P, n)
                if case.tail:
                    at = np.append(at, P - 1)
                if n == P or (at[-1] - at[0] >= n and not (at[BLOCK - 1::BLOCK] % ROUND == ROUND - 1).any()):
                    break
            out = _others(rng, E, e, P)
            out[at] = e
        elif name == "none_valid":
            out = bad[rng.integers(0, bad.size, P)]
        elif name == "sorted":
            w = rng.random(E) + 0.2
            if E >= 3:
                idle = _subset(rng, E, int(rng.integers(1, max(1, E // 3) + 1)))
                w[idle] = 0.0
            w = w * (1.0 + 3.0 * (rng.random(E) < 0.3))  # uneven: some experts four times the others' share
            cum = np.cumsum(w)  # (side="right": an expert of weight 0 is never chosen)
            out = np.sort(np.searchsorted(cum, rng.random(P) * cum[-1], side="right").astype(np.int64))
            out = np.minimum(out, int(np.nonzero(w)[0].max()))
        elif name == "late":
            lo = ROUND * ((P - 1) // ROUND)
            at = lo + _subset(rng, P - lo, int(rng.integers(1, P - lo + 1)))
            out = _others(rng, E, e, P)
            out[at] = e
        else:
            raise ValueError(name)
    if case.invalid_edges:
        out = out.copy()
        at = edge_pairs(P)
        out[at] = bad[(np.arange(len(at)) + case.case_seed) % bad.size]
    return out


def digest(cases):
    """sha256 over every field of every case and the ids that follow from them."""
    h = hashlib.sha256()
    for c in cases:
        h.update(repr(sorted(c.fields().items())).encode())
        h.update(ids(c).tobytes())
    return h.hexdigest()
