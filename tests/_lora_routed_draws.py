"""Drawn calls of the routed adapter launch (nf4_lora_add_routed): pure numpy, no torch, no GPU, in
the manner of _lora_draws.py, whose pools and drawing helpers these are.

``draws(dt, seed)`` is a deterministic list of ``Case``: one call of 1 .. 8 stacks of S adapters over
one x and one id vector.  test_lora_routed_draws_cpu.py checks that the draw is what this text claims
(coverage, legality, size, a pinned digest); test_gpu_lora_routed_drawn.py runs it on the device and
tools/fuzz_gemm.py --semantics lora_routed runs it with other seeds.

The pools: M from ``_family_draws.EDGES``; K from ``_lora_draws.K_POOL``; S in S_POOL; per stack r any
multiple of 8 up to 128, N from ``_lora_draws.N_POOL``, a base mode, a_pad in (0, 8, 24, r * K) and
b_pad in (0, 8, 4096) elements between two adapters; cfg None (the library's choice) or any
(tile_n, waves); one scale of ``_lora_draws.SCALES`` per adapter.  S >= 33 comes only with r <= 32 and
K <= 352, and a call whose inputs exceed MAX_BYTES loses its last stacks, then K, until they fit.

The routing is drawn as GROUP SIZES, not ids: ``Case.groups`` is a list of (adapter, rows) whose sizes
sum to at most M; the remaining rows have no adapter and take their ids from (-1, S, INT32_MIN,
INT32_MAX) in turn.  ``ids(case)`` places the rows by a permutation seeded by the case, so a group
generally straddles row 64, the seam between the kernel's two ballot masks; ``Case.place`` pins the
first group instead: "low" (all its rows below 64), "high" (all from 64 on), "low_plus" (rows 0 .. 63,
every one, and the rest from 64 on).

The first cases of a draw are the MUST list -- what the coverage check names -- so a draw of at
least MIN_CASES cases covers it whatever the seed; the rest are free.  The order is shuffled at the
end.  Only ``Generator.integers`` and ``Generator.random`` are used.

``layout`` says where the outputs of a call lie: ONE allocation, the stacks back to back with only a
gap of GAP sentinel elements between them and BAND outside, so that a tile of stack i that writes
past its end lands in a gap or in stack i + 1, both of which are checked.
"""
from __future__ import annotations

import hashlib
from dataclasses import asdict, dataclass, replace
from typing import Optional, Tuple

import numpy as np

from _family_draws import EDGES, _cycle, _pick, _rng, _shuffled
from _lora_draws import DTYPES, K_POOL, MODES, N_POOL, PAIRS, R_POOL, SCALES

S_POOL = (1, 2, 3, 8, 33, 64)
A_PADS = (0, 8, 24, "rK")               # "rK": one whole adapter of padding
B_PADS = (0, 8, 4096)
GROUP_MAX = 8                           # NF4DQ_LORA_GROUP_MAX
MAX_ADAPTERS = 64                       # NF4DQ_LORA_MAX_ADAPTERS
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
BIG_S, BIG_S_R, BIG_S_K = 33, 32, 352   # S >= BIG_S only with r <= BIG_S_R and K <= BIG_S_K
MAX_BYTES = 8 * 2 ** 20                 # the inputs of one call
PLACES = ("perm", "low", "high", "low_plus")
SIZES = (15, 16, 17, 31, 32, 33, 63, 64, 65)   # the group sizes every draw pins within M = 128
DEFAULT_CASES = 48
MIN_CASES = 44
TEST_SEED = 20262                       # the seed the suite runs; the tool takes any other
GAP = 64                                # sentinel elements between two stacks' outputs: 128 bytes
BAND = 4096                             # and on the outside


@dataclass(frozen=True)
class Stack:
    r: int
    N: int
    mode: str                           # "null" | "inplace" | "separate"
    a_pad: int                          # elements between two adapters beyond r * K
    b_pad: int                          # ... beyond N * r


@dataclass(frozen=True)
class Case:
    dt: str
    seed: int                           # the draw's seed
    index: int                          # position in the draw
    M: int
    K: int
    S: int
    cfg: Optional[Tuple[int, int]]      # None: the library's choice; (tile_n, waves)
    stacks: Tuple[Stack, ...]
    scales: Tuple[float, ...]           # one per adapter
    groups: Tuple[Tuple[int, int], ...]  # (adapter, rows), adapters distinct, sizes >= 1
    place: str                          # PLACES: where the first group's rows lie
    case_seed: int                      # seeds the row placement and the inputs

    def fields(self):
        return asdict(self)

    def rt(self):
        """r tiles of the kernel instantiation: the call's largest r in tiles of 16, up to a power of two."""
        tiles = (max(s.r for s in self.stacks) + 15) // 16
        return 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8

    def none_rows(self):
        return self.M - sum(n for _, n in self.groups)

    def input_bytes(self):
        return _bytes(self.M, self.K, self.S, [(s.r, s.N, s.mode, s.a_pad, s.b_pad) for s in self.stacks])


def _bytes(M, K, S, stacks):
    """x, the ids, and per stack the padded A and B, the scales and the base."""
    n = 2 * M * K + 4 * M
    for r, N, mode, a_pad, b_pad in stacks:
        n += 2 * S * (r * K + a_pad + N * r + b_pad) + 4 * S + (0 if mode == "null" else 2 * M * N)
    return n


def _a_pad(kind, r, K):
    return r * K if kind == "rK" else kind


def _musts():
    """The forced fields of the first cases of every draw.  "first": the size of the first group;
    "rs": the ranks of the stacks, in order (None: drawn); "pads" / "mode": of stack 0."""
    pads = [(a, B_PADS[i % 3]) for i, a in enumerate(A_PADS)] + [(A_PADS[i % 4], b) for i, b in enumerate(B_PADS)]
    m = [{"M": 128, "first": n, "beside": True} for n in SIZES]
    for i, p in enumerate(pads):                                        # every a_pad and every b_pad on a stack 0
        m[i]["pads"] = p
    m[7]["mode"], m[8]["mode"] = MODES[0], MODES[1]
    m += [
        {"M": 128, "place": "high", "beside": True, "mode": MODES[2]},  # a group in rows 64 .. 127 alone: the first mask empty
        {"M": 128, "place": "low", "beside": True},
        {"M": 128, "place": "low_plus", "first": 65, "beside": True},    # 64 rows in the first mask and one in the second
        {"M": 65, "S": (33,), "adapters": (31, 32)},                    # the seam between the halves of the 64-bit set
        {"M": 33, "S": (64,), "adapters": (0, 63), "rs": (32, 24)},     # RT = 2
        {"M": 64, "S": (64,), "distinct": True},
        {"M": 1, "S": (64,), "none": 0, "rs": (8,)},                    # RT = 1
        {"S": (2, 3, 8), "rs": (8, 128) + (None,) * 6},                 # 8 stacks, RT = 8 over a stack of one r tile
        {"S": (2, 3), "rs": (88, 16), "beside": True},                  # t rows (104) narrower than the accumulators' 128 columns
        {"scale0": True, "S": (1,), "rs": (40, 64)},                    # RT = 4
        {"M": 15, "none": "all"},
        {"M": 128, "none": 0, "beside": True},
    ]
    return m


def _groups(rng, M, S, must):
    """((adapter, rows), ..): the sizes drawn, the adapters distinct and in a drawn order."""
    none = must.get("none")
    if none == "all":
        return ()
    if must.get("distinct"):
        return tuple((a, 1) for a in _shuffled(rng, range(S))[:M])
    first = must.get("first")
    if must.get("place") in ("low", "high") and first is None:
        first = int(rng.integers(1, min(M, 128) // 2 + 1))
    want = min(2 if must.get("beside") or "adapters" in must else 1, S, M)  # groups at least
    sizes = [] if first is None else [first]
    if none is None:                                                    # half the calls have a row without an adapter
        none = 0 if rng.random() < 0.5 else int(rng.integers(0, M // 4 + 1))
    none = min(none, M - sum(sizes) - (want - len(sizes)))
    left = M - none - sum(sizes)                                        # rows of the groups still to draw
    forced = list(must.get("adapters", ()))
    order = forced + [a for a in _shuffled(rng, range(S)) if a not in forced]
    g_min, g_max = max(0, want - len(sizes)), min(S - len(sizes), left)
    assert g_min <= g_max, (M, S, must)
    g = 0
    if g_max:                                                           # mostly a few groups, sometimes up to one per row
        g = int(rng.integers(max(1, g_min), (g_max if rng.random() < 0.2 else max(g_min, min(g_max, 6))) + 1))
    if g:
        cuts = sorted(_shuffled(rng, range(1, left))[:g - 1])
        sizes += [b - a for a, b in zip([0] + cuts, cuts + [left])]
    return tuple((order[i], n) for i, n in enumerate(sizes))


def _case(rng, dt, seed, must, cfg, mode_cycle, a_cycle, b_cycle):
    S = int(_pick(rng, [s for s in must.get("S", S_POOL) if s >= 2 or not must.get("beside")]))
    rs = must.get("rs")
    if rs is not None and max(r or 0 for r in rs) > BIG_S_R:
        assert S < BIG_S
    big = S >= BIG_S
    M = must.get("M", int(_pick(rng, EDGES)))
    K = int(_pick(rng, [k for k in K_POOL if not big or k <= BIG_S_K]))
    count = len(rs) if rs is not None else int(rng.integers(1, GROUP_MAX + 1))
    r_pool = [r for r in R_POOL if not big or r <= BIG_S_R]
    stacks = []
    for i in range(count):
        r = int(_pick(rng, r_pool)) if rs is None or rs[i] is None else rs[i]
        stacks.append([r, int(_pick(rng, N_POOL)), mode_cycle.pop(), a_cycle.pop(), b_cycle.pop()])
    if "pads" in must:
        stacks[0][3], stacks[0][4] = must["pads"]
    if "mode" in must:
        stacks[0][2] = must["mode"]
    resolved = lambda: [(r, N, mode, _a_pad(a, r, K), b) for r, N, mode, a, b in stacks]  # noqa: E731
    while _bytes(M, K, S, resolved()) > MAX_BYTES:                      # the last stacks go first, then K
        if rs is None and len(stacks) > 1:
            stacks.pop()
        else:
            K = max(k for k in K_POOL if k < K)
    groups = _groups(rng, M, S, must)
    scales = [float(_pick(rng, SCALES)) for _ in range(S)]
    if must.get("scale0"):
        scales[groups[0][0]] = 0.0
    return Case(dt, seed, -1, M, K, S, cfg, tuple(Stack(*s) for s in resolved()), tuple(scales), groups,
                must.get("place", "perm"), int(rng.integers(1, 2 ** 31 - 1)))


def draws(dt, seed, cases=DEFAULT_CASES):
    """The cases of (dt, seed), in the order they are to run."""
    assert dt in DTYPES and cases >= 1
    rng = _rng("lora_routed", dt, seed)
    musts = _musts()
    # every pair as often as any other (twice at least in a draw of MIN_CASES), the library's choice in 7 of 22
    cfgs = _cycle(rng, [None] * 7 + list(PAIRS), cases)
    modes = _cycle(rng, MODES, GROUP_MAX * cases)
    a_pads = _cycle(rng, A_PADS, GROUP_MAX * cases)
    b_pads = _cycle(rng, B_PADS, GROUP_MAX * cases)
    out = []
    for i in range(cases):
        out.append(_case(rng, dt, seed, dict(musts[i]) if i < len(musts) else {}, cfgs.pop(), modes, a_pads, b_pads))
    order = _shuffled(rng, range(len(out)))
    return [replace(out[j], index=i) for i, j in enumerate(order)]


# ---- what a case stands for ---------------------------------------------------------------------------
def ids(case):
    """adapter_ids [M] (int64; the device gets them as int32): the groups' rows placed by a seeded
    permutation (``Case.place``: the first group's rows pinned), the other rows without an adapter."""
    rng = _rng("ids", case.case_seed)
    M, S = case.M, case.S
    rows = _shuffled(rng, range(M))
    if case.place != "perm":
        n0 = case.groups[0][1]
        low, high = [m for m in rows if m < 64], [m for m in rows if m >= 64]
        first = {"low": low[:n0], "high": high[:n0], "low_plus": low + high[:max(0, n0 - len(low))]}[case.place]
        assert len(first) == n0, (case.place, n0, M)
        taken = set(first)
        rows = first + [m for m in rows if m not in taken]
    bad = (-1, S, INT32_MIN, INT32_MAX)
    out = np.empty(M, np.int64)
    at = 0
    for a, n in case.groups:
        out[rows[at:at + n]] = a
        at += n
    for i, m in enumerate(rows[at:]):
        out[m] = bad[i % 4]
    return out


def layout(case):
    """(offsets, total): the element offset of every stack's y in the call's one allocation
    [BAND | y_0 | GAP | y_1 | .. | y_last | BAND], and its length."""
    at, offs = BAND, []
    for i, s in enumerate(case.stacks):
        offs.append(at)
        at += case.M * s.N + (GAP if i + 1 < len(case.stacks) else 0)
    return offs, at + BAND


def digest(cases):
    """sha256 over every field of every case and the ids that follow from them."""
    h = hashlib.sha256()
    for c in cases:
        h.update(repr(sorted(c.fields().items())).encode())
        h.update(ids(c).tobytes())
    return h.hexdigest()
