"""Drawn cases for the row-tiled and the expert GEMM family (nf4_gemm_bnb_mt, nf4_gemm_bnb_mt_swiglu,
nf4_gemm_bnb_moe, nf4_gemm_bnb_moe_swiglu, nf4_gemm_bnb_moe_down): pure numpy, no torch, no GPU.

``draws(entry, dt, seed)`` is a deterministic list of ``Case``: a weight stack from a small pool and
one call on it.  test_family_draws_cpu.py checks that the draw is what this text claims (coverage,
legality, size, a pinned digest); test_gpu_gemm_family_drawn.py runs it on the device and
tools/fuzz_gemm.py --semantics family runs it with other seeds.

The pool (``pool``): at most 12 stacks, the smallest shapes the kernels accept -- N (I) in N_POOL,
K in K_POOL (one chunk, an even and an uneven two-slice split, five chunks that wrap the four-deep
weight ring, nine chunks), E in E_POOL (E >= 64 only with N = 64 and K <= 384), nested or single
statistics, blocksize2, one shared or a per-expert code2 table, offsets or a NULL pointer, and
padded strides (packed: multiples of 16 bytes).  A stack is what test_gpu_gemm_moe._Stack builds from
a ``Stack``; the SwiGLU entries add ``Stack.up`` through test_gpu_gemm_moe_swiglu._UpStack.  The two
dense entries use expert ``Case.expert`` of a stack as their weight.

A call: P (M for the dense entries) in 1 .. 128 with extra weight at the row-tile edges, x_div in
1 .. 8 (any value, not only divisors of P), cfg None or (waves, ksplit) legal by
include/nf4_dequant.h, a routing by name (``routing_ids``), and for moe_down topk (a divisor of P),
x_div in {1, topk} and the dtype of the routing weights.  The first cases of a draw are the MUST
list -- what the coverage check of test_family_draws_cpu.py names, and the combinations no
enumerated suite has -- so a draw of at least MIN_CASES cases covers them whatever the seed; the
rest are free.  The order is shuffled at the end.

Only ``Generator.integers`` and ``Generator.random`` are used, so the digest does not depend on how
numpy implements its shuffles and choices.
"""
from __future__ import annotations

import hashlib
import zlib
from dataclasses import asdict, dataclass, replace
from typing import Optional, Tuple

import numpy as np

ENTRIES = ("mt", "mt_swiglu", "moe", "moe_swiglu", "moe_down")
DTYPES = ("bf16", "f16")
MOE_ENTRIES = ("moe", "moe_swiglu", "moe_down")
SWIGLU_ENTRIES = ("mt_swiglu", "moe_swiglu")
N_POOL = (64, 128, 192, 256)
K_POOL = (128, 256, 384, 640, 1152)
E_POOL = (1, 3, 8, 17, 64, 256)
BS2_POOL = (16, 64, 256)
ROUTINGS = ("uniform", "zipf", "last", "first", "distinct", "high", "invalid_share", "dead_token", "twice")
INVALID = (-1, None, None, -2 ** 31, 2 ** 31 - 1)  # None: E and E + 1
EDGES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128)
DEFAULT_CASES = 60
TEST_SEED = 20260  # the seed the suites run; the tool takes any other
MIN_CASES = 48
MAX_STACKS = 12


@dataclass(frozen=True)
class Stack:
    """One weight stack.  pads: what packed_stride (bytes, % 16 == 0), nb_stride (bytes) and
    n2_stride (floats) exceed their data by.  bs2 / code2_stride / offset mean nothing in single
    mode.  up: the up stack of the SwiGLU entries (same mode, E, N, K)."""
    mode: str
    E: int
    N: int
    K: int
    bs2: int
    code2_stride: int   # 0: one table for all experts; 256: one per expert
    offset: bool        # False: the descriptor's offset pointer is NULL
    pads: Tuple[int, int, int]
    up: Optional["Stack"] = None

    def nbytes(self):
        """Bytes of the stack on the device (and of its up stack)."""
        nblk = self.N * self.K // 64
        n = self.E * (self.N * self.K // 2 + self.pads[0])
        if self.mode == "nested":
            n += self.E * (nblk + self.pads[1]) + 4 * self.E * (-(-nblk // self.bs2) + self.pads[2])
            n += 4 * 256 * (self.E if self.code2_stride else 1) + 4 * self.E
        else:
            n += 4 * self.E * (nblk + self.pads[2])
        return n + (self.up.nbytes() if self.up else 0)


@dataclass(frozen=True)
class Case:
    entry: str
    dt: str
    seed: int                       # the draw's seed
    index: int                      # position in the draw
    stack_index: int
    stack: Stack
    P: int                          # pairs; the rows M of the dense entries
    x_div: int
    cfg: Optional[Tuple[int, int]]  # None: the library's choice; (waves, ksplit)
    routing: Optional[str]          # None for the dense entries
    case_seed: int                  # seeds the ids and the routing weights
    expert: int = 0                 # dense entries: which weight of the stack
    topk: int = 1                   # moe_down
    rw_dtype: str = "f32"           # moe_down: "f32" or "out"

    def fields(self):
        return asdict(self)


# ---- drawing helpers: integers() and random() only ------------------------------------------------
def _rng(*words):
    return np.random.default_rng([zlib.crc32("/".join(str(w) for w in words).encode()) & 0xFFFFFFFF, 0x6E6634])


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _shuffled(rng, seq):
    out = list(seq)
    for i in range(len(out) - 1, 0, -1):
        j = int(rng.integers(i + 1))
        out[i], out[j] = out[j], out[i]
    return out


def _cycle(rng, seq, n):
    """n values, every one of seq as often as any other (up to one), in a drawn order."""
    out = []
    while len(out) < n:
        out += _shuffled(rng, seq)
    return out[:n]


# ---- the stack pool -------------------------------------------------------------------------------
def _one_stack(rng, mode, E, N, K, bs2, c2s, off):
    pads = (16 * int(rng.integers(0, 300)), int(rng.integers(0, 9)), int(rng.integers(0, 5)))
    return Stack(mode, E, N, K, bs2, c2s, off, pads)


def pool(entry, seed):
    """The stacks of an entry: the same for both dtypes.  Eight nested and four single ones; among
    the nested each blocksize2, both code2 sharings and both offset forms at least twice; every N,
    K and (expert entries) E of the pools."""
    rng = _rng("pool", entry, seed)
    moe = entry in MOE_ENTRIES
    # (E, N or None = drawn, K or None = drawn); the fixed ones are the issue's own combinations
    if moe:
        shapes = [(256, 64, 384), (256, 64, _pick(rng, (128, 256))), (64, 64, _pick(rng, (128, 256, 384))), (64, 64, 256),
                  (17, None, 1152), (17, None, None), (8, 256, None), (8, None, None), (3, None, None), (3, None, None),
                  (1, None, None), (1, None, None)]
    else:
        shapes = [(_pick(rng, (1, 3)), None, None) for _ in range(MAX_STACKS - 1)] + [(3, 256, 1152)]
    free_n = _cycle(rng, N_POOL, sum(s[1] is None for s in shapes))
    free_k = _cycle(rng, K_POOL, sum(s[2] is None for s in shapes))
    shapes = [(E, free_n.pop() if N is None else N, free_k.pop() if K is None else K) for E, N, K in shapes]
    if moe:  # both modes at E = 256 and at E = 64
        modes = _shuffled(rng, ["nested", "single"]) + _shuffled(rng, ["nested", "single"]) + \
            _shuffled(rng, ["nested"] * 6 + ["single"] * 2)
    else:
        modes = _shuffled(rng, ["nested"] * 8 + ["single"] * 4)
    bs2 = _cycle(rng, BS2_POOL, MAX_STACKS)
    c2s = _cycle(rng, (0, 256), MAX_STACKS)
    off = _cycle(rng, (False, True), MAX_STACKS)
    ubs2 = _cycle(rng, BS2_POOL, MAX_STACKS)
    uc2s = _cycle(rng, (0, 256), MAX_STACKS)
    uoff = _cycle(rng, (False, True), MAX_STACKS)
    out, j = [], 0
    for i, (E, N, K) in enumerate(shapes):
        nested = modes[i] == "nested"
        s = _one_stack(rng, modes[i], E, N, K, bs2[j] if nested else 0, c2s[j] if nested else 0, off[j] if nested else False)
        u = _one_stack(rng, modes[i], E, N, K, ubs2[j] if nested else 0, uc2s[j] if nested else 0, uoff[j] if nested else False)
        j += nested
        out.append(replace(s, up=u) if entry in SWIGLU_ENTRIES else s)
    order = _shuffled(rng, range(len(out)))
    return [out[i] for i in order]


# ---- legality (the generator's own; test_family_draws_cpu.py restates it from the header) ----------
def wave_choices(entry, N):
    cols = 16 if entry in SWIGLU_ENTRIES else 32
    return [w for w in (2, 4) if N % (cols * w) == 0]


def ksplit_max(K):
    return min(K // 128, 16)


def last_slice_empty(K, ksplit):
    chunks = K // 128
    cps = -(-chunks // ksplit)
    return (ksplit - 1) * cps >= chunks


# ---- one call --------------------------------------------------------------------------------------
def _draw_P(rng):
    return int(_pick(rng, EDGES)) if rng.random() < 0.6 else int(rng.integers(1, 129))


def _divisors(P):
    return [k for k in range(1, 9) if P % k == 0]


def _case(rng, entry, dt, seed, stacks, si, must):
    """One case on stack `si` (or the first stack from `si` on that satisfies must["stack"]), with
    the fields of `must` forced and the rest drawn."""
    want = must.get("stack")
    if want is not None:
        si = next(i % len(stacks) for i in range(si, si + len(stacks)) if want(stacks[i % len(stacks)]))
    S = stacks[si]
    moe = entry in MOE_ENTRIES
    P = must["P"] if "P" in must else _draw_P(rng)
    topk, x_div, rw = 1, 1, "f32"
    if entry == "moe_down":
        topk = must.get("topk")
        if topk is None:
            topk = int(_pick(rng, _divisors(P)))
        if P % topk:  # a forced topk with a drawn P: the nearest multiple, at least one token
            P = max(topk, P - P % topk)
        x_div = must.get("x_div", int(_pick(rng, (1, topk))))
        rw = must.get("rw_dtype", _pick(rng, ("f32", "out")))
    elif moe:
        x_div = must.get("x_div", int(rng.integers(1, 9)))
    if "cfg" in must:
        cfg = must["cfg"]
        if cfg is not None:
            w, ks = cfg
            w = int(_pick(rng, wave_choices(entry, S.N))) if w is None else w
            ks = int(rng.integers(1, ksplit_max(S.K) + 1)) if ks is None else ksplit_max(S.K) if ks == "max" else ks
            cfg = (w, ks)
    else:
        cfg = (int(_pick(rng, wave_choices(entry, S.N))), int(rng.integers(1, ksplit_max(S.K) + 1)))
    routing = None
    if moe:
        group = topk if entry == "moe_down" else x_div
        ok = [r for r in ROUTINGS if (r != "high" or S.E > 128) and (r != "twice" or (group >= 2 and P >= 2))]
        routing = must.get("routing", _pick(rng, ok))
        assert routing in ok, (routing, S.E, group, P)
    return Case(entry, dt, seed, -1, si, S, P, x_div, cfg, routing, int(rng.integers(1, 2 ** 31 - 1)),
                0 if moe else int(rng.integers(S.E)), topk, rw)


def _musts(entry):
    """The forced fields of the first cases of every draw.  "stack": a predicate on the Stack."""
    w4 = lambda s: 4 in wave_choices(entry, s.N)  # noqa: E731
    m = [
        # every instantiation at its upper edge, both wave counts
        {"P": 32, "cfg": (2, None)}, {"P": 64, "cfg": (4, None), "stack": w4}, {"P": 96, "cfg": (2, None)},
        {"P": 128, "cfg": (4, None), "stack": w4},
        # one slice named, one slice per chunk, empty last slices (K = 1152: 9 chunks in 7 slices of 2; K = 640: 5 in 4 of 2)
        {"cfg": (None, 1)}, {"cfg": (None, "max"), "stack": lambda s: s.K >= 384},
        {"cfg": (2, 7), "stack": lambda s: s.K == 1152 and (entry not in MOE_ENTRIES or s.E == 17)},
        {"cfg": (None, 4), "stack": lambda s: s.K == 640},
        # two waves on N = 256 with one pair
        {"P": 1, "cfg": (2, None), "stack": lambda s: s.N == 256},
    ]
    if entry in MOE_ENTRIES:
        big = lambda s: s.E == 256  # noqa: E731
        xd = (lambda v: {}) if entry == "moe_down" else (lambda v: {"x_div": v})
        two = {"topk": 2} if entry == "moe_down" else {"x_div": 2}
        m += [
            # 128 pairs on 128 distinct experts of 256; the last ticket; E itself as an invalid id; experts >= 128 alone
            {"P": 128, "routing": "distinct", "stack": big}, {"routing": "last", "stack": big},
            {"routing": "invalid_share", "stack": big, "P": 97}, {"routing": "high", "stack": big},
            {"routing": "dead_token", "stack": lambda s: s.E >= 64}, {"routing": "first", "stack": lambda s: s.E >= 64, "cfg": None},
            {"routing": "uniform"}, {"routing": "zipf", "P": 127}, {"routing": "distinct"}, {"routing": "last"},
            {"routing": "first"}, {"routing": "invalid_share"}, dict({"routing": "dead_token"}, **two),
            dict({"routing": "twice", "P": 48}, **two),
            # odd x_div against a row-tile edge
            dict({"P": 33}, **xd(3)), dict({"P": 65}, **xd(5)), dict({"P": 97}, **xd(7)), dict({"P": 17}, **xd(8)),
        ]
    if entry == "moe_down":
        m += [{"topk": k, "rw_dtype": ("f32", "out")[k & 1]} for k in range(1, 9)]
        m += [{"topk": 5, "x_div": 5, "P": 95}, {"topk": 6, "x_div": 6, "P": 96}, {"topk": 7, "x_div": 1, "rw_dtype": "out"},
              {"topk": 2, "x_div": 2, "rw_dtype": "f32"}]
    return m


def draws(entry, dt, seed, cases=DEFAULT_CASES):
    """The cases of (entry, dt, seed), in the order they are to run."""
    assert entry in ENTRIES and dt in DTYPES and cases >= 1
    stacks = pool(entry, seed)
    rng = _rng("calls", entry, dt, seed)
    musts = _musts(entry)
    out = []
    for i in range(cases):
        # two of five cases that force no cfg take the library's choice: more than a quarter of any
        # draw of MIN_CASES or more, whatever the MUST list forces
        must = dict(musts[i]) if i < len(musts) else {}
        if i % 5 in (0, 2):
            must.setdefault("cfg", None)
        out.append(_case(rng, entry, dt, seed, stacks, i % len(stacks), must))
    order = _shuffled(rng, range(len(out)))
    return [replace(out[j], index=i) for i, j in enumerate(order)]


# ---- what a case stands for -------------------------------------------------------------------------
def routing_ids(case):
    """ids[P] (int64; the device gets them as int32) of an expert entry's case."""
    rng = _rng("ids", case.case_seed)
    P, E, name = case.P, case.stack.E, case.routing
    group = max(1, min(P, case.topk if case.entry == "moe_down" else case.x_div))
    bad = np.array([v if v is not None else E + i - 1 for i, v in enumerate(INVALID)], np.int64)  # -1, E, E + 1, INT_MIN, INT_MAX
    ids = rng.integers(0, E, P).astype(np.int64)
    if name == "uniform":
        pass
    elif name == "zipf":  # one hot expert takes most pairs
        ids = np.where(rng.random(P) < 0.75, int(rng.integers(E)), ids)
    elif name == "last":
        ids[:] = E - 1
    elif name == "first":
        ids[:] = 0
    elif name == "distinct":  # min(P, E) experts with one pair each; a pair beyond them has no expert
        experts = np.argsort(rng.random(E), kind="stable")[:min(P, E)]
        slots = np.argsort(rng.random(P), kind="stable")[:experts.size]
        ids[:] = -1
        ids[slots] = experts
    elif name == "high":
        ids = rng.integers(128, E, P).astype(np.int64)
    elif name == "invalid_share":
        hit = rng.random(P) < 0.3
        hit[int(rng.integers(P))] = True
        ids = np.where(hit, bad[rng.integers(0, bad.size, P)], ids)
    elif name == "dead_token":  # token 0: every id invalid
        ids[:group] = bad[(np.arange(group) + int(rng.integers(bad.size))) % bad.size]
    elif name == "twice":
        ids[1] = ids[0]
    else:
        raise ValueError(name)
    return ids


def routing_weights(case):
    """fp32 routing weights in (0, 1) with all their mantissa bits (moe_down): none is a 16-bit value."""
    w = _rng("rw", case.case_seed).random(case.P, dtype=np.float32) * np.float32(0.96) + np.float32(0.02)
    return np.where((w.view(np.uint32) & 0xFFFF) == 0, np.nextafter(w, np.float32(1)), w).astype(np.float32)


def digest(cases):
    """sha256 over every field of every case and the ids / routing weights that follow from them."""
    h = hashlib.sha256()
    for c in cases:
        h.update(repr(sorted(c.fields().items())).encode())
        if c.routing is not None:
            h.update(routing_ids(c).tobytes())
        if c.entry == "moe_down":
            h.update(routing_weights(c).tobytes())
    return h.hexdigest()
