"""Drawn grouped calls of the fused adapter launch (nf4_lora_add): pure numpy, no torch, no GPU, in
the manner of _family_draws.py.

``draws(dt, seed)`` is a deterministic list of ``Case``: one call of 1 .. 8 adapters over one x.
test_lora_draws_cpu.py checks that the draw is what this text claims (coverage, legality, size, a
pinned digest); test_gpu_lora_drawn.py runs it on the device and tools/fuzz_gemm.py --semantics lora
runs it with other seeds.

The pools: M from ``_family_draws.EDGES`` (the row-tile edges; the kernel takes 16 or 32 rows per
row block); K in K_POOL = 1, 2, 3, 5, 7, 11, 17 and 33 chunks of 32 -- empty wave ranges, uneven
splits, and ranges longer than the load step of 2 (r > 64) or 4 chunks with every tail length; N in
N_POOL; r any multiple of 8 up to 128; 1 .. 8 adapters; cfg None (the library's choice) or any
(tile_n, waves); per adapter a base mode (null, in place, separate) and a scale of SCALES.  An
adapter may read the A and B of an earlier one of its call (``share``).

The first cases of a draw are the MUST list -- what the coverage check names -- so a draw of at
least MIN_CASES cases covers it whatever the seed; the rest are free.  The order is shuffled at the
end.  Only ``Generator.integers`` and ``Generator.random`` are used.

``layout`` says where the outputs of a call lie: ONE allocation, the adapters back to back with only
a gap of GAP sentinel elements between them and BAND outside, so that a tile of adapter i that
writes past its end lands in a gap or in adapter i + 1, both of which are checked.
"""
from __future__ import annotations

import hashlib
from dataclasses import asdict, dataclass, replace
from typing import Optional, Tuple

import numpy as np

from _family_draws import EDGES, _cycle, _pick, _rng, _shuffled

DTYPES = ("bf16", "f16")
K_POOL = (32, 64, 96, 160, 224, 352, 544, 1056)
N_POOL = (16, 48, 80, 256, 272, 528)
R_POOL = tuple(range(8, 129, 8))
TILES = (16, 32, 64, 128, 256)          # nf4_lora_cfg.tile_n
WAVES = (1, 2, 4)                       # nf4_lora_cfg.waves
PAIRS = tuple((t, w) for t in TILES for w in WAVES)
MODES = ("null", "inplace", "separate")
FULL_MANTISSA = float(np.float32(1.9999999))
SCALES = (0.0, -0.75, 1.5, 2.0 ** -20, FULL_MANTISSA)
GROUP_MAX = 8                           # NF4DQ_LORA_GROUP_MAX
DEFAULT_CASES = 64
MIN_CASES = 60
TEST_SEED = 20261                       # the seed the suite runs; the tool takes any other
GAP = 64                                # sentinel elements between two adapters' outputs: 128 bytes
BAND = 4096                             # and on the outside


@dataclass(frozen=True)
class Adapter:
    r: int
    N: int
    mode: str                           # "null" | "inplace" | "separate"
    scale: float
    share: Optional[int] = None         # reads the A and B of this earlier adapter of the call (same r and N)


@dataclass(frozen=True)
class Case:
    dt: str
    seed: int                           # the draw's seed
    index: int                          # position in the draw
    M: int
    K: int
    cfg: Optional[Tuple[int, int]]      # None: the library's choice; (tile_n, waves)
    adapters: Tuple[Adapter, ...]
    case_seed: int                      # seeds the inputs

    def fields(self):
        return asdict(self)

    def rt(self):
        """r tiles of the kernel instantiation: the group's largest r in tiles of 16, up to a power of two."""
        tiles = (max(a.r for a in self.adapters) + 15) // 16
        return 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8

    def input_bytes(self):
        own = [a for a in self.adapters if a.share is None]
        n = self.M * self.K + sum(a.r * self.K + a.N * a.r for a in own) + sum(self.M * a.N for a in self.adapters if a.mode != "null")
        return 2 * n


def _adapter(rng, r=None, N=None, mode=None, scale=None):
    return Adapter(int(_pick(rng, R_POOL)) if r is None else r, int(_pick(rng, N_POOL)) if N is None else N,
                   _pick(rng, MODES) if mode is None else mode, float(_pick(rng, SCALES)) if scale is None else scale)


def _draw_M(rng, small=None):
    pool = EDGES if small is None else [m for m in EDGES if (m <= 16) == small]
    return int(_pick(rng, pool))


def _musts():
    """The forced fields of the first cases of every draw.  "rs": the ranks of the adapters, in order."""
    return [
        {"rs": R_POOL[:8]}, {"rs": R_POOL[:7:-1]},                          # a group of 8, twice: every r
        {"rs": (128, 8), "small": True}, {"rs": (8, 128), "small": False},  # RT = 8 over an adapter of one r tile
        {"rs": (72, 16), "small": True}, {"rs": (16, 72, 16), "small": False},
        {"K": 32, "waves": 4},                                              # one chunk, three waves without one
        {"K": 1056, "waves": 1, "rs": (104,)}, {"K": 1056, "waves": 1, "rs": (40, 128)},  # 33 chunks in steps of 2, one wave
        {"K": 1056, "waves": 1, "rs": (48,)},                               # ... and in steps of 4: a tail of one
        {"K": 544, "waves": 2, "rs": (64,)}, {"K": 1056, "waves": 4, "rs": (24, 56)}, {"K": 352, "waves": 1, "rs": (32,)},  # tails 0, 2, 3
        {"K": 544, "waves": 2, "rs": (88,)},                                # steps of 2 without a tail
        {"rs": (16,)}, {"rs": (8, 8)},                                      # RT = 1
        {"tile_n": 256, "Ns": (16, 16)},                                    # a tile almost wholly past the end
        {"share": True},
    ]


def _names_cfg(must):
    return "waves" in must or "tile_n" in must


def _case(rng, dt, seed, must, cfg):
    rs = must.get("rs")
    count = len(rs) if rs is not None else len(must["Ns"]) if "Ns" in must else int(rng.integers(1, GROUP_MAX + 1))
    if must.get("share") and count < 2:
        count = 2
    M = _draw_M(rng, must.get("small"))
    K = must.get("K", int(_pick(rng, K_POOL)))
    if _names_cfg(must):
        cfg = (must.get("tile_n", int(_pick(rng, TILES))), must.get("waves", int(_pick(rng, WAVES))))
    ads = [_adapter(rng, r=None if rs is None else rs[i], N=must["Ns"][i] if "Ns" in must else None) for i in range(count)]
    if must.get("share") or (not must and count >= 2 and rng.random() < 0.15):
        j = int(rng.integers(1, count))
        i = int(rng.integers(0, j))
        src = ads[i] if ads[i].share is None else ads[ads[i].share]
        i = i if ads[i].share is None else ads[i].share
        ads[j] = replace(ads[j], r=src.r, N=src.N, share=i)
    return Case(dt, seed, -1, M, K, cfg, tuple(ads), int(rng.integers(1, 2 ** 31 - 1)))


def draws(dt, seed, cases=DEFAULT_CASES):
    """The cases of (dt, seed), in the order they are to run."""
    assert dt in DTYPES and cases >= 1
    rng = _rng("lora", dt, seed)
    musts = _musts()
    # the cases that force no part of the cfg take theirs from a cycle: every pair as often as any other
    # (twice at least in a draw of MIN_CASES), the library's choice in 7 of 22
    cfgs = _cycle(rng, [None] * 7 + list(PAIRS), cases)
    out = []
    for i in range(cases):
        must = dict(musts[i]) if i < len(musts) else {}
        out.append(_case(rng, dt, seed, must, None if _names_cfg(must) else cfgs.pop()))
    order = _shuffled(rng, range(len(out)))
    return [replace(out[j], index=i) for i, j in enumerate(order)]


# ---- what a case stands for ---------------------------------------------------------------------------
def to_bits(v, dt):
    """float32 -> the 16-bit patterns of ``dt``, round to nearest even (finite inputs)."""
    v = np.asarray(v, np.float32)
    if dt == "f16":
        return v.astype(np.float16).view(np.uint16)
    b = v.view(np.uint32)
    return ((b + (((b >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)


def _uniform(rng, shape, size):
    """Uniform draws of standard deviation ``size`` (``Generator.random`` alone)."""
    return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(3 ** 0.5 * size)).astype(np.float32)


def inputs(case):
    """(x, [A_i], [B_i], [base_i or None]) as uint16 bit patterns: x, t, u and base all of unit size.
    An adapter with ``share`` gets the very arrays of the one it names."""
    rng = _rng("inputs", case.case_seed)
    x = to_bits(_uniform(rng, (case.M, case.K), 1.0), case.dt)
    As, Bs, bases = [], [], []
    for a in case.adapters:
        if a.share is None:
            As.append(to_bits(_uniform(rng, (a.r, case.K), case.K ** -0.5), case.dt))
            Bs.append(to_bits(_uniform(rng, (a.N, a.r), a.r ** -0.5), case.dt))
        else:
            As.append(As[a.share])
            Bs.append(Bs[a.share])
        bases.append(None if a.mode == "null" else to_bits(_uniform(rng, (case.M, a.N), 1.0), case.dt))
    return x, As, Bs, bases


def layout(case):
    """(offsets, total): the element offset of every adapter's y in the call's one allocation
    [BAND | y_0 | GAP | y_1 | .. | y_last | BAND], and its length."""
    at, offs = BAND, []
    for i, a in enumerate(case.adapters):
        offs.append(at)
        at += case.M * a.N + (GAP if i + 1 < len(case.adapters) else 0)
    return offs, at + BAND


def digest(cases):
    """sha256 over every field of every case and, for the first three, the inputs that follow from them."""
    h = hashlib.sha256()
    for c in cases:
        h.update(repr(sorted(c.fields().items())).encode())
    for c in cases[:3]:
        x, As, Bs, bases = inputs(c)
        for a in [x] + As + Bs + [b for b in bases if b is not None]:
            h.update(a.tobytes())
    return h.hexdigest()
