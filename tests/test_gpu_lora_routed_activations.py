"""nf4_lora_add_routed with special rows of x on the GPU (``-m gpu``), both dtypes: what
test_gpu_lora_activations.py does for nf4_lora_add, with the same cases (``_lora_cases.special_case``,
K = 96, N = 80, r = 8 and 40, for the reasons given there) as ONE adapter group of a routed batch.

The batch has S = 3 adapters.  Adapter 0 is named by no row and is NaN throughout (A, B, scale).
Adapter 1 is the group under test, n rows in (1, 5, 17, 33).  Adapter 2 has a plain drawn group of
16 rows, and 4 rows have no adapter.  The rows are interleaved by a fixed permutation in which row 0
of x belongs to adapter 2: the first listed row of the group under test -- which the lanes past the
list re-read -- is not row 0 of x.  ``_activation_cases.positions`` picks LIST positions (0, n - 1, 15,
16): both sides of the 16-row tile edge of the gathered rows.  Under the library's cfg, (16, 1) and
(256, 4), base null and in place, for every kind set:

  * the group under test is judged by class against ``lora_oracle_rows`` on its own rows;
  * a ``zero`` / ``negzero`` row gives the base as values;
  * every row not replaced -- the group's plain rows, the whole of adapter 2's group, the rows without
    an adapter -- has the bits of the same call on the plain draw (``_activation_cases.isolated``): the
    kernel masks by select, and a mask by multiplication (inf * 0 = NaN) would reach them;
  * the group's rows have the bits of nf4_lora_add on those rows at the same waves, or NaN where it
    has NaN (the library's cfg names ``kMaxWaves`` = 4 waves whatever the shape).

Pinned under every cfg: n = 5 with the NaN in the group's first listed row, which list positions
5 .. 15 re-read; a NaN, then +inf, in row 0 of x where that row is adapter 2's or has no adapter.
Further: an infinity in A and a NaN in B of adapter 2 leave every other row's bits; the exact fp16
overflow probe (``overflow_case``) as one group of M = 65, bit for bit with the header's chain; and
one documented consequence of "zero-padded by the caller": an adapter of rank 24 padded to a stack
rank of 40 turns a row of x with an infinity into NaN (inf * 0 in the padded columns of t), where
the unpadded adapter gives infinities -- as the reference on the padded matrices says."""
import copy

import numpy as np
import pytest
import torch

from _activation_cases import isolated
from _lora_cases import (TDT, _INF_BITS, _NAN_BITS, check, check_classes, drawn_case, lora_oracle, lora_oracle_rows, overflow_case,
                         same_bits_or_nan, special_case, special_kind_sets)
from _lora_routed_cases import INT32_MAX, INT32_MIN, scale_of
from test_gpu_lora_routed import CFGS, _lora_add, _run
from nf4_triton_dequantization_amd import _lib

pytestmark = pytest.mark.gpu

K, N, SCALE, S = 96, 80, 1.5, 3         # three K chunks: one per wave and an empty range under four waves
RANKS = (8, 40)
NS_ROWS = (1, 5, 17, 33)
SPECIAL_CFGS = (None, (16, 1), (256, 4))
MODES = ("null", "inplace")
DEFAULT_WAVES = 4                       # nf4_lora_plan.h kMaxWaves: what routed_default_cfg names


def roles(n, n2, none, row0):
    """Who owns each row: 1 (n rows), 2 (n2 rows) or -1 (none), in a fixed shuffled order with row 0 of ``row0``."""
    out = [1] * n + [2] * n2 + [-1] * none
    out = [out[int(i)] for i in np.random.default_rng([n, n2, none]).permutation(len(out))]
    j = out.index(row0)
    out[0], out[j] = out[j], out[0]
    return out


class _Batch:
    """One routed call's inputs on the device: adapter 1 is (A1, B1, SCALE) on rows x1 / base1, adapter 2 and
    the rows without an adapter are drawn, adapter 0 is absent and NaN.  Quacks like ``Routed`` for
    ``test_gpu_lora_routed._run`` and ``_lora_add``."""

    def __init__(self, gpu, dt, x1, A1, B1, base1, n2=16, none=4, row0=2, own_r=None):
        n, self.K = x1.shape
        self.N, self.r = B1.shape
        self.dt, self.S, self.own_r = dt, S, self.r if own_r is None else own_r
        who = roles(n, n2, none, row0)
        self.M = len(who)
        self.groups = {a: [m for m, w in enumerate(who) if w == a] for a in (1, 2)}
        self.none = [m for m, w in enumerate(who) if w == -1]
        assert who[0] == row0 and self.groups[1][0] != 0
        x2, A2, B2, base2 = drawn_case(n2, self.K, self.r, self.N, dt, 2)
        x3, _, _, base3 = drawn_case(none, self.K, self.r, self.N, dt, 99)
        x = torch.zeros(self.M, self.K, dtype=TDT[dt])
        base = torch.zeros(self.M, self.N, dtype=TDT[dt])
        x[self.groups[1]], x[self.groups[2]], x[self.none] = x1, x2, x3
        base[self.groups[1]], base[self.groups[2]], base[self.none] = base1, base2, base3
        A = torch.stack([torch.full_like(A1, float("nan")), A1, A2])
        B = torch.stack([torch.full_like(B1, float("nan")), B1, B2])
        self.scales = [float("nan"), SCALE, scale_of(2)]
        bad = (-1, S, INT32_MIN, INT32_MAX)
        ids = [w if w > 0 else bad[m % 4] for m, w in enumerate(who)]
        self.x, self.base, self.A, self.B = x.to(gpu), base.to(gpu), A.to(gpu), B.to(gpu)
        self.scale = torch.tensor(self.scales, dtype=torch.float32, device=gpu)
        self.ids = torch.tensor(ids, dtype=torch.int32, device=gpu)
        self.a_stride, self.b_stride = self.r * self.K, self.N * self.r

    def x_with(self, x1):
        x = self.x.clone()
        x[self.groups[1]] = x1.to(x.device)
        return x

    def on(self, x):
        """The same batch over another x (a shallow copy: A, B and the rest are shared)."""
        c = copy.copy(self)
        c.x = x
        return c


def _np(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _waves(cfg):
    return DEFAULT_WAVES if cfg is None else cfg[1]


def _special(gpu, n, r, dt, kinds, a_col, cfgs=SPECIAL_CFGS):
    xs, x, A, B, base, rows = special_case(n, K, r, N, dt, kinds, a_col)
    b = _Batch(gpu, dt, x, A, B, base)
    g = b.groups[1]
    bs = b.on(b.x_with(xs))
    replaced = {g[row]: kind for row, kind in rows.items()}
    xg, Ag, Bg, baseg = bs.x[g], b.A[1], b.B[1], b.base[g]
    refs = {"null": lora_oracle_rows(xg, Ag, Bg, SCALE, dt), "inplace": lora_oracle_rows(xg, Ag, Bg, SCALE, dt, baseg)}
    for cfg in cfgs:
        for mode in MODES:
            what = f"n={n} r={r} {dt} {a_col} {rows} rows {g[:4]}.. {mode} cfg={cfg}"
            y = _run(bs, mode, cfg, gpu)
            check_classes(y[g], *refs[mode], what)
            for row, kind in rows.items():
                if kind in ("zero", "negzero"):
                    want = baseg[row] if mode == "inplace" else torch.zeros_like(y[g[row]])
                    assert torch.equal(y[g[row]].float(), want.float()), f"{what}: a {kind} row must give the base"
            isolated(_np(y), _np(_run(b, mode, cfg, gpu)), replaced, what)
            ya = _lora_add(bs, 1, g, mode, (64, _waves(cfg)), gpu, own=False)
            ok = same_bits_or_nan(y[g], ya)
            assert bool(ok.all()), f"{what}: {int((~ok).sum())} outputs are not nf4_lora_add's at {_waves(cfg)} waves"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("n", NS_ROWS)
def test_special_rows_by_class_and_isolated(gpu, n, r, dt):
    for kinds in special_kind_sets(n, dt):
        for a_col in (("nonzero", "mixed") if set(kinds) & {"pinf", "ninf"} else ("nonzero",)):
            _special(gpu, n, r, dt, kinds, a_col)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", RANKS)
def test_nan_in_the_first_listed_row_under_every_cfg(gpu, r, dt):
    """n = 5: list positions 5 .. 15 re-read the first listed row (not row 0 of x), which holds the NaN,
    and must add nothing; the other four rows and every other row of the batch keep their bits."""
    assert special_case(5, K, r, N, dt, ("nan",), "nonzero")[5] == {0: "nan"}
    _special(gpu, 5, r, dt, ("nan",), "nonzero", cfgs=CFGS)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", RANKS)
def test_nan_and_infinity_in_row_zero_of_x_under_every_cfg(gpu, r, dt):
    """Row 0 of x is adapter 2's, or has no adapter: whatever it holds, adapter 1's rows -- whose lanes
    past the list must re-read their own first row, not row 0 of x -- and all others keep their bits."""
    x1, A1, B1, base1 = drawn_case(5, K, r, N, dt, 1)
    for row0 in (2, -1):
        b = _Batch(gpu, dt, x1, A1, B1, base1, row0=row0)
        for kind, bits in (("nan", _NAN_BITS[dt]), ("pinf", _INF_BITS[dt])):
            xs = b.x.clone()
            xs.view(torch.int16)[0, 37] = bits
            bs = b.on(xs)
            for cfg in CFGS:
                for mode in MODES:
                    what = f"r={r} {dt} {kind} in row 0 (of {row0}) {mode} cfg={cfg}"
                    y, y0 = _run(bs, mode, cfg, gpu), _run(b, mode, cfg, gpu)
                    isolated(_np(y), _np(y0), {0: kind} if row0 == 2 else {}, what)
                    if row0 == 2:
                        g = b.groups[2]
                        check_classes(y[g], *lora_oracle_rows(xs[g], b.A[2], b.B[2], b.scales[2], dt, b.base[g] if mode == "inplace" else None), what)
                        assert bool(torch.isnan(y[0]).any() | torch.isinf(y[0]).any())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_non_finite_weights_of_a_neighbour_reach_no_other_row(gpu, dt):
    """Adapter 2's A holds an infinity and its B a NaN: adapter 1's rows and the rows without an adapter
    keep the bits of the clean call."""
    n, r = 17, 40
    x1, A1, B1, base1 = drawn_case(n, K, r, N, dt, 1)
    b = _Batch(gpu, dt, x1, A1, B1, base1)
    d = copy.copy(b)
    d.A, d.B = b.A.clone(), b.B.clone()
    d.A.view(torch.int16)[2, 3, 41] = _INF_BITS[dt]
    d.B.view(torch.int16)[2, 17, 5] = _NAN_BITS[dt]
    keep = b.groups[1] + b.none
    for cfg in SPECIAL_CFGS:
        for mode in MODES:
            y, y0 = _run(d, mode, cfg, gpu), _run(b, mode, cfg, gpu)
            assert torch.equal(y[keep].view(torch.int16), y0[keep].view(torch.int16)), (dt, mode, cfg)
            assert bool(torch.isnan(y[b.groups[2]]).any())           # the dirty adapter was in use
            check(y0[b.groups[1]], *lora_oracle(b.x[b.groups[1]], b.A[1], b.B[1], SCALE, dt, b.base[b.groups[1]] if mode == "inplace" else None),
                  f"{dt} {mode} {cfg}")


def test_exact_overflow_probe_as_one_group_bit_for_bit(gpu):
    """fp16, M = 65: the probe's 33 rows interleaved with a drawn group of 24 and 8 rows without an adapter."""
    x, A, B, base, y_want, v_want = overflow_case()
    b = _Batch(gpu, "f16", x, A, B, base, n2=24, none=8)
    assert b.M == 65 and (b.K, b.r, b.N) == (384, 24, 80)
    g, g2 = b.groups[1], b.groups[2]
    assert g[0] < 64 <= g[-1]                                        # across both ballot masks
    y_want, v_want = y_want.to(gpu), v_want.to(gpu)
    refs2 = {m: lora_oracle(b.x[g2], b.A[2], b.B[2], b.scales[2], "f16", None if m == "null" else b.base[g2]) for m in ("null", "inplace")}
    refs2["separate"] = refs2["inplace"]
    for cfg in CFGS:
        for mode in ("null", "inplace", "separate"):
            y = _run(b, mode, cfg, gpu)
            want = v_want if mode == "null" else y_want
            ok = same_bits_or_nan(y[g], want)
            assert bool(ok.all()), (f"{mode} cfg={cfg}: {int((~ok).sum())} of {ok.numel()} outputs differ from the header's chain "
                                    f"({int(torch.isnan(y[g]).sum())} NaN, {int(torch.isinf(y[g]).sum())} inf; due "
                                    f"{int(torch.isnan(want).sum())} NaN, {int(torch.isinf(want).sum())} inf)")
            check(y[g2], *refs2[mode], f"the drawn group beside the probe: {mode} cfg={cfg}")
            if mode != "inplace":
                want = torch.zeros_like(y[b.none]) if mode == "null" else b.base[b.none]
                assert torch.equal(y[b.none].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_a_zero_padded_adapter_turns_an_infinite_row_into_nan(gpu, dt):
    """The documented consequence of "zero-padded by the caller" (include/nf4_dequant.h): an adapter of
    rank 24 in a stack of rank 40, a row of x with +inf.  t's padded columns are inf * 0 = NaN, so the
    whole row is NaN -- what the reference gives on the padded matrices -- where nf4_lora_add on the
    unpadded adapter gives infinities of a definite sign.  The group's finite rows keep the unpadded bits."""
    n, own_r, r = 5, 24, 40
    xs, x, A, B, base, rows = special_case(n, K, own_r, N, dt, ("pinf",), "nonzero")
    assert rows == {0: "pinf"}
    Ap, Bp = torch.zeros(r, K, dtype=TDT[dt]), torch.zeros(N, r, dtype=TDT[dt])
    Ap[:own_r], Bp[:, :own_r] = A, B
    b = _Batch(gpu, dt, xs, Ap, Bp, base, own_r=own_r)
    g = b.groups[1]
    for cfg in SPECIAL_CFGS:
        for mode in MODES:
            what = f"{dt} {mode} cfg={cfg}"
            bg = b.base[g] if mode == "inplace" else None
            y = _run(b, mode, cfg, gpu)
            check_classes(y[g], *lora_oracle_rows(b.x[g], b.A[1], b.B[1], SCALE, dt, bg), what + " (padded reference)")
            assert bool(torch.isnan(y[g[0]]).all()), what
            ya = _lora_add(b, 1, g, mode, (64, _waves(cfg)), gpu, own=True)
            check_classes(ya, *lora_oracle_rows(b.x[g], b.A[1, :own_r], b.B[1, :, :own_r].contiguous(), SCALE, dt, bg), what + " (unpadded reference)")
            assert bool(torch.isinf(ya[0, :N // 2]).all()) and bool((ya[0, :N // 2] > 0).all()), what
            assert torch.equal(y[g[1:]].view(torch.int16), ya[1:].view(torch.int16)), what + ": the finite rows"
