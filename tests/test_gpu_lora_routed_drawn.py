"""The drawn routed calls of _lora_routed_draws.py on the device (``-m gpu``): nf4_lora_add_routed through
the C ABI, 1 .. 8 stacks per call, up to 64 adapters, group sizes drawn and placed across row 64,
padded adapter strides, every (tile_n, waves).  What the draw covers is checked on the CPU by
test_lora_routed_draws_cpu.py.  The inputs of a stack are a ``_lora_routed_cases.Routed`` with the
drawn pads and scales and ``poison_absent``: the padding between adapters, the A, B and scale of every
adapter no row names and the x of every row without an adapter are NaN, so a launch that reads any of
them shows it.  For every call:

  * the return code is NF4DQ_OK: a rejected draw fails, nothing is skipped;
  * all outputs are carved from ONE allocation, back to back (``_lora_routed_draws.layout``): between
    two stacks lie only 64 sentinel elements, a band of 4096 on the outside, and every gap and band is
    intact afterwards -- a tile of stack i that writes into stack i + 1 has nowhere to hide;
  * an output starts as NaN, or as the base where the stack is in place -- there the rows without an
    adapter start as NaN too, and must come back as they were: not stored at all;
  * every adapter group of every stack is judged by ``lora_oracle`` / ``check`` of _lora_cases.py;
  * rows without an adapter are the base bit for bit, +0 under base NULL;
  * the call is issued again into a fresh allocation and both results have the same bits;
  * under an explicit cfg, the smallest and the largest group of the first and the last stack have the
    bits nf4_lora_add stores for those rows with a contiguous copy of the adapter at the same waves.

A failure names (dtype, seed, index) and the case's fields.  ``Runner`` is also what
tools/fuzz_gemm.py --semantics lora_routed drives with other seeds."""
import pytest
import torch

import _lora_routed_draws as D
from _lora_cases import TDT, check
from _lora_routed_cases import Routed
from test_gpu_lora_routed import SENTINEL, _launch, _lora_add, _stack

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int16)


class Runner:
    """The calls of one dtype.  ``run`` issues one case twice and raises AssertionError if it fails."""

    def __init__(self, dt, gpu):
        from nf4_triton_dequantization_amd import _lib

        self.dt, self.gpu, self._lib = dt, gpu, _lib
        self.launches = self.compared = 0

    def _outputs(self, c, stacks):
        """The one allocation of a call and each stack's y inside it."""
        offs, total = D.layout(c)
        buf = torch.empty(total, dtype=TDT[self.dt], device=self.gpu)
        _bits(buf).fill_(SENTINEL)
        ys = []
        for s, o, R in zip(c.stacks, offs, stacks):
            y = buf[o:o + c.M * s.N].view(c.M, s.N)
            if s.mode == "inplace":
                y.copy_(R.base)
                if R.none:
                    y[R.none] = float("nan")
            else:
                y.fill_(float("nan"))
            ys.append(y)
        return buf, ys

    def _guards_intact(self, c, buf):
        offs, total = D.layout(c)
        own = torch.zeros(total, dtype=torch.bool, device=self.gpu)
        for s, o in zip(c.stacks, offs):
            own[o:o + c.M * s.N] = True
        assert int((~own).sum()) == 2 * D.BAND + D.GAP * (len(c.stacks) - 1)
        return bool((_bits(buf)[~own] == SENTINEL).all())

    def _call(self, c, stacks, which):
        buf, ys = self._outputs(c, stacks)
        first = stacks[0]
        descs = [_stack(R, s.mode, y) for s, R, y in zip(c.stacks, stacks, ys)]
        rc = _launch(first.x, first.ids, c.M, c.K, c.S, descs, self.dt, c.cfg)
        self.launches += 1
        assert rc == self._lib.OK, f"{which}: rejected: {self._lib.strerror(rc)}"
        assert self._guards_intact(c, buf), f"{which}: a gap between two stacks or an outer band was written"
        return buf, ys

    def run(self, c):
        what = f"lora_routed {self.dt} seed {c.seed} case {c.index}"
        try:
            self._run(c)
        except AssertionError as e:
            raise AssertionError(f"{what}: {c.fields()}\n{e}") from None

    def _run(self, c):
        assert c.dt == self.dt
        id_list = [int(v) for v in D.ids(c)]
        stacks = [Routed(self.gpu, c.K, s.r, s.N, self.dt, c.S, id_list, seed=c.case_seed, a_pad=s.a_pad, b_pad=s.b_pad,
                         poison_absent=True, scales=c.scales) for s in c.stacks]
        x = stacks[0].x
        for s, R in zip(c.stacks, stacks):
            assert torch.equal(_bits(R.x), _bits(x))     # drawn from (seed, rows, K) alone: one shared x
            assert (R.a_stride, R.b_stride) == (s.r * c.K + s.a_pad, s.N * s.r + s.b_pad)
            assert {a: len(v) for a, v in R.groups.items()} == dict(c.groups) and len(R.none) == c.none_rows()
        buf, ys = self._call(c, stacks, "first call")
        buf2, ys2 = self._call(c, stacks, "second call")
        for i, (s, R, y, y2) in enumerate(zip(c.stacks, stacks, ys, ys2)):
            what = f"stack {i} (r={s.r} N={s.N} {s.mode} a_pad={s.a_pad} b_pad={s.b_pad})"
            for a, rows in R.groups.items():
                check(y[rows], *R.ref[a][s.mode], f"{what} adapter {a} ({len(rows)} rows {rows[:4]}.., scale {R.scales[a]})")
            if R.none:
                got = _bits(y[R.none])
                want = {"null": torch.zeros_like(got), "separate": _bits(R.base[R.none]),
                        "inplace": torch.full_like(got, _bits(torch.full((1,), float("nan"), dtype=TDT[self.dt]))[0].item())}[s.mode]
                bad = (got != want).any(1).nonzero().flatten().tolist()
                assert not bad, f"{what}: rows without an adapter {[R.none[j] for j in bad][:8]} are not {'untouched' if s.mode == 'inplace' else 'the base'}"
            same = _bits(y) == _bits(y2)
            if not bool(same.all()):
                at = (~same).nonzero()
                m, n = (int(v) for v in at[0])
                raise AssertionError(f"{what}: the same call gave other bits in {at.shape[0]} elements, rows {at[:, 0].unique().tolist()[:8]}; "
                                     f"first at ({m}, {n}): {float(y[m, n])!r} then {float(y2[m, n])!r}")
        if c.cfg is not None and c.groups:               # the bits of nf4_lora_add at the same waves
            by_size = sorted(stacks[0].groups.items(), key=lambda g: (len(g[1]), g[0]))
            for i in sorted({0, len(stacks) - 1}):
                s, R = c.stacks[i], stacks[i]
                for a, rows in dict((by_size[0], by_size[-1])).items():
                    ya = _lora_add(R, a, rows, s.mode, (64, c.cfg[1]), self.gpu, own=False)
                    self.compared += 1
                    assert torch.equal(_bits(ys[i][rows]), _bits(ya)), \
                        f"stack {i} (r={s.r} N={s.N} {s.mode}) adapter {a} ({len(rows)} rows): not the bits of nf4_lora_add at {c.cfg[1]} waves"


@pytest.mark.parametrize("dt", D.DTYPES)
def test_drawn_routed_calls(gpu, dt):
    cases = D.draws(dt, D.TEST_SEED)
    assert len(cases) == D.DEFAULT_CASES >= D.MIN_CASES
    R = Runner(dt, gpu)
    for c in cases:
        R.run(c)
    assert R.launches == 2 * len(cases) and R.compared >= len(cases) // 2
