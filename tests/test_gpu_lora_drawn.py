"""The drawn grouped calls of _lora_draws.py on the device (``-m gpu``): nf4_lora_add through the C
ABI, 1 .. 8 adapters per call, every rank, K from 1 to 33 chunks, every (tile_n, waves).  What the
draw covers is checked on the CPU by test_lora_draws_cpu.py.  For every call:

  * the return code is NF4DQ_OK: a rejected draw fails, nothing is skipped;
  * all outputs are carved from ONE allocation, back to back (``_lora_draws.layout``): between two
    adapters lie only 64 sentinel elements, a band of 4096 on the outside, and every gap and band is
    intact afterwards -- a tile of adapter i that writes into adapter i + 1 has nowhere to hide;
  * an output starts as NaN, or as the base where the adapter is in place;
  * every adapter is judged by ``lora_oracle`` / ``check`` of _lora_cases.py, the suite's own judge;
  * the call is issued again into a fresh allocation and both results have the same bits;
  * afterwards x, every A, every B and every separate base are bitwise what they were.

A failure names (dtype, seed, index) and the case's fields.  ``Runner`` is also what
tools/fuzz_gemm.py --semantics lora drives with other seeds."""
import numpy as np
import pytest
import torch

import _lora_draws as D
from _lora_cases import TDT, check, lora_oracle
from test_gpu_lora import SENTINEL, _launch

pytestmark = pytest.mark.gpu


class Runner:
    """The calls of one dtype.  ``run`` issues one case twice and raises AssertionError if it fails."""

    def __init__(self, dt, gpu):
        from nf4_triton_dequantization_amd import _lib

        self.dt, self.gpu, self._lib = dt, gpu, _lib
        self.launches = 0

    def _dev(self, bits):
        return torch.from_numpy(bits.view(np.int16)).to(self.gpu).view(TDT[self.dt])

    def _outputs(self, c, bases):
        """The one allocation of a call and each adapter's y inside it."""
        offs, total = D.layout(c)
        buf = torch.empty(total, dtype=TDT[self.dt], device=self.gpu)
        buf.view(torch.int16).fill_(SENTINEL)
        ys = []
        for a, o, base in zip(c.adapters, offs, bases):
            y = buf[o:o + c.M * a.N].view(c.M, a.N)
            if a.mode == "inplace":
                y.copy_(base)
            else:
                y.fill_(float("nan"))
            ys.append(y)
        return buf, ys

    def _guards_intact(self, c, buf):
        offs, total = D.layout(c)
        bits = buf.view(torch.int16)
        own = torch.zeros(total, dtype=torch.bool, device=self.gpu)
        for a, o in zip(c.adapters, offs):
            own[o:o + c.M * a.N] = True
        assert int((~own).sum()) == 2 * D.BAND + D.GAP * (len(c.adapters) - 1)
        return bool((bits[~own] == SENTINEL).all())

    def _call(self, c, x, As, Bs, bases, which):
        buf, ys = self._outputs(c, bases)
        descs = []
        for a, A, B, base, y in zip(c.adapters, As, Bs, bases, ys):
            bp = {"null": None, "inplace": y.data_ptr(), "separate": base.data_ptr() if base is not None else None}[a.mode]
            descs.append(self._lib.LoraMat(A.data_ptr(), B.data_ptr(), bp, y.data_ptr(), a.N, a.r, a.scale))
        rc = _launch(x, c.M, c.K, descs, self.dt, c.cfg)
        self.launches += 1
        assert rc == self._lib.OK, f"{which}: rejected: {self._lib.strerror(rc)}"
        assert self._guards_intact(c, buf), f"{which}: a gap between two adapters or an outer band was written"
        return buf, ys

    def run(self, c):
        what = f"lora {self.dt} seed {c.seed} case {c.index}"
        try:
            self._run(c, what)
        except AssertionError as e:
            raise AssertionError(f"{what}: {c.fields()}\n{e}") from None

    def _run(self, c, what):
        assert c.dt == self.dt
        xb, Ab, Bb, baseb = D.inputs(c)
        x = self._dev(xb)
        As, Bs = [], []
        for a, A, B in zip(c.adapters, Ab, Bb):                       # a shared adapter gets the very tensors
            As.append(self._dev(A) if a.share is None else As[a.share])
            Bs.append(self._dev(B) if a.share is None else Bs[a.share])
        bases = [None if b is None else self._dev(b) for b in baseb]
        before = [t.clone() for t in [x] + As + Bs + [b for b in bases if b is not None]]
        buf, ys = self._call(c, x, As, Bs, bases, "first call")
        buf2, ys2 = self._call(c, x, As, Bs, bases, "second call")
        after = [x] + As + Bs + [b for b in bases if b is not None]
        for i, (p, q) in enumerate(zip(before, after)):
            assert torch.equal(p.view(torch.int16), q.view(torch.int16)), f"input tensor {i} (x, the A, the B, the bases) was written"
        for i, (a, A, B, base, y, y2) in enumerate(zip(c.adapters, As, Bs, bases, ys, ys2)):
            ref, bound = lora_oracle(x, A, B, a.scale, self.dt, base)
            check(y, ref, bound, f"adapter {i} (r={a.r} N={a.N} {a.mode} scale={a.scale})")
            if a.scale == 0.0 and base is not None:
                assert torch.equal(y.float(), base.float()), f"adapter {i}: scale 0 must give the base"
            same = y.view(torch.int16) == y2.view(torch.int16)
            if not bool(same.all()):
                at = (~same).nonzero()
                m, n = (int(v) for v in at[0])
                rows, cols = at[:, 0].unique().tolist(), at[:, 1].unique().tolist()
                raise AssertionError(f"adapter {i} (r={a.r} N={a.N} {a.mode}): the same call gave other bits in {at.shape[0]} elements, "
                                     f"rows {rows[:8]}, columns {cols[0]} .. {cols[-1]} ({len(cols)}); first at ({m}, {n}): "
                                     f"{float(y[m, n])!r} then {float(y2[m, n])!r}, reference {float(ref[m, n])!r} +- {float(bound[m, n]):.3g}; "
                                     f"the second call has {int(torch.isnan(y2).sum())} NaN and "
                                     f"{int(((y2.double() - ref).abs() > bound).sum())} elements outside the bound")


@pytest.mark.parametrize("dt", D.DTYPES)
def test_drawn_grouped_calls(gpu, dt):
    cases = D.draws(dt, D.TEST_SEED)
    assert len(cases) == D.DEFAULT_CASES
    R = Runner(dt, gpu)
    for c in cases:
        R.run(c)
    assert R.launches == 2 * len(cases)
