"""The drawn calls of _moe_rb_draws.py on the device (``-m gpu``): nf4_gemm_bnb_moe_rb through the
C ABI, 1 .. 1024 pairs on the stacks of ``_family_draws.pool("moe", seed)`` (built once per process
by test_gpu_gemm_family_drawn.py's ``_build``, whose cache this file shares).  What the draw covers
is checked on the CPU by test_moe_rb_draws_cpu.py; here every drawn call of a dtype runs in drawn
order on ONE workspace, sized to the largest need of the sequence, zero-filled once and never
cleared again.  For every call:

  * the return code is NF4DQ_OK: a rejected draw fails, nothing is skipped;
  * y is NaN-prefilled between two sentinel bands of 8 rows, which stay intact; x is followed by 16
    NaN rows in the same buffer; the ids are the first P entries of a buffer whose next 64 entries
    are the valid id 0 -- a ballot round that forgot ``p < P`` would list rows beyond P and hit a band;
  * afterwards nf4_gemm_check_workspace is clean and the shared workspace reads 0 over its whole
    length, not only over this call's need;
  * the result is judged by test_gpu_gemm_moe.py's ``_check``, unchanged: the float64 oracle of the
    pair's expert's exact 16-bit weights with the suite's bound, rows of invalid ids zero bits.  No
    tolerance of this file's own;
  * the call is issued again at once, on the used workspace, into a fresh NaN-prefilled output: the
    two outputs are equal bit for bit;
  * a named cfg beyond 128 pairs: two subsets of at most 128 pairs -- a drawn window
    [128 j, 128 j + 128) of the pairs, and every ceil(P / 128)-th pair from a drawn start -- run
    through nf4_gemm_bnb_moe at the same (waves, ksplit) on their own gathered x rows (x_div 1) and on
    the same shared workspace; the subset's rows of the row-block output have exactly those bits;
  * up to 128 pairs: the whole output equals nf4_gemm_bnb_moe's bit for bit, under the named cfg and
    under each library's own choice;
  * ``none_valid``: y is all zero bits (no workgroup computes; the workspace stays zero as after
    every call).

A failure names (dtype, seed, index) and the case's fields.  ``Runner`` is also what
tools/fuzz_gemm.py --semantics moe_rb drives with other seeds."""
import ctypes

import numpy as np
import pytest
import torch

import _family_draws as F
import _moe_rb_draws as D
import test_gpu_gemm_moe as MOE
import test_gpu_gemm_moe_rb as RB
from test_gpu_gemm_family_drawn import BAND, HEADER, _build

pytestmark = pytest.mark.gpu

_tdt = MOE._tdt
X_TAIL, ID_TAIL = 16, 64


class Runner:
    """The calls of one dtype on one workspace.  ``prepare`` builds the stacks and the workspace for
    a list of cases; ``run`` issues one case and raises AssertionError if it fails."""

    def __init__(self, dt, coracle, gpu):
        self.dt, self.coracle, self.gpu = dt, coracle, gpu
        self._lib, self.L = MOE._lib_and_L()
        self.ws = None
        self.launches = 0

    def stack(self, c):
        return _build(self.coracle, self.gpu, c.stack, self.dt, False)

    def need(self, c):
        """The largest workspace any launch of the case asks for."""
        d = self.stack(c).desc()
        dp = ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
        cfg = None if c.cfg is None else RB._cfg(*c.cfg)
        out = [self.L.nf4_gemm_bnb_moe_rb_workspace_bytes(c.P, dp, ctypes.byref(cfg) if cfg is not None else None)]
        if c.cfg is not None and c.cfg[1] > 1:
            assert out[0] == HEADER + c.cfg[1] * c.P * c.stack.N * 4
        if c.P <= D.BLOCK:
            out.append(self.L.nf4_gemm_bnb_moe_rb_workspace_bytes(c.P, dp, None))
            out.append(self.L.nf4_gemm_bnb_moe_workspace_bytes(c.P, dp, None))
        return max(out)  # (nf4_gemm_bnb_moe under the named cfg: the same slabs over at most as many pairs)

    def prepare(self, cases):
        """One workspace for the whole sequence: zero-filled here, never again."""
        size = max([HEADER] + [self.need(c) for c in cases])
        if self.ws is None or self.ws.numel() < size:
            self.ws = torch.zeros(size, dtype=torch.uint8, device=self.gpu)

    def out(self, P, N):
        """A fresh output [band | NaN rows | band]."""
        buf = torch.full((BAND + P + BAND, N), 0x5A5B, dtype=torch.int16, device=self.gpu)
        buf[BAND:BAND + P] = torch.full((P, N), float("nan"), dtype=_tdt(self.dt), device=self.gpu).view(torch.int16)
        return buf, buf[BAND:BAND + P]

    def launch(self, call, S, x_ptr, ids, P, x_div, cfg, which):
        """One launch of ``call`` (an entry's ``_call``) on the shared workspace into a fresh output;
        bands, error word and workspace afterwards."""
        buf, y = self.out(P, S.N)
        call(S, x_ptr, ids, P, x_div, y.data_ptr(), cfg, ws=self.ws)  # asserts NF4DQ_OK
        self.launches += 1
        sp = torch.cuda.current_stream().cuda_stream
        assert self.L.nf4_gemm_check_workspace(self.ws.data_ptr(), self.ws.numel(), sp) == 0, f"{which}: workspace error word"
        assert bool((buf[:BAND] == 0x5A5B).all()) and bool((buf[BAND + P:] == 0x5A5B).all()), f"{which}: a sentinel band was written"
        left = int(self.ws.count_nonzero())
        assert left == 0, f"{which}: {left} bytes of the shared workspace left set"
        return y

    def run(self, c):
        what = f"moe_rb {self.dt} seed {c.seed} case {c.index}"
        try:
            self._run(c, what)
        except AssertionError as e:
            raise AssertionError(f"{what}: {c.fields()}\n{e}") from None

    def _run(self, c, what):
        assert c.dt == self.dt
        assert self.ws is not None and self.need(c) <= self.ws.numel(), "prepare() the sequence first"
        S, P, N, K = self.stack(c), c.P, c.stack.N, c.stack.K
        M = -(-P // c.x_div)
        xt, xb = MOE._x(M, K, self.dt)
        xbuf = torch.full((M + X_TAIL, K), float("nan"), dtype=_tdt(self.dt), device=self.gpu)
        xbuf[:M] = xt.to(self.gpu)
        ids_np = D.ids(c)
        idbuf = torch.zeros(P + ID_TAIL, dtype=torch.int32, device=self.gpu)
        idbuf[:P] = torch.from_numpy(ids_np.astype(np.int32)).to(self.gpu)
        ids = idbuf[:P]
        cfg = None if c.cfg is None else RB._cfg(*c.cfg)
        y = self.launch(RB._call, S, xbuf.data_ptr(), ids, P, c.x_div, cfg, "first call")
        y2 = self.launch(RB._call, S, xbuf.data_ptr(), ids, P, c.x_div, cfg, "second call")
        MOE._check(S, y.view(_tdt(self.dt)), xb, ids_np, c.x_div, what)
        assert torch.equal(y, y2), f"the same call on the used workspace gave other bits in {int((y != y2).sum())} elements"
        if c.routing == "none_valid":
            assert int(y.count_nonzero()) == 0, "every id invalid: y must be all zero bits"
        if P <= D.BLOCK:  # the two entries agree up to 128 pairs
            for name, rb_cfg, moe_cfg in (("the named cfg", cfg, c.cfg and MOE._cfg(*c.cfg)), ("the library's choice", None, None)):
                if name == "the named cfg" and cfg is None:
                    continue
                a = y if rb_cfg is cfg else self.launch(RB._call, S, xbuf.data_ptr(), ids, P, c.x_div, None, f"{name}, row blocks")
                b = self.launch(MOE._call, S, xbuf.data_ptr(), ids, P, c.x_div, moe_cfg, f"{name}, nf4_gemm_bnb_moe")
                assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ from nf4_gemm_bnb_moe's at {P} pairs"
        elif cfg is not None:  # row independence
            rng = F._rng("moe_rb rows", c.case_seed)
            blocks = -(-P // D.BLOCK)
            j, start = int(rng.integers(blocks)), int(rng.integers(blocks))
            for name, sel in ((f"pairs {D.BLOCK * j} .. {min(P, D.BLOCK * j + D.BLOCK) - 1}", np.arange(D.BLOCK * j, min(P, D.BLOCK * j + D.BLOCK))),
                              (f"every {blocks}-th pair from {start}", np.arange(start, P, blocks))):
                assert 1 <= sel.size <= D.BLOCK
                sel_t = torch.from_numpy(sel).to(self.gpu)
                xs = torch.full((sel.size + X_TAIL, K), float("nan"), dtype=_tdt(self.dt), device=self.gpu)
                xs[:sel.size] = xbuf[sel_t // c.x_div]
                sub_ids = idbuf[sel_t].contiguous()
                sub = self.launch(MOE._call, S, xs.data_ptr(), sub_ids, sel.size, 1, MOE._cfg(*c.cfg), f"{name}, nf4_gemm_bnb_moe")
                same = sub == y[sel_t]
                assert bool(same.all()), (f"{name}: {int((~same).sum())} of {same.numel()} outputs differ from nf4_gemm_bnb_moe's "
                                          f"at cfg {c.cfg}, first at {(~same).nonzero()[0].tolist()}")


@pytest.mark.parametrize("dt", D.DTYPES)
def test_drawn_calls_on_one_workspace(coracle, gpu, dt):
    cases = D.draws(dt, D.TEST_SEED)
    assert len(cases) == D.DEFAULT_CASES
    R = Runner(dt, coracle, gpu)
    R.prepare(cases)
    for c in cases:
        R.run(c)
