"""nf4_lora_add with special rows of x on the GPU (``-m gpu``), both dtypes: what
test_gpu_gemm_activations.py does for the GEMM entries.  Rows chosen by ``_activation_cases.positions``
(both sides of the 16-row tile edge, the last row) are replaced by a NaN, +inf, -inf, all +0, all -0,
and fp16 subnormals (``tiny``) or bf16 values of 2^-100 (``small``); ``_lora_cases.special_case``
says where the infinity sits and what A and B are.  One adapter with r = 8 (padding inside a 16-row
tile of A) and one with r = 40 (padding inside the MFMA depth of 32, three r tiles in the RT = 4
instantiation), at M = 1, 17 and 33, under the library's cfg, (16, 1) and (256, 4), base null and in
place.  For every call:

  * the float64 chain by elementwise product and sum (``lora_oracle_rows``) judges by class: NaN where
    the reference is NaN, the same infinity where it is infinite, within ``lora_oracle``'s bound where
    it is finite;
  * a ``zero`` / ``negzero`` row with a base equals the base as values;
  * every row not replaced has the bits of the same call on the plain draw
    (``_activation_cases.isolated``): the kernel masks by select, and a mask by multiplication --
    inf * 0 = NaN -- would reach a neighbour's row or a padded column;
  * the sentinel bands around the output stay intact, and the output starts as NaN.

One case puts the NaN in row 0 of x with M = 5: the lanes past M re-read row 0 and must contribute
nothing.  ``huge`` is left out -- a float64 chain cannot say where rn(t) overflows -- and its place is
taken by the exact overflow probe (``overflow_case``, fp16): some exact t exceed 65520 and become
infinity, and u, v and y follow by the header's chain, compared bit for bit (NaN where NaN)."""
import numpy as np
import pytest
import torch

from _activation_cases import isolated
from _lora_cases import check_classes, lora_oracle_rows, overflow_case, same_bits_or_nan, special_case, special_kind_sets
from test_gpu_lora import CFGS, _bands_intact, _guarded, _launch
from nf4_triton_dequantization_amd import _lib

pytestmark = pytest.mark.gpu

K, N, SCALE = 96, 80, 1.5               # three K chunks: one per wave and an empty range under four waves
RANKS = (8, 40)
MS = (1, 17, 33)
SPECIAL_CFGS = (None, (16, 1), (256, 4))
MODES = ("null", "inplace")


class _Call:
    """One adapter's inputs on the device; ``run`` launches it on a given x."""

    def __init__(self, gpu, M, A, B, base, dt, scale=SCALE):
        self.M, self.N, self.r, self.dt, self.scale = M, B.shape[0], A.shape[0], dt, scale
        self.A, self.B, self.base = A.to(gpu), B.to(gpu), base.to(gpu)

    def run(self, x, mode, cfg, gpu):
        buf, y = _guarded(self, mode, gpu)
        base = {"null": None, "inplace": y.data_ptr(), "separate": self.base.data_ptr()}[mode]
        d = _lib.LoraMat(self.A.data_ptr(), self.B.data_ptr(), base, y.data_ptr(), self.N, self.r, self.scale)
        rc = _launch(x, self.M, x.shape[1], [d], self.dt, cfg)
        assert rc == _lib.OK, (rc, cfg)
        assert _bands_intact(buf, self.M * self.N), f"a write outside the output: {mode} {cfg}"
        return y


def _bits(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _special(gpu, M, r, dt, kinds, a_col, cfgs=SPECIAL_CFGS):
    xs, x, A, B, base, rows = special_case(M, K, r, N, dt, kinds, a_col)
    call = _Call(gpu, M, A, B, base, dt)
    xs, x = xs.to(gpu), x.to(gpu)
    refs = {"null": lora_oracle_rows(xs, call.A, call.B, SCALE, dt), "inplace": lora_oracle_rows(xs, call.A, call.B, SCALE, dt, call.base)}
    for cfg in cfgs:
        for mode in MODES:
            what = f"M={M} r={r} {dt} {a_col} {rows} {mode} cfg={cfg}"
            y = call.run(xs, mode, cfg, gpu)
            check_classes(y, *refs[mode], what)
            for row, kind in rows.items():
                if kind in ("zero", "negzero"):
                    want = call.base[row] if mode == "inplace" else torch.zeros_like(y[row])
                    assert torch.equal(y[row].float(), want.float()), f"{what}: a {kind} row must give the base"
            if M > len(rows):
                isolated(_bits(y), _bits(call.run(x, mode, cfg, gpu)), rows, what)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M", MS)
def test_special_rows_by_class_and_isolated(gpu, M, r, dt):
    for kinds in special_kind_sets(M, dt):
        for a_col in (("nonzero", "mixed") if set(kinds) & {"pinf", "ninf"} else ("nonzero",)):
            _special(gpu, M, r, dt, kinds, a_col)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("r", RANKS)
def test_nan_in_row_zero_under_every_cfg(gpu, r, dt):
    """M = 5: lanes 5 .. 15 of the row tile re-read row 0, which holds the NaN; rows 1 .. 4 keep their bits."""
    _special(gpu, 5, r, dt, ("nan",), "nonzero", cfgs=CFGS)


def test_exact_overflow_probe_bit_for_bit(gpu):
    x, A, B, base, y_want, v_want = overflow_case()
    M = x.shape[0]
    call = _Call(gpu, M, A, B, base, "f16")
    x, y_want, v_want = x.to(gpu), y_want.to(gpu), v_want.to(gpu)
    for cfg in CFGS:
        for mode in ("null", "inplace", "separate"):
            y = call.run(x, mode, cfg, gpu)
            want = v_want if mode == "null" else y_want
            ok = same_bits_or_nan(y, want)
            assert bool(ok.all()), (f"{mode} cfg={cfg}: {int((~ok).sum())} of {ok.numel()} outputs differ from the header's chain "
                                    f"({int(torch.isnan(y).sum())} NaN, {int(torch.isinf(y).sum())} inf; due "
                                    f"{int(torch.isnan(want).sum())} NaN, {int(torch.isinf(want).sum())} inf)")
