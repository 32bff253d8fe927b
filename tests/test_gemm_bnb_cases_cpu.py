"""tests/_gemm_bnb_cases.py checked on the host, on the oracle alone: the sensitive bnb weight
is a real nested weight, and in at least 32 of its 64-blocks each near-miss restatement of
the scale (a fused multiply-add; a single rounding of the last product) gives another
16-bit weight than oracle/nf4_oracle.py::dequant_bnb_np -- so an exact-weight walk through
the fused GEMM (test_gpu_gemm_bnb.py) can tell them apart.  The fused scale is judged with
rational arithmetic, the single rounding with float64 (the product of two fp32 values is
exact there)."""
import numpy as np
import pytest

import nf4_oracle as O
from _gemm_bnb_cases import (BLOCKSIZE2, KINDS_BNB, OFFSET, bnb_scale, f32_rne, fma_scale_exact,
                             sensitive_weight_bnb)
from _gemm_cases import bits_to_f64, single_rounding_bits, weight_bits

N, K = 128, 1024


def test_f32_rne_rounds_rationals_to_nearest_even():
    from fractions import Fraction

    one = Fraction(1)
    ulp = Fraction(1, 1 << 23)
    assert f32_rne(one + ulp / 2) == np.float32(1.0)                      # tie: to even
    assert f32_rne(one + ulp * 3 / 2) == np.float32(1.0) + np.float32(2.0 ** -22)  # tie: to even (up)
    assert f32_rne(one + ulp / 2 + Fraction(1, 1 << 80)) == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert f32_rne(-Fraction(1, 3)) == np.float32(-1.0 / 3.0)
    assert f32_rne(Fraction(1, 1 << 149)) == np.float32(2.0 ** -149)
    assert f32_rne(Fraction(0)) == 0.0


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_sensitive_weight_is_a_real_nested_weight(dt):
    packed, a1, code2, a2, offset, kinds = sensitive_weight_bnb(N, K, dt)
    nblk = N * K // 64
    assert packed.shape == (N * K // 2,) and a1.shape == (nblk,) and code2.shape == (256,)
    assert a2.shape == (nblk // BLOCKSIZE2,) == (128,)
    assert (a2 > 0).all() and offset == float(OFFSET) != 0.0
    assert (np.bincount(kinds[kinds >= 0]) == 64).all()  # one block per nested group, the kinds in turn
    bits = O.dequant_bnb_np(packed, a1, code2, a2, offset, N * K, O.BF16 if dt == "bf16" else O.F16, 64, BLOCKSIZE2)
    w = bits_to_f64(bits, dt)
    assert np.isfinite(w).all() and np.abs(w).max() < 256.0


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_each_near_miss_differs_in_at_least_32_blocks(dt):
    packed, a1, code2, a2, offset, kinds = sensitive_weight_bnb(N, K, dt)
    nblk = N * K // 64
    dt_code = O.BF16 if dt == "bf16" else O.F16
    want = O.dequant_bnb_np(packed, a1, code2, a2, offset, N * K, dt_code, 64, BLOCKSIZE2).reshape(nblk, 64)
    nib = np.empty(N * K, np.uint8)
    nib[0::2], nib[1::2] = packed >> 4, packed & 0xF
    codes = nib.reshape(nblk, 64).astype(np.int64)
    c2 = code2[a1]
    a2b = np.repeat(a2, BLOCKSIZE2)
    s = bnb_scale(c2, a2b, offset)
    assert (weight_bits(s[:, None], codes, dt) == want).all()  # this module's formula is the oracle's
    restated = {
        "fma_scale": weight_bits(fma_scale_exact(c2, a2b, offset)[:, None], codes, dt),
        "single_rounding": single_rounding_bits(np.repeat(s[:, None], 64, axis=1), codes, dt),
    }
    for k, kind in enumerate(KINDS_BNB):
        differ = (restated[kind] != want).any(axis=1)
        aimed = kinds == k
        print(f"{dt} {kind}: {int(differ.sum())} blocks differ, {int((differ & aimed).sum())} of {int(aimed.sum())} aimed")
        assert int((differ & aimed).sum()) >= 32, (kind, int((differ & aimed).sum()))
