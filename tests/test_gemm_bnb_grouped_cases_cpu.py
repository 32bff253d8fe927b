"""tests/_gemm_bnb_grouped_cases.py checked on the host, on the oracle alone: the three nested
weights of a group differ in offset, code2 and blocksize2, every oracle weight is finite, and
dequantizing any of them with another weight's code2, offset or blocksize2 -- or with its flat
block index starting at the launch-wide row instead of 0 -- changes the oracle's 16-bit output
in at least one element of EVERY 16-row strip.  That is a condition on the inputs (no
tolerance): with it, the exact identity walks of test_gpu_gemm_bnb_grouped.py tell a grouped
kernel that shares any of these between weights from a right one, whichever strip a workgroup
took."""
import numpy as np
import pytest

import nf4_oracle as O
from _gemm_bnb_grouped_cases import BLOCKSIZE2S, OFFSETS, SMALL_NS, misread_bits, nested_group, offset_value
from _gemm_cases import bits_to_f64

SHAPES = [(SMALL_NS, 1024), (SMALL_NS, 2048)]


def _oracle(w, N, K, dt):
    packed, a1, code2, a2, off, bs2 = w
    return O.dequant_bnb_np(packed, a1, code2, a2, offset_value(off), N * K, O.BF16 if dt == "bf16" else O.F16, 64, bs2)


def _strips_differ(a, b, N, K):
    """Per 16-row strip: whether any 16-bit weight differs."""
    return (a.reshape(N // 16, 16 * K) != b.reshape(N // 16, 16 * K)).any(axis=1)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Ns,K", SHAPES)
def test_group_is_three_real_and_different_nested_weights(Ns, K, dt):
    g = nested_group(Ns, K, dt)
    assert tuple(w[4] for w in g) == OFFSETS == (0.0123, 0.05, None)
    assert tuple(w[5] for w in g) == BLOCKSIZE2S == (256, 16, 4)
    dyn = g[0][2]
    assert np.array_equal(g[1][2], dyn) and np.array_equal(g[2][2], dyn[::-1]) and not np.array_equal(g[2][2], dyn)
    for w, N in zip(g, Ns):
        packed, a1, code2, a2, off, bs2 = w
        nblk = N * K // 64
        # statistics arrays of exactly the needed length
        assert packed.size == N * K // 2 and a1.size == nblk and a2.size == -(-nblk // bs2) and code2.size == 256
        assert np.isfinite(code2).all() and np.isfinite(a2).all()
        bits = _oracle(w, N, K, dt)
        assert np.isfinite(bits_to_f64(bits, dt)).all()  # every oracle weight is finite
        assert np.array_equal(misread_bits(w, dt).reshape(-1), bits.reshape(-1))  # the restatement's base IS the oracle


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Ns,K", SHAPES)
def test_another_weights_code2_offset_or_blocksize2_changes_every_strip(Ns, K, dt):
    g = nested_group(Ns, K, dt)
    told = {"code2": 0, "offset": 0, "blocksize2": 0}
    for i, (w, N) in enumerate(zip(g, Ns)):
        want = _oracle(w, N, K, dt)
        for j, o in enumerate(g):
            if j == i:
                continue
            variants = {}
            if not np.array_equal(o[2], w[2]):
                variants["code2"] = misread_bits(w, dt, code2=o[2])
            if o[4] != w[4]:
                variants["offset"] = misread_bits(w, dt, offset=o[4])
            if o[5] != w[5]:
                variants["blocksize2"] = misread_bits(w, dt, blocksize2=o[5])
            assert "offset" in variants and "blocksize2" in variants  # all three differ in these
            for name, bits in variants.items():
                d = _strips_differ(bits, want, N, K)
                assert d.all(), f"weight {i} with weight {j}'s {name}: strips {np.flatnonzero(~d)[:8]} unchanged"
                told[name] += 1
    assert told == {"code2": 4, "offset": 6, "blocksize2": 6}, told  # code2: every pair with weight 2


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Ns,K", SHAPES)
def test_launch_wide_block_index_changes_every_strip(Ns, K, dt):
    g = nested_group(Ns, K, dt)
    row0 = 0
    for i, (w, N) in enumerate(zip(g, Ns)):
        if row0:
            bits = misread_bits(w, dt, first_block=row0 * (K // 64))
            d = _strips_differ(bits, _oracle(w, N, K, dt), N, K)
            assert d.all(), f"weight {i} numbered from launch row {row0}: strips {np.flatnonzero(~d)[:8]} unchanged"
        row0 += N
    assert row0 == sum(Ns)
