"""Special activation rows across a row-block edge of nf4_gemm_bnb_moe_rb on the GPU (``-m gpu``):
NaN, infinities, zero rows, fp16 subnormals, rows that overflow the fp16 output and bf16 rows of
extreme magnitude (tests/_activation_cases.py builds them and test_activation_cases_cpu.py proves the
checks and this case's routing on the host).

The stack is the expert GEMM's of test_gpu_gemm_activations.py (E = 4, N = 192, K = 768, sensitive
weights).  300 pairs over 150 tokens (x_div 2) under ``_activation_cases.moe_rb_routing``: expert 1
has 159 pairs -- a full row block and one of 31 rows -- and the special tokens own entries 127 and
128 of its ascending pair list (the last staged row of block 0 and the first of block 1, in the
middle of a ballot round), its last entry (a partly filled row tile of the last block, rows past it
zero-filled in LDS), pair 0 and pair P - 1.  One special token also owns a pair with an invalid id.

Every call has a NaN-prefilled output and is made twice, on the matrix with the special rows and on
the plain draw it was made from.  Each expert's rows are judged with ``judge`` against the float64
reference by class and value; rows of invalid ids are zero bits even when the token row is NaN or
Inf; ``isolated`` demands over all 300 rows that every plain pair has the same bits in both calls.
After every call the workspace is all zero and nf4_gemm_check_workspace is clean.  The library's
choice and (2, 3): three K slices through the slab and the slice-order reducer.

The finite kinds (zero, negzero, tiny / small, huge) run before the non-finite ones."""
import numpy as np
import pytest

import _activation_cases as A
import test_gpu_gemm_moe as MOE
import test_gpu_gemm_moe_rb as RB
from test_gpu_gemm_activations import _bits, _dev

pytestmark = pytest.mark.gpu


def _run(coracle, gpu, dt, which):
    E, N, K, P, x_div = A.MOE["E"], A.MOE["N"], A.MOE["K"], A.MOE_RB["P"], A.MOE_RB["x_div"]
    S = MOE._stack(coracle, gpu, "nested", "sensitive", E, N, K, dt)
    ids, tokens = A.moe_rb_routing()
    T = P // x_div
    tok = np.arange(P) // x_div
    valid = (ids >= 0) & (ids < E)
    shares = []
    for kinds in A.kind_sets(T, dt, which):
        for at in A.moe_rb_passes(kinds, tokens):
            xs, base, rows = A.special_x(T, K, dt, A.x_seed(T, K), kinds, S.bits, at=at)
            pair_rows = {p: rows[tok[p]] for p in range(P) if tok[p] in rows}
            assert any(not valid[p] for p in pair_rows) or at != tokens, "no invalid id on a special token"
            xd, bd = _dev(xs, dt, gpu), _dev(base, dt, gpu)
            refs = {}
            for cfg in (None, RB._cfg(2, 3)):
                tag = f"moe_rb {dt} cfg {RB._tag(cfg)} rows {rows}"
                # (RB._rb: a fresh zeroed workspace per call, checked clean and all zero afterwards)
                yb, ys = _bits(RB._rb(S, bd, ids, x_div, cfg)), _bits(RB._rb(S, xd, ids, x_div, cfg))
                assert (ys[~valid] == 0).all() and (yb[~valid] == 0).all(), f"{tag}: rows of invalid ids are not zero bits"
                for e in range(E):
                    sel = np.nonzero(ids == e)[0]
                    if e not in refs:
                        refs[e] = A.reference(xs[tok[sel]], S.bits[e], dt)
                    sel_rows = {i: pair_rows[p] for i, p in enumerate(sel) if p in pair_rows}
                    shares.append(A.judge(ys[sel], xs[tok[sel]], S.bits[e], dt, f"{tag} expert {e}", rows=sel_rows, ref=refs[e]))
                A.isolated(ys, yb, pair_rows, tag)
    print(f"moe_rb {dt} {which}: borderline share at most {max(shares):.3%}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_finite_rows_across_a_row_block_edge(coracle, gpu, dt):
    _run(coracle, gpu, dt, "finite")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_nonfinite_rows_across_a_row_block_edge(coracle, gpu, dt):
    _run(coracle, gpu, dt, "nonfinite")
