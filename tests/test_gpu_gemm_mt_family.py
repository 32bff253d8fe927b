"""Every instantiation of the row-tiled GEMM family once: the three entries (nf4_gemm_bnb_mt,
nf4_gemm_bnb_mt_swiglu, nf4_gemm_bnb_moe) are built from one device header (csrc/nf4_gemm_mt_dev.h),
instantiated per entry for dtype x mode x waves x row tiles -- 96 kernels.  The entries' own
modules reach most of them; this one reaches each, with one and with two K slices, and judges it
with its entry's own acceptance helper and bounds.

N (or I) = 128, K = 640: five chunks, so one slice wraps the four-slot weight ring once and two
slices get 3 + 2 chunks (both run past their end: clamped chunk numbers); ten 64-blocks per row,
so a blocksize2 = 256 boundary falls inside a row.  16 / 48 / 80 / 128 rows are 2 / 4 / 6 / 8 row
tiles.  The expert GEMM routes every pair to expert 1 but the last, which goes to expert 0: one
workgroup runs the largest instantiation with one live row tile, another with all of them live.
Every call checks its workspace clean and all zero afterwards (the modules' _call).
"""
import numpy as np
import pytest

import test_gpu_gemm_moe as MOE
import test_gpu_gemm_mt as MT
import test_gpu_gemm_mt_swiglu as SG
from _gemm_cases import check_gemm

pytestmark = pytest.mark.gpu

N, K = 128, 640


def _run_mt(coracle, gpu, dt, mode, waves, rows, ksplit, what):
    W = MT._weight(coracle, gpu, mode, "drawn", N, K, dt)
    xt, xb = MT._x(rows, K, dt)
    check_gemm(MT._gemm(W, xt.to(gpu), rows, MT._cfg(waves, ksplit)), xb, W.bits, dt, what)


def _run_swiglu(coracle, gpu, dt, mode, waves, rows, ksplit, what):
    G, U = SG._pair(coracle, gpu, mode, N, K, dt)
    xt, xb = SG._x(rows, K, dt)
    SG._check_chain(SG._swiglu(G, U, xt.to(gpu), rows, SG._cfg(waves, ksplit)), xb, G, U, dt, what)


def _run_moe(coracle, gpu, dt, mode, waves, rows, ksplit, what):
    S = MOE._stack(coracle, gpu, mode, "drawn", 2, N, K, dt)
    ids = np.ones(rows, np.int32)
    ids[-1] = 0
    xt, xb = MOE._x(rows, K, dt)
    MOE._check(S, MOE._moe(S, xt.to(gpu), ids, 1, MOE._cfg(waves, ksplit)), xb, ids, 1, what)


_RUN = {"mt": _run_mt, "swiglu": _run_swiglu, "moe": _run_moe}


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("rows", [16, 48, 80, 128])
@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("entry", ["mt", "swiglu", "moe"])
def test_every_instantiation(coracle, gpu, entry, dt, mode, waves, rows, ksplit):
    _RUN[entry](coracle, gpu, dt, mode, waves, rows, ksplit, f"{entry} {dt} {mode} waves={waves} rows={rows} ksplit={ksplit}")
