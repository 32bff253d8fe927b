"""The fused GEMM as a dequantizer: exact weights, element for element (``-m gpu``).

Every GEMM family documents that it multiplies x by the bit-exact weights
nf4_dequant_ref would write (fp32 code x scale, IEEE q / 127, RNE to 16 bits).  The
float64 oracle of test_gpu_gemm.py cannot see a weight one 16-bit ulp off; this suite can.

Method.  With x = rows k0 .. k0+M-1 of the K x K identity, every output is one weight plus
exact zeros, y[m][n] = W[n][k0 + m] -- on the VALU, through MFMA, through split-K partial
sums and through the final rounding (the sum of one 16-bit value and zeros is that value).
Walking k0 over K recovers the whole dequantized matrix, K / M launches of a few
microseconds each (the last window starts at K - M when M does not divide K).  It is
compared with the C oracle's output BY VALUE WITH NO TOLERANCE: -0 == +0 is allowed (a zero
partial sum may lose the sign), NaN never.  The identity and the recovered matrix stay on
the device; one comparison per configuration.

Weights: the sensitive weight of tests/_gemm_cases.py (its 64-blocks sit where single
rounding, q * (1/127) and (q * a2) / 127 each give another 16-bit value;
test_gemm_cases_cpu.py proves that on the reference alone) and one ordinary drawn weight.
"""
import ctypes

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_cases import GEMV_FORMS, bits_to_f64, cfg_tuple, gemm_cfgs, sensitive_weight
from _helpers import make_module

pytestmark = pytest.mark.gpu

FAMILY = {1: "STREAM", 2: "K128", 3: "PERSIST", 4: "XS", 5: "XR", 7: "GEMV"}


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _weight(kind, N, K, dt, seed=0):
    if kind == "sensitive":
        return sensitive_weight(N, K, dt)[:3]
    return O.make_inputs(N, K, seed=N + K + seed, a2_kind="normal")


def _want(coracle, inputs, N, K, dt, gpu):
    """The oracle's weights as a device tensor [N, K] of the 16-bit dtype; all finite
    (0 x inf in a dot product would not be exact)."""
    bits = coracle.dequant_ref(*inputs, N, K, O.BF16 if dt == "bf16" else O.F16)
    assert np.isfinite(bits_to_f64(bits, dt)).all()
    return torch.from_numpy(bits.view(np.int16)).to(gpu).view(_tdt(dt)), bits


def _starts(K, M):
    return [min(k0, K - M) for k0 in range(0, K, M)]


def _assemble(Y, starts, N, K, M):
    """Y [windows, M, N] -> the recovered W [N, K]."""
    rec = torch.empty((N, K), dtype=Y.dtype, device=Y.device)
    full = K // M
    rec[:, :full * M] = Y[:full].permute(2, 0, 1).reshape(N, full * M)
    if K % M:
        rec[:, K - M:] = Y[-1].t()
    return rec


def _assert_exact(rec, want, what):
    ok = rec == want  # by value: -0 == +0, NaN equal to nothing
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} weights differ "
                             f"({int(torch.isnan(rec.float()).sum())} NaN); first at row {r} column {c}: "
                             f"got {float(rec[r, c])!r} want {float(want[r, c])!r}; rows "
                             f"{sorted(set(bad[:, 0].tolist()))[:8]} columns {sorted(set(bad[:, 1].tolist()))[:8]}")


def _identity(K, dt, gpu):
    return torch.eye(K, dtype=_tdt(dt), device=gpu)


def _recover_cfg(L, _lib, eye, t, dt, N, K, M, cfg):
    """W recovered through nf4_gemm_ref_cfg with `cfg`, or None if the ABI rejects it
    (ERR_ARG); the split-K error word is read after the walk (it is sticky)."""
    starts = _starts(K, M)
    Y = torch.full((len(starts), M, N), float("nan"), dtype=eye.dtype, device=eye.device)
    wsz = L.nf4_gemm_workspace_bytes_cfg(M, N, K, ctypes.byref(cfg))
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=eye.device)
    sp = torch.cuda.current_stream().cuda_stream
    code = _lib.BF16 if dt == "bf16" else _lib.F16
    for i, k0 in enumerate(starts):
        rc = L.nf4_gemm_ref_cfg(eye.data_ptr() + k0 * K * 2, M, t[0].data_ptr(), t[0].numel(), t[1].data_ptr(),
                                t[1].numel(), t[2].data_ptr(), t[2].numel(), Y[i].data_ptr(), code, N, K,
                                ws.data_ptr() if wsz else None, wsz, ctypes.byref(cfg), sp)
        if rc == _lib.ERR_ARG and i == 0:
            return None
        assert rc == 0, (cfg_tuple(cfg), k0, _lib.strerror(rc))
    assert L.nf4_gemm_check_workspace(ws.data_ptr() if wsz else None, wsz, sp) == 0, cfg_tuple(cfg)
    if wsz:
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg_tuple(cfg)}"
    return _assemble(Y, starts, N, K, M)


def _recover_linear(eye, mod, N, K, M):
    from nf4_triton_dequantization_amd import nf4_linear

    starts = _starts(K, M)
    Y = torch.stack([nf4_linear(eye[k0:k0 + M], mod) for k0 in starts])
    return _assemble(Y, starts, N, K, M)


def _recover_grouped(eye, mods, Ns, K, M):
    from nf4_triton_dequantization_amd import nf4_linear_grouped

    starts = _starts(K, M)
    outs = [nf4_linear_grouped(eye[k0:k0 + M], mods) for k0 in starts]
    return [_assemble(torch.stack([o[i] for o in outs]), starts, N, K, M) for i, N in enumerate(Ns)]


def _dev(inputs, gpu):
    return tuple(torch.from_numpy(v).to(gpu) for v in inputs)


# ---- explicit configurations ----------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sensitive", "normal"])
@pytest.mark.parametrize("M", [32, 5])
def test_every_decomposition_recovers_exact_weights(coracle, gpu, dt, kind, M):
    """N = 128, K = 1024: every entry of the shared decomposition list.  M = 32 runs STREAM,
    K128, XS and XR; the persistent kernel takes at most 16 rows at any shape, so it runs
    (with the other four again) at M = 5, whose last window overlaps (1024 = 204 x 5 + 4)."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 128, 1024
    inputs = _weight(kind, N, K, dt)
    want, _ = _want(coracle, inputs, N, K, dt, gpu)
    t = _dev(inputs, gpu)
    eye = _identity(K, dt, gpu)
    ran = {}
    for cfg in gemm_cfgs(K, M):
        rec = _recover_cfg(L, _lib, eye, t, dt, N, K, M, cfg)
        if rec is None:
            continue
        _assert_exact(rec, want, f"{FAMILY[cfg.kernel]} cfg {cfg_tuple(cfg)} M={M} {dt} {kind}")
        ran[FAMILY[cfg.kernel]] = ran.get(FAMILY[cfg.kernel], 0) + 1
    print(f"exact {dt} {kind} M={M}: configurations run {ran}")
    for fam in ("STREAM", "K128", "XS", "XR") + (("PERSIST",) if M <= 16 else ()):
        assert ran.get(fam, 0) >= 1, (fam, ran)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sensitive", "normal"])
@pytest.mark.parametrize("N,K,forms", [(64, 2048, GEMV_FORMS), (128, 4096, [(16, 1), (8, 4)])])
def test_gemv_recovers_exact_weights(coracle, gpu, dt, kind, N, K, forms):
    """The decode GEMV at M = 1: one piece of 2048 columns per row, and two."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    inputs = _weight(kind, N, K, dt)
    want, _ = _want(coracle, inputs, N, K, dt, gpu)
    t = _dev(inputs, gpu)
    eye = _identity(K, dt, gpu)
    for waves, rows in forms:
        cfg = _lib.GemmCfg(_lib.GEMM_GEMV, waves, rows, 1, 0)
        rec = _recover_cfg(L, _lib, eye, t, dt, N, K, 1, cfg)
        assert rec is not None, (waves, rows)
        _assert_exact(rec, want, f"GEMV ({waves}, {rows}) {N}x{K} {dt} {kind}")


# ---- the library's choice -------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sensitive", "normal"])
@pytest.mark.parametrize("N,K,M", [(128, 2048, 1), (128, 2048, 8), (128, 2048, 12), (2048, 1024, 17),
                                   (2048, 1024, 32)])
def test_library_choice_recovers_exact_weights(coracle, gpu, dt, kind, N, K, M):
    """nf4_linear: the GEMV (M = 1), the persistent kernel (8), its K slices or the
    register-resident kernel (12), the register-resident default (17, 32)."""
    inputs = _weight(kind, N, K, dt)
    want, _ = _want(coracle, inputs, N, K, dt, gpu)
    mod = make_module(*inputs, N, K, dt, gpu)
    rec = _recover_linear(_identity(K, dt, gpu), mod, N, K, M)
    _assert_exact(rec, want, f"nf4_linear {N}x{K} M={M} {dt} {kind}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["sensitive", "normal"])
@pytest.mark.parametrize("M", [1, 4])
def test_grouped_recovers_exact_weights(coracle, gpu, dt, kind, M):
    """nf4_linear_grouped over three weights: the GEMV's multi-weight walk (M = 1) and the
    persistent kernel (M = 4)."""
    K, Ns = 2048, (64, 192, 64)
    ins = [_weight(kind, N, K, dt, seed=31 * i) for i, N in enumerate(Ns)]
    mods = [make_module(*inp, N, K, dt, gpu) for inp, N in zip(ins, Ns)]
    recs = _recover_grouped(_identity(K, dt, gpu), mods, Ns, K, M)
    for i, (rec, inp, N) in enumerate(zip(recs, ins, Ns)):
        want, _ = _want(coracle, inp, N, K, dt, gpu)
        _assert_exact(rec, want, f"grouped weight {i} ({N}x{K}) M={M} {dt} {kind}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 4])
def test_row_boundary_wrap_recovers_exact_weights(coracle, gpu, dt, M):
    """absmax of 5 rows' worth, nested absmax of 3 rows' worth (the reference's repeat wraps
    at row boundaries only): single and grouped, the GEMV (M = 1) and the persistent kernel
    (M = 4), both of which index a row's statistics from a per-row modulo."""
    K, Ns = 2048, (64, 192, 64)
    bpr, groups = K // 64, -(-(K // 64) // 4)
    ins = [O.golden_case_inputs(N, K, 80 + i, {"nb": 5 * bpr, "n2": 3 * groups, "a2_kind": "normal"})[:3]
           for i, N in enumerate(Ns)]
    mods = [make_module(*inp, N, K, dt, gpu) for inp, N in zip(ins, Ns)]
    eye = _identity(K, dt, gpu)
    wants = [_want(coracle, inp, N, K, dt, gpu)[0] for inp, N in zip(ins, Ns)]
    for i, rec in enumerate(_recover_grouped(eye, mods, Ns, K, M)):
        _assert_exact(rec, wants[i], f"grouped wrap weight {i} M={M} {dt}")
    _assert_exact(_recover_linear(eye, mods[1], Ns[1], K, M), wants[1], f"single wrap M={M} {dt}")


# ---- subnormal weights ----------------------------------------------------------------------
@pytest.mark.parametrize("dt,a2_scale", [("f16", 1e-5), ("bf16", 1e-39)])
@pytest.mark.parametrize("M", [1, 8])
def test_subnormal_weights_come_through_exactly(coracle, gpu, dt, a2_scale, M):
    """Weights in the 16-bit subnormal range through the library's choice: the GEMV's
    v_dot2c_f32_f16 / _bf16 (M = 1) and the persistent kernel's 16-bit MFMA operands
    (M = 8) must keep subnormal inputs, and the final rounding must keep subnormal outputs."""
    N, K = 64, 2048
    inputs = O.golden_case_inputs(N, K, 7, {"a2_kind": "uniform", "a2_scale": a2_scale})[:3]
    want, bits = _want(coracle, inputs, N, K, dt, gpu)
    exp = (bits & 0x7C00) if dt == "f16" else (bits & 0x7F80)
    sub = (exp == 0) & ((bits & 0x7FFF) != 0)
    print(f"subnormal {dt}: {sub.mean():.1%} of the weights subnormal, {((bits & 0x7FFF) == 0).mean():.1%} zero")
    assert sub.mean() > 0.5
    mod = make_module(*inputs, N, K, dt, gpu)
    rec = _recover_linear(_identity(K, dt, gpu), mod, N, K, M)
    _assert_exact(rec, want, f"subnormal weights, nf4_linear M={M} {dt}")


@pytest.mark.parametrize("dt,a2_scale", [("f16", 1e-5), ("bf16", 1e-39)])
def test_subnormal_weights_every_family(coracle, gpu, dt, a2_scale):
    """The same subnormal weights through explicit configurations, up to three per family
    at M = 1 (the GEMV among them), 8 (the persistent kernel among them) and 32: the record,
    per family, that neither the dot / MFMA operands nor the split-K sums nor the final
    rounding flush a 16-bit subnormal."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    N, K = 64, 2048
    inputs = O.golden_case_inputs(N, K, 7, {"a2_kind": "uniform", "a2_scale": a2_scale})[:3]
    want, _ = _want(coracle, inputs, N, K, dt, gpu)
    t = _dev(inputs, gpu)
    eye = _identity(K, dt, gpu)
    ran = {}
    for M in (1, 8, 32):
        seen = {}
        for cfg in gemm_cfgs(K, M):
            fam = FAMILY[cfg.kernel]
            if seen.get(fam, 0) >= 3:
                continue
            rec = _recover_cfg(L, _lib, eye, t, dt, N, K, M, cfg)
            if rec is None:
                continue
            seen[fam] = seen.get(fam, 0) + 1
            _assert_exact(rec, want, f"subnormal weights, {fam} cfg {cfg_tuple(cfg)} M={M} {dt}")
        for fam, n in seen.items():
            ran[fam] = ran.get(fam, 0) + n
    print(f"subnormal {dt}: configurations run {ran}")
    assert set(ran) == set(FAMILY.values()), ran
