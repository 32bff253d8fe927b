"""Guard-band checks of the bitsandbytes-semantics GEMM entries on the GPU (``-m gpu``):
nf4_gemm_bnb and nf4_gemm_bnb_single with every buffer they are handed -- x, the packed
weight, the statistics, code2, the offset, y, the workspace -- carved out of a larger
allocation with 64 KiB bands of a fixed byte pattern on both sides (the method of
test_gpu_redzones.py).  After each call: every band intact, the inputs unchanged, the output
within the GEMM tolerance of the float64 oracle, the workspace all zero."""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_bnb_cases import drawn_weight_bnb, single_weight_bnb
from _gemm_cases import bits_to_f64, check_close, gemm_oracle, x_bits

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024
PAT = 0xA5
N, K = 128, 1024


class Guarded:
    """``nbytes`` usable bytes between two guard bands (offset 64 KiB: 256-B aligned)."""

    def __init__(self, nbytes, device, fill=PAT):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + max(self.n, 1),), PAT, dtype=torch.uint8, device=device)
        if fill != PAT:
            self.buf[GUARD:GUARD + self.n].fill_(fill)

    @classmethod
    def of(cls, arr, device):
        arr = np.ascontiguousarray(arr)
        g = cls(arr.nbytes, device)
        g.src = arr.reshape(-1).view(np.uint8).copy()
        g.buf[GUARD:GUARD + g.n].copy_(torch.from_numpy(g.src))
        return g

    def body(self, dtype=torch.uint8):
        return self.buf[GUARD:GUARD + self.n].view(dtype)

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def bands_intact(self):
        return bool((self.buf[:GUARD] == PAT).all()) and bool((self.buf[GUARD + self.n:] == PAT).all())

    def unchanged(self):
        return np.array_equal(self.body().cpu().numpy(), self.src)


def _check(L, rc, inputs, y, ws, wsz, ref, bound, dt, what):
    from nf4_triton_dequantization_amd import _lib

    torch.cuda.synchronize()
    assert rc == 0, (what, _lib.strerror(rc))
    for name, g in inputs.items():
        assert g.bands_intact(), f"{what}: band of {name} overwritten"
        assert g.unchanged(), f"{what}: {name} modified"
    assert y.bands_intact(), f"{what}: write outside y"
    assert ws.bands_intact(), f"{what}: write outside the workspace"
    sp = torch.cuda.current_stream().cuda_stream
    assert L.nf4_gemm_check_workspace(ws.ptr() if wsz else None, wsz, sp) == 0, what
    assert int(ws.body().count_nonzero()) == 0, f"{what}: workspace not all zero"
    yb = y.body(torch.int16).cpu().numpy().view(np.uint16).reshape(ref.shape)
    check_close(bits_to_f64(yb, dt), ref, bound, what)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 8, 32])
def test_gemm_bnb_between_guard_bands(coracle, gpu, dt, M):
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    code = _lib.BF16 if dt == "bf16" else _lib.F16
    ocode = O.BF16 if dt == "bf16" else O.F16
    sp = torch.cuda.current_stream().cuda_stream
    _, xb = x_bits(M, K, dt, seed=40 + M)
    wsz = L.nf4_gemm_bnb_workspace_bytes(M, N, K, None)

    packed, a1, code2, a2, offset = drawn_weight_bnb(N, K, seed=50 + M)
    wb = coracle.dequant_bnb(packed, a1, code2, a2, offset, N * K, ocode, 64, 256).reshape(N, K)
    ref, bound = gemm_oracle(xb, wb, dt)
    g = {"x": Guarded.of(xb, gpu), "packed": Guarded.of(packed, gpu), "absmax_q": Guarded.of(a1, gpu),
         "code2": Guarded.of(code2, gpu), "absmax2": Guarded.of(a2, gpu),
         "offset": Guarded.of(np.array([offset], np.float32), gpu)}
    y, ws = Guarded(M * N * 2, gpu, fill=0x5A), Guarded(wsz, gpu, fill=0)
    rc = L.nf4_gemm_bnb(g["x"].ptr(), M, g["packed"].ptr(), packed.size, g["absmax_q"].ptr(), a1.size,
                        g["code2"].ptr(), g["absmax2"].ptr(), a2.size, g["offset"].ptr(), 64, 256, y.ptr(), code, N, K,
                        ws.ptr() if wsz else None, wsz, None, sp)
    _check(L, rc, g, y, ws, wsz, ref, bound, dt, f"nested M={M} {dt}")

    packed, absmax = single_weight_bnb(N, K, seed=60 + M)
    wb = coracle.dequant_bnb_single(packed, absmax, N * K, ocode, 64).reshape(N, K)
    ref, bound = gemm_oracle(xb, wb, dt)
    g = {"x": Guarded.of(xb, gpu), "packed": Guarded.of(packed, gpu), "absmax": Guarded.of(absmax, gpu)}
    y, ws = Guarded(M * N * 2, gpu, fill=0x5A), Guarded(wsz, gpu, fill=0)
    rc = L.nf4_gemm_bnb_single(g["x"].ptr(), M, g["packed"].ptr(), packed.size, g["absmax"].ptr(), absmax.size, 64,
                               y.ptr(), code, N, K, ws.ptr() if wsz else None, wsz, None, sp)
    _check(L, rc, g, y, ws, wsz, ref, bound, dt, f"single M={M} {dt}")
