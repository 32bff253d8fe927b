"""The HIP quantizer on the GPU (``-m gpu``) against the Python quantizer, bit for bit.

Expected values: ``bnb_layout.quantize_nf4`` / ``quantize_blockwise_8bit`` on host tensors
(tests/_quant_cases.py); every comparison is exact, the nested offset being the rounded fp64
mean or an fp32 neighbour.  Sizes walk the streaming kernel's tile and workgroup edges and
the second-level block edges; value cases put quotients on both sides of every decision
threshold; the alignment cases drive the general kernel through the C ABI inside guard bands.
"""
import numpy as np
import pytest
import torch

import nf4_oracle as O
from _helpers import assert_bits_equal, out_bits

import _quant_cases as Q

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024
PAT = 0xA5


class Guarded:
    """``nbytes`` usable bytes at byte ``shift`` past a 256-byte aligned start, between two
    guard bands of a fixed pattern (the pattern of test_gpu_redzones.py)."""

    def __init__(self, nbytes, device, fill=PAT, shift=0):
        self.n, self.off = int(nbytes), GUARD + int(shift)
        self.buf = torch.full((2 * GUARD + max(self.n, 1) + shift,), PAT, dtype=torch.uint8, device=device)
        if fill != PAT:
            self.buf[self.off:self.off + self.n].fill_(fill)

    @classmethod
    def of(cls, arr: np.ndarray, device, shift=0):
        g = cls(arr.nbytes, device, shift=shift)
        if arr.nbytes:
            g.buf[g.off:g.off + g.n].copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8)))
        return g

    def body(self, dtype=torch.uint8):
        b = self.buf[self.off:self.off + self.n]
        return b.view(dtype) if dtype == torch.uint8 or self.off % 4 == 0 else b.clone().view(dtype)

    def ptr(self):
        return self.buf.data_ptr() + self.off

    def bands_intact(self):
        return bool((self.buf[:self.off] == PAT).all()) and bool((self.buf[self.off + self.n:] == PAT).all())


def _both(w_host, bs, gpu):
    from nf4_triton_dequantization_amd import nf4_quantize

    want = Q.expect_single(w_host, bs)
    w = w_host.to(gpu)
    packed, qs = nf4_quantize(w, blocksize=bs, compress_statistics=False)
    assert packed.shape == ((w.numel() + 1) // 2, 1) and packed.dtype == torch.uint8 and packed.device == w.device
    Q.check_state(qs, w, bs, nested=False)
    Q.check_single(packed, qs.absmax, want)
    packed, qs = nf4_quantize(w, blocksize=bs, compress_statistics=True)
    Q.check_state(qs, w, bs, nested=True)
    o = Q.check_nested(packed, qs.absmax, qs.state2.absmax, qs.offset, want)
    _, qs2 = nf4_quantize(w, blocksize=bs, compress_statistics=True)
    assert np.float32(qs2.offset.item()).tobytes() == o.tobytes()   # two calls: the same bits
    assert torch.equal(w.cpu(), w_host)                             # the input is only read


@pytest.mark.parametrize("dt", list(Q.DTYPES))
@pytest.mark.parametrize("numel,bs", Q.SIZE_CASES)
def test_sizes(gpu, numel, bs, dt):
    _both(Q.normal_weight(numel, dt), bs, gpu)


@pytest.mark.parametrize("name,dt", Q.VALUE_CASES)
def test_values(gpu, name, dt):
    _both(Q.value_weight(name, dt), 64, gpu)


@pytest.mark.parametrize("dt", list(Q.DTYPES))
def test_boundary_at_larger_blocks(gpu, dt):
    _both(Q.boundary_weight(dt), 256, gpu)


@pytest.mark.parametrize("dt", list(Q.DTYPES))
@pytest.mark.parametrize("shift", [1, 3])
def test_input_views_with_a_storage_offset(gpu, dt, shift):
    """A weight that starts 1 or 3 elements into its storage is not 16-byte aligned: the
    general kernel, same bits.  The threshold-straddling values go through it too."""
    from nf4_triton_dequantization_amd import nf4_quantize

    for w_host in (Q.normal_weight(64 * 257 + 5, dt, seed=2), Q.boundary_weight(dt), Q.bucket_weight(dt)):
        store = torch.zeros(w_host.numel() + 8, dtype=w_host.dtype, device=gpu)
        w = store[shift:shift + w_host.numel()]
        w.copy_(w_host)
        assert w.storage_offset() == shift and w.data_ptr() % 16 != 0
        want = Q.expect_single(w_host, 64)
        packed, qs = nf4_quantize(w, compress_statistics=False)
        Q.check_single(packed, qs.absmax, want)
        packed, qs = nf4_quantize(w, compress_statistics=True)
        Q.check_nested(packed, qs.absmax, qs.state2.absmax, qs.offset, want)


DT_CODE = {"f16": O.F16, "bf16": O.BF16, "f32": O.F32}


@pytest.mark.parametrize("dt", list(Q.DTYPES))
@pytest.mark.parametrize("pshift", [0, 1, 2])
def test_c_abi_inside_guard_bands(gpu, dt, pshift):
    """Both entries with every buffer between guard bands, `packed` at byte offsets 0 (the
    streaming kernel), 1 and 2 (the general one): bands and inputs intact afterwards, nothing
    written outside the outputs, outputs exact.  Ragged sizes, where range handling matters."""
    from nf4_triton_dequantization_amd import _lib
    from nf4_triton_dequantization_amd.bnb_layout import dynamic_map

    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    code2 = dynamic_map().numpy()
    gc = Guarded.of(code2, gpu)
    for numel, bs in ((1, 64), (65, 64), (Q.TILE + 1, 64), (Q.WG_ELEMS + 63, 64), (64 * 257 + 3, 64), (8193, 128),
                      (5000, 4096)):
        w_host = Q.normal_weight(numel, dt, seed=3)
        want = Q.expect_single(w_host, bs)
        wbits = Q.tensor_bits(w_host, dt)
        nblk, plen = -(-numel // bs), (numel + 1) // 2
        gw = Guarded.of(wbits, gpu)
        gp = Guarded(plen, gpu, fill=0x5A, shift=pshift)
        ga = Guarded(4 * nblk, gpu, fill=0x5A)
        rc = L.nf4_quant_bnb(gw.ptr(), DT_CODE[dt], numel, bs, gp.ptr(), ga.ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0, _lib.strerror(rc)
        assert gp.bands_intact() and ga.bands_intact(), f"write outside an output, numel {numel} bs {bs}"
        Q.check_single(gp.body(), ga.body(torch.float32), want)
        wsz = L.nf4_quant_workspace_bytes(numel, bs)
        gp2 = Guarded(plen, gpu, fill=0x5A, shift=pshift)
        gq, g2, go = Guarded(nblk, gpu, fill=0x5A), Guarded(4 * (-(-nblk // 256)), gpu, fill=0x5A), Guarded(4, gpu)
        gws = Guarded(wsz, gpu, fill=0x5A)
        rc = L.nf4_quant_bnb_nested(gw.ptr(), DT_CODE[dt], numel, bs, gc.ptr(), 256, gp2.ptr(), gq.ptr(), g2.ptr(),
                                    go.ptr(), gws.ptr(), wsz, stream)
        torch.cuda.synchronize()
        assert rc == 0, _lib.strerror(rc)
        for g, what in ((gp2, "packed"), (gq, "absmax_q"), (g2, "absmax2"), (go, "offset"), (gws, "workspace")):
            assert g.bands_intact(), f"write outside {what}, numel {numel} bs {bs}"
        Q.check_nested(gp2.body(), gq.body(), g2.body(torch.float32), go.body(torch.float32)[0], want)
        for g, arr in ((gw, wbits), (gc, code2)):
            assert g.bands_intact(), "guard band of an input overwritten"
            assert np.array_equal(g.body().cpu().numpy(), np.ascontiguousarray(arr).reshape(-1).view(np.uint8)), \
                "input modified"


def test_graph_capture(gpu):
    """The nested call is three launches on the current stream with no host synchronisation:
    it captures (a synchronisation would fail the capture) and a replay quantizes whatever
    the static input then holds."""
    from nf4_triton_dequantization_amd import nf4_quantize

    numel = 64 * 300 + 6
    first, second = Q.normal_weight(numel, "bf16", seed=20), Q.normal_weight(numel, "bf16", seed=21)
    w_static = first.to(gpu)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        nf4_quantize(w_static)  # warm-up: loads the library, caches the code books on the device
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        packed, qs = nf4_quantize(w_static)
    for contents in (first, second):
        w_static.copy_(contents.to(gpu))
        graph.replay()
        torch.cuda.synchronize()
        Q.check_nested(packed, qs.absmax, qs.state2.absmax, qs.offset, Q.expect_single(contents, 64))


def test_memory_of_one_call(gpu):
    """A 2048x2048 bf16 weight: the call's own buffers are ~2.3 MiB (packed 2 MiB, fp32 absmax
    256 KiB in the workspace, absmax_q 64 KiB); the torch-op quantizer needs > 48 MiB for its
    fp32 copy and int64 indices alone."""
    from nf4_triton_dequantization_amd import nf4_quantize

    w = Q.normal_weight(2048 * 2048, "bf16", seed=30).to(gpu).view(2048, 2048)
    out = nf4_quantize(w)  # library loaded, code books cached
    del out
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    out = nf4_quantize(w)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(gpu) - base
    print(f"peak rise of one nested call: {rise / 2 ** 20:.2f} MiB")
    assert rise <= 8 * 2 ** 20, rise
    assert out[0].shape == (2048 * 2048 // 2, 1)


def test_round_trip_module(coracle, gpu, tmp_path):
    """Linear4bit.from_float -> dequantize_nf4_bnb equals the C oracle's dequant_bnb of the
    same packed data and statistics; the module saves and loads like a constructor-built one;
    nf4_linear accepts it."""
    from nf4_triton_dequantization_amd import (Linear4bit, dequantize_nf4_bnb, load_nf4_safetensors, nf4_linear,
                                               save_nf4_safetensors)

    torch.manual_seed(12)
    lin = torch.nn.Linear(1024, 192, bias=True).to(torch.bfloat16).to(gpu)
    mod = Linear4bit.from_float(lin)
    qs = mod.weight.quant_state
    assert (mod.out_features, mod.in_features) == (192, 1024) and qs.dtype == torch.bfloat16
    assert torch.equal(mod.bias.data, lin.bias.data)
    Q.check_nested(mod.weight.data, qs.absmax, qs.state2.absmax, qs.offset,
                   Q.expect_single(lin.weight.detach().cpu(), 64))

    def oracle(m):
        q = m.weight.quant_state
        return coracle.dequant_bnb(m.weight.data.cpu().numpy().reshape(-1), q.absmax.cpu().numpy(),
                                   q.state2.code.cpu().numpy(), q.state2.absmax.cpu().numpy(), float(q.offset),
                                   192 * 1024, O.BF16, 64, 256).reshape(192, 1024)

    got = dequantize_nf4_bnb(mod)
    assert_bits_equal(out_bits(got), oracle(mod), "bf16", "from_float -> dequantize_nf4_bnb")
    path = str(tmp_path / "m.safetensors")
    save_nf4_safetensors(path, {"l.weight": (mod.weight.data, qs)})
    back = load_nf4_safetensors(path, device=gpu)["l"]
    assert torch.equal(back.weight.data, mod.weight.data)
    assert_bits_equal(out_bits(dequantize_nf4_bnb(back)), oracle(mod), "bf16", "checkpoint round trip")
    x = torch.randn(3, 1024, device=gpu).to(torch.bfloat16)
    y = nf4_linear(x, mod)
    torch.cuda.synchronize()
    assert y.shape == (3, 192) and y.dtype == torch.bfloat16 and bool(torch.isfinite(y).all())
    assert mod(x).shape == (3, 192)
