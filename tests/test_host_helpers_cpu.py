"""The private helpers of kernel.py's host layer, on host tensors (no GPU, no native library):
``_rows`` (x as an entry reads it), ``_bnb_stats`` / ``_offset_ptr`` (the statistics operands in
bitsandbytes semantics), ``_ref_stats`` (reference semantics), ``_check_out`` and the cross-device
error.  They are plain tensor plumbing; every fused entry of the Python API goes through them."""
from types import SimpleNamespace

import pytest
import torch

from nf4_triton_dequantization_amd import kernel

CPU = torch.device("cpu")


def _at_byte_offset(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    """A copy of ``t`` whose storage starts ``nbytes`` bytes into a 64-byte-aligned buffer."""
    raw = torch.empty(t.numel() * t.element_size() + 128, dtype=torch.uint8)
    start = -raw.data_ptr() % 64 + nbytes
    view = raw[start:start + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 64 == nbytes
    return view


# ---------------------------------------------------------------- _rows
def test_rows_passes_a_row_major_matrix_of_the_dtype_through():
    x = _at_byte_offset(torch.randn(3, 8).to(torch.bfloat16), 0)
    for align16 in (False, True):
        xc = kernel._rows(x, 8, torch.bfloat16, align16)
        assert xc.data_ptr() == x.data_ptr() and xc.shape == (3, 8) and xc.dtype == torch.bfloat16


def test_rows_flattens_casts_and_makes_contiguous():
    x = torch.randn(2, 3, 8)
    xc = kernel._rows(x, 8, torch.float16, False)
    assert xc.shape == (6, 8) and xc.dtype == torch.float16 and xc.is_contiguous()
    assert torch.equal(xc, x.to(torch.float16).reshape(6, 8))
    t = torch.randn(8, 5).to(torch.bfloat16).t()  # [5, 8], column-major
    tc = kernel._rows(t, 8, torch.bfloat16, False)
    assert tc.is_contiguous() and tc.data_ptr() != t.data_ptr() and torch.equal(tc, t)


def test_rows_clones_a_misaligned_view_only_when_asked():
    x = _at_byte_offset(torch.randn(4, 8).to(torch.float16), 2)
    same = kernel._rows(x, 8, torch.float16, False)
    assert same.data_ptr() == x.data_ptr()
    moved = kernel._rows(x, 8, torch.float16, True)
    assert moved.data_ptr() != x.data_ptr() and moved.data_ptr() % 16 == 0 and torch.equal(moved, x)


def test_lead_rows():
    assert kernel._lead_rows(torch.empty(2, 3, 8), 8) == (torch.Size((2, 3)), 6)
    assert kernel._lead_rows(torch.empty(2, 0), 0) == (torch.Size((2,)), 0)


# ---------------------------------------------------------------- _bnb_stats
def _nested(code_dtype=torch.float32, a2_dtype=torch.float32, offset="tensor", entries=256):
    st2 = SimpleNamespace(absmax=torch.rand(3).to(a2_dtype), code=torch.linspace(-1, 1, entries).to(code_dtype),
                          blocksize=256)
    off = torch.tensor(0.25) if offset == "tensor" else offset
    return SimpleNamespace(absmax=torch.randint(0, 256, (12,), dtype=torch.uint8), state2=st2, offset=off, blocksize=64)


def test_bnb_stats_nested_passes_operands_of_the_entry_types_as_they_are():
    qs, keep = _nested(), []
    got = kernel._bnb_stats("caller", qs, CPU, keep)
    assert got == (qs.absmax.data_ptr(), 12, qs.state2.code.data_ptr(), qs.state2.absmax.data_ptr(), 3,
                   qs.offset.data_ptr(), 64, 256)
    assert keep == []  # nothing was made: the quant state holds every tensor


def test_bnb_stats_casts_fp16_code2_and_absmax2_and_keeps_the_casts():
    qs, keep = _nested(code_dtype=torch.float16, a2_dtype=torch.float16), []
    ap, an, cp, bp, bn, op, bs, bs2 = kernel._bnb_stats("caller", qs, CPU, keep)
    assert (ap, an, bn, op, bs, bs2) == (qs.absmax.data_ptr(), 12, 3, qs.offset.data_ptr(), 64, 256)
    assert len(keep) == 2 and all(t.dtype == torch.float32 for t in keep)
    assert (cp, bp) == (keep[0].data_ptr(), keep[1].data_ptr())
    assert torch.equal(keep[0], qs.state2.code.float()) and torch.equal(keep[1], qs.state2.absmax.float())


def test_bnb_stats_single_fills_the_nested_fields_with_null():
    qs = SimpleNamespace(absmax=torch.rand(12), state2=None, offset=None, blocksize=128)
    keep = []
    assert kernel._bnb_stats("caller", qs, CPU, keep) == (None, 0, None, qs.absmax.data_ptr(), 12, None, 128, 0)
    assert keep == []
    qs.absmax = qs.absmax.to(torch.float16)  # any absmax that is not uint8 is cast to fp32
    got = kernel._bnb_stats("caller", qs, CPU, keep)
    assert len(keep) == 1 and keep[0].dtype == torch.float32 and got[3:5] == (keep[0].data_ptr(), 12)
    # a uint8 absmax without state2 is single too
    assert not kernel._bnb_nested(SimpleNamespace(absmax=torch.zeros(4, dtype=torch.uint8), state2=None))
    assert not kernel._bnb_nested(SimpleNamespace(absmax=torch.zeros(4), state2=SimpleNamespace()))
    assert kernel._bnb_nested(_nested())


def test_bnb_stats_messages_name_the_caller():
    with pytest.raises(RuntimeError) as e:
        kernel._bnb_stats("nf4_linear_bnb_grouped", _nested(entries=255), CPU, [])
    assert str(e.value) == "nf4_linear_bnb_grouped: state2.code has 255 entries, expected 256"
    with pytest.raises(RuntimeError) as e:
        kernel._bnb_stats("nf4_linear_bnb", _nested(offset=torch.zeros(2)), CPU, [])
    assert str(e.value) == "nf4_linear_bnb: quant_state.offset has 2 elements, expected 1"
    qs = _nested()
    qs.state2.code = qs.state2.code.to("meta")
    with pytest.raises(RuntimeError) as e:
        kernel._bnb_stats("caller", qs, CPU, [])
    assert str(e.value) == ("NF4 quant state tensor on 'meta', packed weight on 'cpu': all of them must be on the "
                            "same ROCm device")


def test_bnb_stats_offsets():
    keep = []
    assert kernel._bnb_stats("caller", _nested(offset=None), CPU, keep)[5] is None and keep == []
    op = kernel._bnb_stats("caller", _nested(offset=0.5), CPU, keep)[5]
    assert len(keep) == 1 and keep[0].dtype == torch.float32 and keep[0].numel() == 1 and keep[0].item() == 0.5
    assert keep[0].device == CPU and op == keep[0].data_ptr()  # a host weight gets a host pointer
    keep.clear()
    op = kernel._bnb_stats("caller", _nested(offset=torch.tensor(0.5, dtype=torch.float64)), CPU, keep)[5]
    assert len(keep) == 1 and keep[0].dtype == torch.float32 and op == keep[0].data_ptr()


# ---------------------------------------------------------------- _ref_stats
def test_ref_stats():
    a1, a2, keep = torch.randint(0, 256, (8,), dtype=torch.uint8), torch.rand(2), []
    assert kernel._ref_stats(a1, a2, keep) == (a1.data_ptr(), 8, a2.data_ptr(), 2) and keep == []
    got = kernel._ref_stats(a1, a2.to(torch.float16), keep)
    assert len(keep) == 1 and keep[0].dtype == torch.float32 and got == (a1.data_ptr(), 8, keep[0].data_ptr(), 2)
    for e1, e2 in ((a1[:0], a2), (a1, a2[:0])):
        with pytest.raises(ZeroDivisionError) as e:
            kernel._ref_stats(e1, e2, [])
        assert str(e.value) == "integer division or modulo by zero (empty absmax)"


# ---------------------------------------------------------------- out= and the cross-device error
def test_check_out_messages():
    bf = torch.bfloat16
    ok = torch.empty(3, 2, 64, dtype=bf)
    assert kernel._check_out("nf4_moe_linear_bnb", None, [3, 2, 64], bf, CPU) is None
    assert kernel._check_out("nf4_moe_linear_bnb", ok, [3, 2, 64], bf, CPU) is None
    for bad in (torch.empty(3, 2, 63, dtype=bf), ok.half(), torch.empty(3, 2, 128, dtype=bf)[..., ::2],
                torch.empty(3, 2, 64, dtype=bf, device="meta")):
        with pytest.raises(ValueError) as e:
            kernel._check_out("nf4_moe_linear_bnb", bad, [3, 2, 64], bf, CPU)
        assert str(e.value) == "nf4_moe_linear_bnb: out must be a contiguous torch.bfloat16 [3, 2, 64] tensor on cpu"
    lead = torch.empty(2, 5, 8).shape[:-1]
    with pytest.raises(ValueError) as e:
        kernel._check_out("nf4_swiglu_bnb", torch.empty(2, 5, 63), [*lead, 64], torch.float16, CPU)
    assert str(e.value) == "nf4_swiglu_bnb: out must be a contiguous torch.float16 [2, 5, 64] tensor on cpu"


def test_into():
    v, out = torch.arange(4.0), torch.zeros(4)
    assert kernel._into(None, v) is v
    assert kernel._into(out, v) is out and torch.equal(out, v)


def test_two_devices_message():
    e = kernel._two_devices(torch.device("cuda", 0), CPU)
    assert isinstance(e, RuntimeError)
    assert str(e) == "Expected all tensors to be on the same device, but found at least two devices, cuda:0 and cpu!"
    with pytest.raises(RuntimeError) as raised:
        kernel._same_device(torch.empty(1), torch.empty(1, device="meta"))
    assert str(raised.value) == ("Expected all tensors to be on the same device, but found at least two devices, "
                                 "meta and cpu!")
