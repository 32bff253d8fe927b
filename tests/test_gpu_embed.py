"""The NF4 embedding gather on an MI355X: ``nf4_embedding_bnb`` / ``Embedding4bit`` against the
C oracle's dequantization of the whole table indexed by the ids (raw bit patterns, equal):
nested and single statistics, the three output dtypes, shapes at which rows and statistics
blocks do not line up, counts that are no multiple of a wave or a workgroup, ids outside
[0, rows), graph capture, the tied lm_head and the offset read on the device."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _embed_cases import (ALIGNED, DTYPES, SHAPES, TORCH_DT, bits_of, case_id, expected, gather, ids_for,
                          make_module, oracle_table, table)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ids_t", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("single", [False, True], ids=["nested", "single"])
@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_rows_equal_the_oracle(gpu, coracle, shape, single, dt, ids_t):
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    rows, dim = shape[:2]
    mod = make_module(shape, single, dt, gpu)
    ids = ids_for(rows)  # first, last, a repeated row, a descending run
    y = nf4_embedding_bnb(torch.from_numpy(ids).to(gpu, ids_t), mod)
    assert y.shape == (ids.size, dim) and y.dtype == getattr(torch, TORCH_DT[dt]) and y.device == mod.weight.device
    assert np.array_equal(bits_of(y), expected(coracle, shape, single, dt, ids))


@pytest.mark.parametrize("count", [1, 33, 64])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", ALIGNED, ids=case_id)
def test_counts_off_the_wave_and_workgroup(gpu, coracle, shape, dt, count):
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    mod = make_module(shape, False, dt, gpu)
    ids = ids_for(shape[0], count)
    y = nf4_embedding_bnb(torch.from_numpy(ids).to(gpu), mod)
    assert np.array_equal(bits_of(y), expected(coracle, shape, False, dt, ids))


@pytest.mark.parametrize("count", [2048, 2049, 2081])
@pytest.mark.parametrize("single", [False, True], ids=["nested", "single"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
def test_both_sides_of_the_blocks_per_group_threshold(gpu, coracle, dt, single, count):
    """6 x 1024: 2048 rows are 32768 output blocks, the last size at which a lane group owns one
    block; 2049 and 2081 rows take the four-block kernel, whose last workgroup is partial (2081:
    and its last wave's last steps empty)."""
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    shape = SHAPES[3]
    mod = make_module(shape, single, dt, gpu)
    ids = ids_for(shape[0], count)
    y = nf4_embedding_bnb(torch.from_numpy(ids).to(gpu), mod)
    assert np.array_equal(bits_of(y), expected(coracle, shape, single, dt, ids))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[6]], ids=case_id)
def test_ids_of_any_shape_and_a_strided_view(gpu, coracle, shape):
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    mod = make_module(shape, False, O.BF16, gpu)
    ids = torch.from_numpy(ids_for(shape[0], 6).reshape(2, 3)).to(gpu)
    y = nf4_embedding_bnb(ids, mod)
    assert y.shape == (2, 3, shape[1])
    assert np.array_equal(bits_of(y), expected(coracle, shape, False, O.BF16, ids.cpu().numpy()))
    wide = torch.from_numpy(ids_for(shape[0], 14)).to(gpu, torch.int32)
    view = wide[1::3]
    assert not view.is_contiguous()
    y = nf4_embedding_bnb(view, mod)
    assert np.array_equal(bits_of(y), expected(coracle, shape, False, O.BF16, view.cpu().numpy()))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5]], ids=case_id)
def test_out_inside_a_larger_buffer(gpu, coracle, shape, dt):
    """The bytes before and after ``out`` keep their sentinel."""
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    rows, dim = shape[:2]
    mod = make_module(shape, False, dt, gpu)
    ids = ids_for(rows, 5)
    dtype = getattr(torch, TORCH_DT[dt])
    pad = 64  # elements: keeps `out` 16-byte aligned
    buf = torch.full((pad + 5 * dim + pad,), -7.0, dtype=dtype, device=gpu)
    out = buf[pad:pad + 5 * dim].view(5, dim)
    assert nf4_embedding_bnb(torch.from_numpy(ids).to(gpu), mod, out=out) is out
    assert np.array_equal(bits_of(out), expected(coracle, shape, False, dt, ids))
    assert bool((buf[:pad] == -7.0).all()) and bool((buf[pad + 5 * dim:] == -7.0).all())


def _slack_module(shape, single, dt, gpu):
    """The case's module with packed bytes and statistics as views into allocations that carry
    two rows' worth of other (nonzero) data on each side: a read through an id just outside
    [0, rows) stays inside the allocation and shows as a nonzero value."""
    rows, dim, bs, bs2, _ = shape
    mod = make_module(shape, single, dt, gpu)
    qs = mod.weight.quant_state

    def with_slack(t, n, fill):
        pad = torch.full((max(n, 1),), fill, dtype=t.dtype, device=gpu)
        big = torch.cat([pad, t.reshape(-1), pad])
        return big, big[pad.numel():pad.numel() + t.numel()]

    keep = []
    big, v = with_slack(mod.weight.data, 2 * dim // 2, 0x1F)
    keep.append(big)
    mod.weight.data = v.view(-1, 1)
    if single:
        big, qs.absmax = with_slack(qs.absmax, 2 * dim // bs + 1, 0.5)
    else:
        big, qs.absmax = with_slack(qs.absmax, 2 * dim // bs + 1, 200)
        keep.append(big)
        big, qs.state2.absmax = with_slack(qs.state2.absmax, 2, 0.25)
    keep.append(big)
    mod._keep = keep
    return mod


@pytest.mark.parametrize("ids_t", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("single", [False, True], ids=["nested", "single"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[6]], ids=case_id)
def test_ids_out_of_range_give_zero_rows(gpu, coracle, shape, single, ids_t):
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    rows, dim = shape[:2]
    mod = _slack_module(shape, single, O.BF16, gpu)
    bad = [-1, rows, rows + 1]
    if ids_t == torch.int64:
        bad.append(2 ** 32 + 1)  # its low half names a valid row: a 32-bit compare is caught
    ids = []
    for i, b in enumerate(bad):
        ids += [i % rows, b]
    ids += [rows - 1]
    ids = np.array(ids, np.int64)
    y = nf4_embedding_bnb(torch.from_numpy(ids).to(gpu, ids_t), mod)
    want = expected(coracle, shape, single, O.BF16, ids)
    got = bits_of(y)
    oob = (ids < 0) | (ids >= rows)
    assert oob.sum() == len(bad) and not got[oob].any()  # all-zero bits
    assert want[~oob].any() and np.array_equal(got, want)


def test_graph_capture_follows_new_ids(gpu):
    from nf4_triton_dequantization_amd import Embedding4bit

    torch.manual_seed(11)
    w = torch.randn(96, 256, device=gpu, dtype=torch.bfloat16)
    emb = Embedding4bit.from_float(w)
    ids = torch.tensor([3, 95, 0, 3, 17], device=gpu)
    new = torch.tensor([90, 1, 1, 64, 2], device=gpu)
    with torch.no_grad():
        emb(ids)  # (code books cached, library loaded)
        eager_new = emb(new)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # a host read of ids or the offset would be refused here
            y = emb(ids)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, emb(ids))
        ids.copy_(new)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager_new) and bool(y.float().abs().sum() > 0)


def test_tied_lm_head_runs_the_fused_gemm_on_the_embedding_storage(gpu, monkeypatch):
    from nf4_triton_dequantization_amd import Embedding4bit, Linear4bit, kernel

    torch.manual_seed(12)
    w = torch.randn(192, 256, device=gpu, dtype=torch.bfloat16)
    emb = Embedding4bit.from_float(w)
    ref = Linear4bit.from_float(w)  # the same packed weight, its own storage
    head = emb.as_linear()
    assert head.weight is emb.weight and torch.equal(ref.weight.data, emb.weight.data)
    x = torch.randn(4, 256, device=gpu, dtype=torch.bfloat16)

    def unfused(*a, **k):
        raise AssertionError("the tied lm_head fell back to dequantize + matmul at a decode size")

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", unfused)
    with torch.no_grad():
        y, y_ref = head(x), ref(x)
    assert y.shape == (4, 192) and torch.equal(y, y_ref) and bool(torch.isfinite(y.float()).all())


def test_offset_is_read_on_the_device(gpu, coracle):
    from nf4_triton_dequantization_amd import nf4_embedding_bnb

    shape = SHAPES[1]
    mod = make_module(shape, False, O.F16, gpu)
    ids = ids_for(shape[0])
    dev_ids = torch.from_numpy(ids).to(gpu)
    y = nf4_embedding_bnb(dev_ids, mod)
    assert np.array_equal(bits_of(y), expected(coracle, shape, False, O.F16, ids))
    mod.weight.quant_state.offset.fill_(0.25)  # in place, on the device
    y2 = nf4_embedding_bnb(dev_ids, mod)
    want = gather(oracle_table(coracle, shape, False, O.F16, table(shape, False, O.F16), offset=0.25), ids)
    assert np.array_equal(bits_of(y2), want) and not np.array_equal(bits_of(y2), bits_of(y))
