"""What the Python API hands to the C ABI on every fused route (``-m gpu``): a recording proxy around
the loaded library (_host_call_cases.py) notes each entry and its arguments, descriptors read back
through the ``_lib`` structures.  Operands already in the entry's form must arrive as their own
pointers (no hidden copy); operands that need preparation (fp32 x, a strided x, x two bytes off
alignment, int64 ids, an fp16 code2) arrive as 16-byte-aligned temporaries with nothing else in
the call changed and the result bit for bit the clean call's; the workspace is null exactly when
the size query returned 0 and otherwise the cached tensor of (device, current stream); the stream
is the current one, on the default stream and inside ``torch.cuda.stream``; cfg is never set."""
import ctypes

import pytest
import torch

from _host_call_cases import CASES, expect_prepared, launches, normalise, pointer_names, record

from nf4_triton_dequantization_amd import _lib, kernel

pytestmark = pytest.mark.gpu

_CLEAN = {}


def _clean(gpu, name):
    """The clean call of a case on the default stream, run once: (call, result, raw calls, normalised)."""
    if name not in _CLEAN:
        call = CASES[name][0](gpu, None)
        result, calls = record(kernel, call)
        _CLEAN[name] = (call, result.clone(), calls, normalise(calls, call.tensors, kernel, gpu))
    return _CLEAN[name]


def _check_workspace_and_stream(call, calls, gpu):
    """The launch's workspace, stream and cfg arguments against the size query and the caches."""
    handle = torch.cuda.current_stream(gpu).cuda_stream
    cache = kernel._MOE_DOWN_WS if call.fn == "nf4_moe_down_bnb" else kernel._GEMM_WS
    sizes = [c for c in calls if c[0].endswith("_workspace_bytes")]
    for name, args, rv in launches(calls):
        assert rv == 0, (name, rv)
        assert (args[-1][1] or 0) == handle, f"{name}: stream {args[-1][1]} is not the current one ({handle})"
        assert all(v is None for kind, v in args if kind == "cfg"), f"{name}: cfg is set"
        types = _lib.SIGNATURES[name][1]
        if ctypes.c_size_t not in types:
            assert name in ("nf4_lora_add", "nf4_lora_add_routed", "nf4_embedding_bnb")
            assert name == "nf4_embedding_bnb" or args[-2] == ("ptr", None), f"{name}: cfg is set"
            continue
        at = types.index(ctypes.c_size_t)
        (_, wp), (_, ws_bytes) = args[at - 1], args[at]
        size = {"nf4_gemm_ref": "nf4_gemm", "nf4_gemm_ref_grouped": "nf4_gemm_grouped"}.get(name, name.replace("_single", ""))
        query = [c for c in sizes if c[0] == size + "_workspace_bytes"]
        assert len(query) == 1 and query[0][2] == ws_bytes, (name, ws_bytes, [c[0] for c in sizes])
        if ws_bytes == 0:
            assert wp is None, f"{name}: a workspace for a launch that wants none"
        else:
            ws, stream = cache[gpu.index, handle]
            assert wp == ws.data_ptr() and ws_bytes <= ws.numel() and stream.cuda_stream == handle, name


@pytest.mark.parametrize("name", list(CASES))
def test_clean_operands_arrive_as_they_are(gpu, name):
    call, _result, calls, norm = _clean(gpu, name)
    assert [c[0] for c in launches(calls)] == call.entries
    assert len(calls) - len(call.entries) == sum(ctypes.c_size_t in _lib.SIGNATURES[e][1] for e in call.entries)
    missing = set(call.tensors) - pointer_names(norm)
    assert not missing, f"{name}: the entry never saw the pointer of {sorted(missing)}"
    _check_workspace_and_stream(call, calls, gpu)


@pytest.mark.parametrize("name", list(CASES))
def test_side_stream_gets_its_own_handle_and_workspace(gpu, name):
    _call, want, _calls, norm_default = _clean(gpu, name)
    call = CASES[name][0](gpu, None)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(gpu).cuda_stream == side.cuda_stream != 0
        result, calls = record(kernel, call)
        _check_workspace_and_stream(call, calls, gpu)
        assert normalise(calls, call.tensors, kernel, gpu) == norm_default
    side.synchronize()
    assert torch.equal(result, want)


@pytest.mark.parametrize("name,variant,operand,copied_in",
                         [(n, *v) for n, (_b, variants) in CASES.items() for v in variants],
                         ids=[f"{n}-{v[0]}" for n, (_b, variants) in CASES.items() for v in variants])
def test_prepared_operands_arrive_as_aligned_temporaries(gpu, name, variant, operand, copied_in):
    _call, want, _calls, norm_clean = _clean(gpu, name)
    call = CASES[name][0](gpu, variant)
    result, calls = record(kernel, call)
    own = call.tensors[operand]
    assert normalise(calls, call.tensors, kernel, gpu) == expect_prepared(norm_clean, operand, copied_in,
                                                                          own.data_ptr() % 16)
    assert operand not in pointer_names(normalise([c for c in calls if copied_in is None or c[0] in copied_in],
                                                  call.tensors, kernel, gpu))
    _check_workspace_and_stream(call, calls, gpu)
    assert torch.equal(result, want), f"{name} with {variant}: not the clean call's result"
