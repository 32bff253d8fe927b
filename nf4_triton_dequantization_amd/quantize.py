"""NF4 quantization on the device: float weights into the bitsandbytes 4-bit layout.

``nf4_quantize(w)`` is the HIP form of ``bnb_layout.quantize_nf4(w)``: the same
``(packed uint8 [ceil(numel/2), 1], QuantState)``, computed by ``libnf4dq.so``
(``nf4_quant_bnb`` / ``nf4_quant_bnb_nested``, csrc/nf4_quant.hip) in one pass over
the weight instead of a chain of torch ops with fp32 / int64 temporaries.  ``packed``
and the fp32 ``absmax`` are bit-identical to the Python quantizer's.  With
``compress_statistics=True`` the ``offset`` is the correctly rounded fp64 mean of the
absmax (the Python quantizer reduces in fp32, so the two may differ in the last
bit), and ``absmax_q`` / ``state2.absmax`` follow from that offset exactly as
``quantize_blockwise_8bit`` computes them.

Device tensors run on their device, on the current stream, without a host
synchronisation (the call can be captured in a graph once the code books are cached,
i.e. after one call on that device).  Host tensors raise, as every other entry does,
unless ``NF4_BACKEND=cpu`` selects the library's host path.  Importing this module
loads no native code.
"""
from __future__ import annotations

import torch

from . import _lib
from .bnb_layout import NF4_CODE, QuantState, dynamic_map
from .kernel import _DTYPE_CODE, _raw_stream, _require_device, backend, cpu_threads

BLOCKSIZE2 = 256
_BLOCKSIZES = (64, 128, 256, 512, 1024, 2048, 4096)

# device -> (NF4 code points, dynamic-map code book), both fp32 on that device
_CODES = {}


def _codes(device: torch.device):
    ent = _CODES.get(device)
    if ent is None:
        ent = (NF4_CODE.to(device), dynamic_map(signed=True).to(device))
        _CODES[device] = ent
    return ent


def nf4_quantize(w: torch.Tensor, blocksize: int = 64, compress_statistics: bool = True):
    """NF4-quantize ``w`` (fp16 / bf16 / fp32 / fp64, any shape) as ``quantize_nf4`` does.

    Returns ``(packed uint8 [ceil(numel/2), 1], QuantState)`` with ``shape``, ``code``,
    ``blocksize``, ``quant_type="nf4"``, ``dtype = w.dtype`` and, when
    ``compress_statistics``, ``offset`` (0-dim fp32 tensor on the weight's device) and
    ``state2`` (``code``: the dynamic map, ``blocksize`` 256, ``dtype`` float32).
    """
    if blocksize not in _BLOCKSIZES:
        raise ValueError(f"nf4_quantize: blocksize {blocksize} not one of {_BLOCKSIZES}")
    shape, dtype, dev = w.shape, w.dtype, w.device
    src = w.detach()
    if src.dtype == torch.float64:
        src = src.to(torch.float32)  # the Python quantizer computes in fp32
    code = _DTYPE_CODE.get(src.dtype)
    if code is None:
        raise TypeError(f"nf4_quantize: unsupported weight dtype {dtype}; expected float16, bfloat16, float32 "
                        f"or float64")
    on_host = dev.type != "cuda"
    if on_host and (dev.type != "cpu" or backend() != "cpu"):
        _require_device(w)
    src = src.contiguous().view(-1)
    numel = src.numel()
    nblk = (numel + blocksize - 1) // blocksize
    code1, code2 = _codes(dev)
    packed = torch.empty(((numel + 1) // 2, 1), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    if not compress_statistics:
        absmax = torch.empty(nblk, dtype=torch.float32, device=dev)
        if numel:
            if on_host:
                rc = L.nf4_quant_bnb_cpu(src.data_ptr(), code, numel, blocksize, packed.data_ptr(),
                                         absmax.data_ptr(), cpu_threads())
            else:
                with torch.cuda.device(dev):
                    rc = L.nf4_quant_bnb(src.data_ptr(), code, numel, blocksize, packed.data_ptr(),
                                         absmax.data_ptr(), _raw_stream(dev.index))
            _lib.check(rc, "nf4 quantize")
        qs = QuantState(absmax=absmax, shape=shape, code=code1, blocksize=blocksize, quant_type="nf4", dtype=dtype)
        return packed, qs
    absmax_q = torch.empty(nblk, dtype=torch.uint8, device=dev)
    absmax2 = torch.empty((nblk + BLOCKSIZE2 - 1) // BLOCKSIZE2, dtype=torch.float32, device=dev)
    if numel:
        offset = torch.empty((), dtype=torch.float32, device=dev)
        if on_host:
            rc = L.nf4_quant_bnb_nested_cpu(src.data_ptr(), code, numel, blocksize, code2.data_ptr(), BLOCKSIZE2,
                                            packed.data_ptr(), absmax_q.data_ptr(), absmax2.data_ptr(),
                                            offset.data_ptr(), cpu_threads())
        else:
            nws = int(L.nf4_quant_workspace_bytes(numel, blocksize))
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)  # fp32 absmax + partial sums; dead after the call
            with torch.cuda.device(dev):
                rc = L.nf4_quant_bnb_nested(src.data_ptr(), code, numel, blocksize, code2.data_ptr(), BLOCKSIZE2,
                                            packed.data_ptr(), absmax_q.data_ptr(), absmax2.data_ptr(),
                                            offset.data_ptr(), ws.data_ptr(), nws, _raw_stream(dev.index))
        _lib.check(rc, "nf4 quantize (nested)")
    else:
        offset = torch.full((), float("nan"), dtype=torch.float32, device=dev)  # the mean of no blocks
    state2 = QuantState(absmax=absmax2, code=code2, blocksize=BLOCKSIZE2, quant_type=None, dtype=torch.float32)
    qs = QuantState(absmax=absmax_q, shape=shape, code=code1, blocksize=blocksize, quant_type="nf4", dtype=dtype,
                    offset=offset, state2=state2)
    return packed, qs
