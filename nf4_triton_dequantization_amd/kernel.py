"""Drop-in host side of the NF4 dequantization path (MI355X / gfx950).

Mirrors the reference's operator interface
(/root/reference/nf4_triton_dequantization/kernel_optimized.py):

* ``triton_dequantize_nf4(module)``          <- :113-139 (+ launcher :142-205)
* ``reset_triton_dequantize_state()``       <- :317-319 (no-op; no caches here either)

Same attribute reads (``module.weight.data``, ``.weight.quant_state.absmax``,
``.quant_state.state2.absmax``, ``.quant_state.dtype``, ``module.out_features``,
``module.in_features``), same value casts (qweight -> uint8 :162-163, nested
absmax -> fp32 :182), same output (new row-major ``[m, n]`` tensor of
``quant_state.dtype`` on the weight's device, :189), launched on the caller's
current stream.  A uint8 absmax takes the double-dequant kernel; any other
absmax dtype takes the single-quant kernel, exactly where the reference falls
back to ``_aggressive_pytorch_t4`` (:166-167 -> :273-274).

Error behaviour: the reference raises from torch/Triton (RuntimeError for a
tensor it cannot view or a CPU tensor -- "0 active drivers" --,
AttributeError for a missing ``state2``, ZeroDivisionError for an empty
absmax); the same exception types are raised here.  There is no CPU path and
no silent fallback: compute always goes through ``libnf4dq.so``.

Extensions beyond the reference: ``dequantize_nf4_many`` (one
launch for many weights), ``dequantize_nf4_bnb`` (bitsandbytes semantics,
parity unpinned), ``dequantize_nf4_into`` (caller-provided output) and the
consumer ``x @ W.t()`` fused: ``nf4_linear`` / ``nf4_linear_grouped`` (reference
semantics) and ``nf4_linear_bnb`` (bitsandbytes semantics, what ``Linear4bit.forward`` runs);
``nf4_moe_linear_bnb`` runs one projection of a mixture-of-experts block for all experts
(``Experts4bit``) in one launch, routed on the device.
"""
from __future__ import annotations

import ctypes
import os
from typing import Iterable, List, Optional, Sequence

import torch

from . import _lib

_DTYPE_CODE = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16, torch.float32: _lib.F32}


BACKEND_ENV = "NF4_BACKEND"
THREADS_ENV = "NF4_CPU_THREADS"


def backend() -> str:
    """Where host (CPU) tensors go: ``NF4_BACKEND`` = ``hip`` (default) or ``cpu``.

    ``hip`` keeps the reference's behaviour: a weight on the host raises
    (the reference hands it to Triton, which has no CPU driver).  ``cpu`` runs
    host tensors through the library's own host path (``nf4_dequant_ref_cpu``,
    SURVEY §8b), bit-identical to the HIP kernels and to the reference
    fallback.  Device tensors always run on their device.  Read on every call.
    """
    b = os.environ.get(BACKEND_ENV, "hip").strip().lower() or "hip"
    if b not in ("hip", "cpu"):
        raise ValueError(f"{BACKEND_ENV}={b!r}: expected 'hip' or 'cpu'")
    return b


def cpu_threads() -> int:
    """Worker threads of the host path: ``NF4_CPU_THREADS``, else torch's intra-op thread count."""
    v = os.environ.get(THREADS_ENV, "")
    return int(v) if v.strip() else torch.get_num_threads()


def _dtype_code(dtype: torch.dtype) -> int:
    try:
        return _DTYPE_CODE[dtype]
    except KeyError:
        raise TypeError(f"unsupported quant_state.dtype {dtype}; expected float16, bfloat16, float32 "
                        f"or float64") from None


def _require_device(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        # The reference hands a CPU tensor to Triton, which raises
        # RuntimeError("0 active drivers ..."); there is no CPU path here either.
        raise RuntimeError(
            f"triton_dequantize_nf4: weight is on '{t.device}'; the NF4 HIP path needs a ROCm device tensor")


def _on_device(device: torch.device, *tensors: torch.Tensor) -> None:
    """Quant statistics must live with the packed weight (the reference hands them
    to Triton, which refuses a host tensor); never pass a host pointer to a kernel."""
    for t in tensors:
        if t.device != device:
            raise RuntimeError(f"NF4 quant state tensor on '{t.device}', packed weight on '{device}': "
                               f"all of them must be on the same ROCm device")


def _two_devices(a, b) -> RuntimeError:
    # what `x @ W.t()` raises for tensors on different devices
    return RuntimeError(f"Expected all tensors to be on the same device, but found at least two devices, "
                        f"{a} and {b}!")


def _as_u8_flat(q: torch.Tensor) -> torch.Tensor:
    if q.dtype != torch.uint8:
        q = q.to(torch.uint8)              # value cast, as :162-163
    return q.contiguous().view(-1)


def _prepare(module):
    """Attribute reads and casts of kernel_optimized.py:146-186."""
    weight = module.weight
    quant_state = weight.quant_state
    qweight = weight.data
    absmax = quant_state.absmax
    absmax32 = quant_state.state2.absmax    # AttributeError when state2 is None, as :151
    dtype = quant_state.dtype
    m = int(module.out_features)
    n = int(module.in_features)
    return qweight, absmax, absmax32, dtype, m, n


def _operand(t: torch.Tensor, dtype, keep: list) -> tuple:
    """(data pointer, numel) of ``t`` as a contiguous tensor of ``dtype`` (None: its own).  A cast or
    copy made for that goes to ``keep``, which the caller holds until the entry has returned."""
    c = t if dtype is None or t.dtype == dtype else t.to(dtype)
    if not c.is_contiguous():
        c = c.contiguous()
    if c is not t:
        keep.append(c)
    return c.data_ptr(), c.numel()


def _ref_stats(absmax: torch.Tensor, absmax32: torch.Tensor, keep: list) -> tuple:
    """The statistics operands in reference semantics, ``(ap, an, bp, bn)``: uint8 absmax as it is,
    absmax32 cast to fp32 (:182); an empty one raises as the reference's ceil(total / 0) does (:175, :184)."""
    ap, an = _operand(absmax, None, keep)
    bp, bn = _operand(absmax32, torch.float32, keep)
    if an == 0 or bn == 0:
        raise ZeroDivisionError("integer division or modulo by zero (empty absmax)")
    return ap, an, bp, bn


def _launch(qweight, absmax, absmax32, out, m, n, code, stream) -> None:
    """Casts of kernel_optimized.py:162-186 and one C-ABI call on `stream`."""
    keep = []
    qp, qn = _operand(qweight, torch.uint8, keep)  # value cast, as :162-163
    _on_device(qweight.device, absmax, absmax32 if absmax.dtype == torch.uint8 else absmax)
    L = _lib.lib()
    if absmax.dtype == torch.uint8:
        rc = L.nf4_dequant_ref(qp, qn, *_ref_stats(absmax, absmax32, keep), out.data_ptr(), code, m, n, stream)
    else:
        # single-quant branch (:166-167 -> :273-274): absmax.view(m, -1)[:, :bpr].to(float32)
        rc = L.nf4_dequant_single(qp, qn, *_operand(absmax, torch.float32, keep), out.data_ptr(), code, m, n, stream)
    if rc:
        _lib.check(rc, "nf4 dequantize")


def dequantize_nf4_into(qweight: torch.Tensor, absmax: torch.Tensor, absmax32: torch.Tensor,
                        out: torch.Tensor, m: int, n: int) -> torch.Tensor:
    """Dequantize into a caller-provided contiguous ``out`` ([m, n] elements, fp16/bf16/fp32)."""
    _require_device(qweight)
    code = _dtype_code(out.dtype)
    if not out.is_contiguous() or out.numel() != m * n:
        raise RuntimeError("dequantize_nf4_into: out must be a contiguous tensor of m*n elements")
    if m == 0 or n == 0:
        return out
    with torch.cuda.device(qweight.device):
        _launch(qweight, absmax, absmax32, out, m, n, code, torch.cuda.current_stream().cuda_stream)
    return out


def _launch_cpu(qweight, absmax, absmax32, out, m, n, code) -> None:
    """NF4_BACKEND=cpu: the same casts and checks, then the library's host path
    (``nf4_dequant_ref_cpu`` / ``nf4_dequant_single_cpu``, synchronous)."""
    for t in (absmax, absmax32) if absmax.dtype == torch.uint8 else (absmax,):
        if t.device.type != "cpu":
            raise RuntimeError(f"NF4 quant state tensor on '{t.device}', packed weight on the host: "
                               f"all of them must be on the same device")
    keep = []
    qp, qn = _operand(qweight, torch.uint8, keep)  # value cast, as :162-163
    L = _lib.lib()
    threads = cpu_threads()
    if absmax.dtype == torch.uint8:
        rc = L.nf4_dequant_ref_cpu(qp, qn, *_ref_stats(absmax, absmax32, keep), out.data_ptr(), code, m, n, threads)
    else:
        rc = L.nf4_dequant_single_cpu(qp, qn, *_operand(absmax, torch.float32, keep), out.data_ptr(), code, m, n,
                                      threads)
    if rc:
        _lib.check(rc, "nf4 dequantize (cpu)")


_REF = None  # bound nf4_dequant_ref (fast path: one attribute lookup less per call)
_raw_stream = torch._C._cuda_getCurrentRawStream  # device index -> hipStream_t of the current stream
_U8, _F32 = torch.uint8, torch.float32
# tensor-level fast entry (csrc/nf4_torch_ext.cpp), resolved on the first drop-in call
# (importing the package loads no native code; a missing libnf4dq.so raises there)
_EXT = None
_EXT_READY = False


def _ext():
    global _EXT, _EXT_READY
    if not _EXT_READY:
        _EXT = _lib.ext()  # raises when libnf4dq.so is missing; None when nf4ext.so is absent / unusable
        _EXT_READY = True
    return _EXT


def _dequantize(qweight, absmax, absmax32, dtype, m, n) -> torch.Tensor:
    if dtype == torch.float64:
        # the reference computes in fp32 and casts on the store (:109-110, :310):
        # fp64 output = the fp32 product, widened exactly
        return _dequantize(qweight, absmax, absmax32, torch.float32, m, n).to(torch.float64)
    code = _dtype_code(dtype)  # raise before allocating
    ext = _EXT if _EXT_READY else _ext()
    if ext is not None:
        # uint8 / uint8 / fp32 contiguous device tensors: checks, allocation, stream
        # and launch in one C++ call (None = this call needs the general path below)
        out = ext.dequant_ref(qweight, absmax, absmax32, m, n, code)
        if out is not None:
            return out
    dev = qweight.device
    if dev.type != "cuda":
        if dev.type != "cpu" or backend() != "cpu":
            _require_device(qweight)
        out = torch.empty((m, n), dtype=dtype)
        if m and n:
            _launch_cpu(qweight, absmax, absmax32, out, m, n, code)
        return out
    out = torch.empty((m, n), dtype=dtype, device=dev)
    if m == 0 or n == 0:
        return out
    idx = dev.index
    if idx == torch.cuda.current_device():
        # fast path: inputs already in the kernel's types, contiguous, on this device
        if (qweight.dtype == _U8 and absmax.dtype == _U8 and absmax32.dtype == _F32 and qweight.is_contiguous()
                and absmax.is_contiguous() and absmax32.is_contiguous() and absmax.device == dev
                and absmax32.device == dev):
            nb = absmax.numel()
            n2 = absmax32.numel()
            if nb and n2:
                global _REF
                if _REF is None:
                    _REF = _lib.lib().nf4_dequant_ref
                rc = _REF(qweight.data_ptr(), qweight.numel(), absmax.data_ptr(), nb, absmax32.data_ptr(), n2,
                          out.data_ptr(), code, m, n, _raw_stream(idx))
                if rc:
                    _lib.check(rc, "nf4 dequantize")
                return out
        _launch(qweight, absmax, absmax32, out, m, n, code, _raw_stream(idx))
    else:
        with torch.cuda.device(dev):
            _launch(qweight, absmax, absmax32, out, m, n, code, torch.cuda.current_stream().cuda_stream)
    return out


def triton_dequantize_nf4(module) -> torch.Tensor:
    """Dequantize a bitsandbytes-layout NF4 ``Linear4bit`` weight to ``[out_features, in_features]``.

    Drop-in for ``nf4_triton_dequantization.triton_dequantize_nf4``
    (kernel_optimized.py:113).  Returns a new contiguous tensor of
    ``quant_state.dtype`` on the weight's device.  Host tensors raise (as the
    reference's Triton path does) unless ``NF4_BACKEND=cpu`` selects the
    library's host path.
    """
    weight = module.weight
    quant_state = weight.quant_state
    absmax32 = quant_state.state2.absmax  # AttributeError when state2 is None, as :151
    # `.data` of an nn.Parameter builds a new tensor object per access (~0.8 us);
    # a Parameter is itself the tensor whose storage `.data` would expose
    qweight = weight if isinstance(weight, torch.Tensor) else weight.data
    m, n = int(module.out_features), int(module.in_features)
    dtype = quant_state.dtype
    ext = _EXT if _EXT_READY else _ext()
    if ext is not None:
        code = _DTYPE_CODE.get(dtype)
        if code is not None:
            # common call straight to the tensor-level entry (None = general path)
            out = ext.dequant_ref(qweight, quant_state.absmax, absmax32, m, n, code)
            if out is not None:
                return out
    return _dequantize(weight.data, quant_state.absmax, absmax32, dtype, m, n)


def reset_triton_dequantize_state() -> None:
    """No-op, as kernel_optimized.py:317-319: the path keeps no cached state."""
    return None


def dequantize_nf4_many(modules: Iterable, out: Optional[Sequence[Optional[torch.Tensor]]] = None
                        ) -> List[torch.Tensor]:
    """Dequantize several weights with as few launches as possible.

    Equivalent to ``[triton_dequantize_nf4(m) for m in modules]`` (the
    benchmark.py:68-84 pattern) but folds every uint8-absmax weight of one
    device and dtype into batched launches of up to ``NF4DQ_BATCH_MAX`` matrices.
    ``out`` (optional, one entry per module, None = allocate): caller-owned
    contiguous ``[out_features, in_features]`` tensors of ``quant_state.dtype`` on
    the weight's device, written in place and returned (a preallocated weight
    buffer reused across steps or graph replays).
    """
    modules = list(modules)
    given = list(out) if out is not None else [None] * len(modules)
    if len(given) != len(modules):
        raise ValueError("dequantize_nf4_many: one out tensor (or None) per module")
    outs: List[Optional[torch.Tensor]] = [None] * len(modules)
    groups = {}
    keep = []  # tensors referenced by descriptors must outlive the launch
    for i, mod in enumerate(modules):
        qweight, absmax, absmax32, dtype, m, n = _prepare(mod)
        o = given[i]
        if o is not None and (o.shape != (m, n) or o.dtype != dtype or o.device != qweight.device
                              or not o.is_contiguous()):
            raise RuntimeError(f"dequantize_nf4_many: out[{i}] must be a contiguous {dtype} tensor of shape "
                               f"({m}, {n}) on {qweight.device}")
        if qweight.device.type != "cuda" or absmax.dtype != torch.uint8 or dtype not in _DTYPE_CODE:
            # host tensors (NF4_BACKEND=cpu, or the reference's error), single-quant
            # absmax, fp64 output: one call each
            r = triton_dequantize_nf4(mod)
            outs[i] = o.copy_(r) if o is not None else r
            continue
        code = _dtype_code(dtype)
        out_t = o if o is not None else torch.empty((m, n), dtype=dtype, device=qweight.device)
        outs[i] = out_t
        if m == 0 or n == 0:
            continue
        q = _as_u8_flat(qweight)
        _on_device(q.device, absmax, absmax32)
        keep.append(q)
        d = _lib.MatrixDesc(q.data_ptr(), q.numel(), *_ref_stats(absmax, absmax32, keep), out_t.data_ptr(), m, n)
        groups.setdefault((q.device, code), []).append(d)
    L = _lib.lib()
    for (device, code), descs in groups.items():
        arr = (_lib.MatrixDesc * len(descs))(*descs)
        _stream_call("nf4 batched dequantize", device, L.nf4_dequant_ref_batched, arr, len(descs), code)
    # Temporaries in `keep` (value casts) were allocated on the stream the
    # launches use, so the caching allocator's stream-ordered reuse already
    # protects them; no record_stream needed (and it would break graph capture).
    del keep
    return outs  # type: ignore[return-value]


def dequantize_nf4_bnb(module) -> torch.Tensor:
    """bitsandbytes ``dequantize_4bit`` semantics (parity unpinned).

    Reads ``quant_state.{absmax, code?, offset, blocksize, shape, dtype}`` and, when
    nested, ``state2.{absmax, code, blocksize}``; output has ``quant_state.shape``.
    """
    weight = module.weight
    qs = weight.quant_state
    _require_device(weight.data)
    q = _as_u8_flat(weight.data)
    shape = tuple(qs.shape) if getattr(qs, "shape", None) is not None else (int(module.out_features),
                                                                            int(module.in_features))
    numel = 1
    for s in shape:
        numel *= int(s)
    code = _dtype_code(qs.dtype)
    out = torch.empty(shape, dtype=qs.dtype, device=q.device)
    if numel == 0:
        return out
    bs = int(qs.blocksize)
    with torch.cuda.device(q.device):  # the launch's device = the weight's (not the current one)
        rc = _launch_bnb(q, qs, out, code, numel, bs)
    _lib.check(rc, "nf4 bnb dequantize")
    return out


def _launch_bnb(q, qs, out, code, numel, bs) -> int:
    L = _lib.lib()
    stream = _raw_stream(q.device.index)
    if _bnb_nested(qs):
        _on_device(q.device, qs.absmax, qs.state2.code, qs.state2.absmax)
        a1 = qs.absmax.contiguous().view(-1)
        code2 = qs.state2.code.to(torch.float32).contiguous()
        a2 = qs.state2.absmax.to(torch.float32).contiguous().view(-1)
        off = qs.offset
        off = float(off.item()) if torch.is_tensor(off) else float(off or 0.0)
        rc = L.nf4_dequant_bnb(q.data_ptr(), a1.data_ptr(), a1.numel(), code2.data_ptr(), a2.data_ptr(),
                               a2.numel(), ctypes.c_float(off), out.data_ptr(), code, numel, bs,
                               int(qs.state2.blocksize), stream)
    else:
        _on_device(q.device, qs.absmax)
        am = qs.absmax.to(torch.float32).contiguous().view(-1)
        rc = L.nf4_dequant_bnb_single(q.data_ptr(), am.data_ptr(), am.numel(), out.data_ptr(), code, numel,
                                      bs, stream)
    return rc


_IDS_CODE = {torch.int32: _lib.IDS_I32, torch.int64: _lib.IDS_I64}


def _bnb_nested(qs) -> bool:
    """Nested statistics or plain fp32 absmax: the one decision of every bitsandbytes-semantics entry."""
    return getattr(qs, "state2", None) is not None and qs.absmax.dtype == torch.uint8


def _offset_ptr(name: str, off, device, keep: list):
    """``quant_state.offset`` as a pointer on ``device``: never a host read.  A tensor already there
    passes as it is (a kernel reads its one float when it runs), a Python number becomes a scalar
    on ``device``, None a null pointer (= 0).  A tensor made here goes to ``keep``."""
    if off is None:
        return None
    made = off
    if not torch.is_tensor(off):
        made = torch.tensor(float(off), dtype=torch.float32, device=device)
    elif off.device != device or off.dtype != torch.float32:
        made = off.to(device=device, dtype=torch.float32)  # stream-ordered copy, no synchronisation
    if made.numel() != 1:
        raise RuntimeError(f"{name}: quant_state.offset has {made.numel()} elements, expected 1")
    if made is not off:
        keep.append(made)
    return made.data_ptr()


def _bnb_stats(name: str, qs, dev, keep: list) -> tuple:
    """The statistics operands of one weight in bitsandbytes semantics, in the order of the entries'
    arguments and of ``GemmBnbMat``'s fields: ``(ap, an, cp, bp, bn, op, bs, bs2)``.  Plain fp32
    absmax fills the nested-only fields with null and 0 and passes absmax as (bp, bn).  The pointers
    are on ``dev``, the packed weight's device (the host for ``nf4_embedding_bnb`` under
    NF4_BACKEND=cpu); every cast or copy made goes to ``keep``."""
    bs = int(qs.blocksize)
    if not _bnb_nested(qs):
        _on_device(dev, qs.absmax)
        return (None, 0, None, *_operand(qs.absmax, torch.float32, keep), None, bs, 0)
    st2 = qs.state2
    _on_device(dev, qs.absmax, st2.code, st2.absmax)
    ap, an = _operand(qs.absmax, None, keep)
    cp, cn = _operand(st2.code, torch.float32, keep)
    bp, bn = _operand(st2.absmax, torch.float32, keep)
    if cn != 256:
        raise RuntimeError(f"{name}: state2.code has {cn} entries, expected 256")
    return ap, an, cp, bp, bn, _offset_ptr(name, qs.offset, dev, keep), bs, int(st2.blocksize)


def _bnb_mat(name: str, mod, dev, y_ptr, keep: list) -> "_lib.GemmBnbMat":
    """The ``GemmBnbMat`` descriptor of one ``Linear4bit`` for the grouped and the SwiGLU launch."""
    return _lib.GemmBnbMat(*_operand(mod.weight.data, None, keep), *_bnb_stats(name, mod.weight.quant_state, dev, keep),
                           y_ptr, int(mod.out_features))


def nf4_embedding_bnb(ids: torch.Tensor, module, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rows ``ids`` of an NF4 table in bitsandbytes semantics: ``dequantize_nf4_bnb(module)[ids]``
    bit for bit, without dequantizing the table.

    ``module.weight`` is a ``Params4bit`` whose ``quant_state.shape`` is ``[rows, dim]``;
    ``ids`` has any shape, int32 or int64, on the weight's device.  Returns
    ``ids.shape + (dim,)`` in ``quant_state.dtype`` (fp16, bf16 or fp32); ``out=`` takes a
    contiguous tensor of that shape and dtype.  On a GPU weight this is ONE launch on the
    current stream (``nf4_embedding_bnb`` / ``nf4_embedding_bnb_single``) that reads only the
    selected rows' packed bytes and statistics and reads ``offset`` on the device: nothing is
    read back, so the call can be captured in a graph.  An id outside ``[0, rows)`` gives a
    row of zeros (never a device assert or an out-of-bounds read).  Host tensors run the
    library's host path under ``NF4_BACKEND=cpu`` and raise otherwise.  There is no
    fallback: a ``quant_type`` other than nf4, a blocksize that is not a power of two in
    64..4096 (nested: a blocksize2 that is not a power of two >= 4), an ``ids`` dtype other
    than int32 / int64 or ``ids`` on another device raise.
    """
    weight = module.weight
    qs = weight.quant_state
    qweight = weight.data
    dev = qweight.device
    on_host = dev.type != "cuda"
    if on_host and (dev.type != "cpu" or backend() != "cpu"):
        _require_device(qweight)
    qt = getattr(qs, "quant_type", None)
    if qt != "nf4":
        raise ValueError(f"nf4_embedding_bnb: quant_type {qt!r} is not supported, expected 'nf4'")
    shape = tuple(int(s) for s in qs.shape) if getattr(qs, "shape", None) is not None else ()
    if len(shape) != 2:
        raise ValueError(f"nf4_embedding_bnb: quant_state.shape {shape} is not [rows, dim]")
    rows, dim = shape
    bs = int(qs.blocksize)
    if bs < 64 or bs > 4096 or bs & (bs - 1):
        raise ValueError(f"nf4_embedding_bnb: blocksize {bs} is not a power of two in 64..4096")
    nested = _bnb_nested(qs)
    bs2 = int(qs.state2.blocksize) if nested else 0
    if nested and (bs2 < 4 or bs2 & (bs2 - 1)):
        raise ValueError(f"nf4_embedding_bnb: state2.blocksize {bs2} is not a power of two >= 4")
    if not torch.is_tensor(ids) or ids.dtype not in _IDS_CODE:
        raise TypeError(f"nf4_embedding_bnb: ids dtype {getattr(ids, 'dtype', type(ids))} is not supported, "
                        f"expected torch.int32 or torch.int64")
    if ids.device != dev:
        raise RuntimeError(f"nf4_embedding_bnb: ids on '{ids.device}', weight on '{dev}': both must be on the "
                           f"same device")
    code = _dtype_code(qs.dtype)
    if qweight.dtype != torch.uint8:
        raise TypeError(f"nf4_embedding_bnb: packed weight dtype {qweight.dtype} is not supported, expected "
                        f"torch.uint8")
    if qweight.numel() < (rows * dim + 1) // 2:
        raise RuntimeError(f"nf4_embedding_bnb: packed weight has {qweight.numel()} bytes, [{rows}, {dim}] "
                           f"needs {(rows * dim + 1) // 2}")
    want = tuple(ids.shape) + (dim,)
    if out is None:
        out = torch.empty(want, dtype=qs.dtype, device=dev)
    elif (tuple(out.shape) != want or out.dtype != qs.dtype or out.device != dev or not out.is_contiguous()):
        raise ValueError(f"nf4_embedding_bnb: out must be a contiguous {qs.dtype} tensor of shape {want} on "
                         f"'{dev}', got {out.dtype} {tuple(out.shape)} on '{out.device}'")
    count = ids.numel()
    if count == 0 or dim == 0:
        return out
    keep = []  # every temporary outlives the call
    idc = ids.contiguous()
    L = _lib.lib()
    stats = _bnb_stats("nf4_embedding_bnb", qs, dev, keep)
    if not nested:
        stats = (stats[3], stats[4], bs)  # the single entries take (absmax, its count, blocksize) alone
    args = (idc.data_ptr(), _IDS_CODE[idc.dtype], count, _operand(qweight, None, keep)[0], *stats, out.data_ptr(), code,
            rows, dim)
    entry = "nf4_embedding_bnb" if nested else "nf4_embedding_bnb_single"
    if on_host:
        _lib.check(getattr(L, entry + "_cpu")(*args, cpu_threads()), "nf4 embedding")
    else:
        _stream_call("nf4 embedding", dev, getattr(L, entry), *args)
    return out


# (device index, raw stream handle) -> (workspace, the torch stream object): holding the
# stream object keeps a torch-created stream alive for the cache's lifetime, so the
# check below never hands HIP a dangling handle (an ExternalStream's owner must keep
# its stream alive while nf4_linear has a workspace for it, or call
# release_gemm_workspaces() first)
_GEMM_WS = {}


def _same_device(x: torch.Tensor, w: torch.Tensor) -> None:
    # what `x @ W.t()` raises for tensors on different devices (never hand a host
    # or foreign-device pointer to the kernel)
    if x.device != w.device:
        raise _two_devices(w.device, x.device)


def _workspace(cache: dict, device: torch.device, nbytes: int, floor: int) -> torch.Tensor:
    """Zero-filled workspace of ``cache``, one per (device, stream), grown on demand (``floor``: the
    smallest allocation)."""
    key = (device.index, _raw_stream(device.index))
    ent = cache.get(key)
    if ent is None or ent[0].numel() < nbytes:
        ent = cache[key] = (torch.zeros(max(nbytes, floor), dtype=torch.uint8, device=device),
                            torch.cuda.current_stream(device))
    return ent[0]


def _gemm_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Zero-filled split-K workspace, one per (device, stream), grown on demand.

    The fused kernel leaves its ticket counters at 0 after every call, so the
    buffer stays valid; a new stream gets its own (calls on different streams
    may run concurrently and must not share counters).
    """
    return _workspace(_GEMM_WS, device, nbytes, 1 << 16)


# nf4_moe_down_bnb's workspaces, apart from the shared ones: the launch leaves its 16-bit products
# behind the slabs, where another entry's larger slabs would expect zeros.  Their tickets are 0
# between calls like the shared ones'; a later call of another (P, N, ksplit) may find those
# products in its own slabs, which it overwrites before it reads them (include/nf4_dequant.h).  No
# workgroup of that launch waits for another, so their error word is never set and
# check_gemm_workspaces() has nothing to read in them.
_MOE_DOWN_WS = {}


def _moe_down_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """``_gemm_workspace`` for ``nf4_moe_down_bnb`` alone: one per (device, stream), grown on demand."""
    return _workspace(_MOE_DOWN_WS, device, nbytes, 0)


def _stream_call(what: str, dev, entry, *args) -> None:
    """One entry on the current stream of ``dev``, the tensors' device (not the current one): the stream
    handle is the entry's last argument, a failure raises as ``what``."""
    with torch.cuda.device(dev):
        rc = entry(*args, _raw_stream(dev.index))
    _lib.check(rc, what)


def _fused_call(what: str, dev, entry, args, size, size_args, workspace=_gemm_workspace, cfg=(None,)) -> None:
    """The one launch of a fused route, on ``dev``: ask ``size(*size_args)`` for the workspace bytes, take
    the current stream's workspace (null when the entry wants none), and call ``entry`` with ``args``,
    then the workspace, its size, the plan override ``cfg`` (none; ``()`` for an entry without the
    argument) and the current stream's handle.  Whatever ``args`` points to is the caller's to hold."""
    with torch.cuda.device(dev):
        ws_bytes = size(*size_args)
        wp = workspace(dev, ws_bytes).data_ptr() if ws_bytes else None
        rc = entry(*args, wp, ws_bytes, *cfg, _raw_stream(dev.index))
    _lib.check(rc, what)


def _lead_rows(x: torch.Tensor, K: int) -> tuple:
    """x's leading dims and its row count as a ``[M, K]`` matrix."""
    return x.shape[:-1], (x.numel() // K if K else 0)


def _rows(x: torch.Tensor, K: int, dtype: torch.dtype, align16: bool) -> torch.Tensor:
    """x as an entry reads it: ``[M, K]``, ``dtype``, contiguous and, for the entries that load 16 bytes
    at a time (``align16``), 16-byte aligned -- a view at an odd offset is cloned."""
    xc = x.reshape(-1, K)
    if xc.dtype != dtype:
        xc = xc.to(dtype)
    xc = xc.contiguous()
    if align16 and xc.data_ptr() % 16:
        xc = xc.clone()
    return xc


def _check_out(name: str, out: Optional[torch.Tensor], shape: list, dtype: torch.dtype, dev) -> None:
    if out is not None and (list(out.shape) != shape or out.dtype != dtype or out.device != dev
                            or not out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous {dtype} {shape} tensor on {dev}")


def _into(out: Optional[torch.Tensor], value: torch.Tensor) -> torch.Tensor:
    """``value``, copied into ``out`` when the caller gave one."""
    return value if out is None else out.copy_(value)


def release_gemm_workspaces() -> None:
    """Forget every cached split-K workspace: for callers that destroy their own external
    streams.  Each workspace's sticky error word is read first (which also waits for its
    stream), so a split-K timeout since the last ``check_gemm_workspaces()`` is not lost
    with the workspace: the cache is cleared either way, then RuntimeError is raised as
    ``check_gemm_workspaces`` would."""
    try:
        check_gemm_workspaces()
    finally:
        _GEMM_WS.clear()
        _MOE_DOWN_WS.clear()


def check_gemm_workspaces() -> None:
    """Raise if a fused-GEMM split-K reduction gave up waiting since the last check.

    Waits for every stream that owns one of ``nf4_linear``'s cached workspaces and reads
    its sticky error word (``nf4_gemm_check_workspace``); a stalled K slice
    makes the reducer emit NaN for the missing partial and set the word.  The library
    re-zeroes such a workspace, so the next call starts clean.  Raises RuntimeError
    naming the device and stream; returns None when every workspace is clean.
    """
    bad = []
    L = _lib.lib() if _GEMM_WS else None
    for (dev_index, handle), (ws, stream) in list(_GEMM_WS.items()):
        with torch.cuda.device(dev_index):  # the HIP calls run on the workspace's device
            rc = L.nf4_gemm_check_workspace(ws.data_ptr(), ws.numel(), stream.cuda_stream)
        if rc:
            bad.append(f"cuda:{dev_index} stream {handle:#x}: {_lib.strerror(rc)}")
    if bad:
        raise RuntimeError("nf4 fused GEMM: " + "; ".join(bad))


def nf4_linear(x: torch.Tensor, module, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x @ W.t() (+ bias)`` for an NF4 ``Linear4bit`` weight W (reference semantics).

    The consumer of the reference harness (benchmark.py:61-66,
    ``X @ triton_dequantize_nf4(W).t()``).  Decode-shaped inputs (at most
    ``NF4DQ_GEMM_MAX_M`` rows, N % 64 == 0, K % 128 == 0, uint8 absmax) run the
    fused kernel: the 4-bit weight is read once and dequantized in registers
    into exactly the bf16/fp16 values ``triton_dequantize_nf4`` returns, then
    multiplied on MFMA with fp32 accumulation.  Anything else dequantizes with
    the HIP kernel and multiplies with torch (hipBLASLt).  Output dtype =
    ``quant_state.dtype``; ``x`` is cast to it first, as the reference harness's
    inputs already are.
    """
    qweight, absmax, absmax32, dtype, m, n = _prepare(module)
    if qweight.device.type != "cuda" and backend() != "cpu":
        _require_device(qweight)
    _same_device(x, qweight)
    N, K = m, n
    if x.shape[-1] != K:
        raise RuntimeError(f"nf4_linear: x has {x.shape[-1]} features, weight expects {K}")
    lead, M = _lead_rows(x, K)
    fused = (qweight.device.type == "cuda" and dtype in (torch.float16, torch.bfloat16)
             and absmax.dtype == torch.uint8 and 0 < M <= _lib.GEMM_MAX_M
             and N % 64 == 0 and K % 128 == 0 and qweight.numel() * qweight.element_size() == N * K // 2
             and qweight.dtype == torch.uint8)
    if not fused:
        w = triton_dequantize_nf4(module)
        y = x.to(dtype) @ w.t()
    else:
        dev = qweight.device
        xc = _rows(x, K, dtype, False)
        y = torch.empty((M, N), dtype=dtype, device=dev)
        _on_device(dev, absmax, absmax32)
        L = _lib.lib()
        keep = []
        args = (xc.data_ptr(), M, *_operand(qweight, None, keep), *_ref_stats(absmax, absmax32, keep), y.data_ptr(),
                _dtype_code(dtype), N, K)
        _fused_call("nf4 fused gemm", dev, L.nf4_gemm_ref, args, L.nf4_gemm_workspace_bytes, (M, N, K), cfg=())
        y = y.reshape(*lead, N)
    if bias is not None:
        y = y + bias.to(y.dtype)
    return y.reshape(*lead, N)


# Rows up to which nf4_linear_bnb routes to the row-tiled entry (nf4_gemm_bnb_mt*): the largest
# M of {64, 96, 128} at which it measured faster than both dequantize + matmul and ceil(M / 32)
# nf4_gemm_bnb calls on row slices at 4096^2, 14336x4096 and 4096x14336 by more than the
# run-to-run spread (profiles/gemm_mt/).  That holds at 128 rows (narrowly at
# 4096^2: 34.6 against 35.4 us for the slices, spread 0.3 %).  Below it the entry beats the
# composite -- the only other route this function has -- at every measured M and shape, but at
# 64 and 96 rows the row slices, a C-ABI route, are faster where K = 4096.
GEMM_MT_ROUTED_M = 128


def _bnb_gemm_blocksizes(qs) -> bool:
    """The statistics block sizes the fused bnb GEMM takes: blocksize a power of two in
    64..4096 and, when nested, blocksize2 a power of two >= 4 (others dequantize + matmul)."""
    bs = int(qs.blocksize)
    if bs < 64 or bs > 4096 or bs & (bs - 1):
        return False
    if _bnb_nested(qs):
        bs2 = int(qs.state2.blocksize)
        return bs2 >= 4 and not bs2 & (bs2 - 1)
    return True


def nf4_linear_bnb(x: torch.Tensor, module, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x @ W.t() (+ bias)`` for a ``Linear4bit`` weight W in bitsandbytes semantics.

    W is what ``dequantize_nf4_bnb(module)`` returns, bit for bit: nested statistics
    (``code2[absmax] * absmax2 + offset``) or plain fp32 ``absmax``
    (``compress_statistics=False``), chosen as ``dequantize_nf4_bnb`` chooses.  Decode-shaped
    inputs run ONE fused launch (``nf4_gemm_bnb`` / ``nf4_gemm_bnb_single``): the 4-bit
    weight is read once, dequantized in registers and multiplied with fp32 accumulation;
    ``offset`` is read on the device, so the call never synchronises with the host.  The
    fused path is taken when the weight is on a GPU, ``quant_state.dtype`` is fp16 or bf16,
    0 < M <= ``GEMM_MAX_M`` rows, N % 64 == 0, K % 128 == 0, the packed weight is uint8 of
    N * K / 2 bytes, ``quant_type`` is nf4 and no gradient is being recorded for ``x`` (the
    fused call is not differentiable).  ``GEMM_MAX_M`` < M <= ``GEMM_MT_ROUTED_M`` rows
    (batched decode, a speculative verify step, a short prompt) take the row-tiled entry
    (``nf4_gemm_bnb_mt`` / ``nf4_gemm_bnb_mt_single``) under the same rules when ``blocksize``
    is 64: again one launch, no host read of the offset, capturable.  Everything else --
    a gradient being recorded for ``x``, other block sizes above ``GEMM_MAX_M`` rows, CPU
    tensors, more rows than ``GEMM_MT_ROUTED_M`` -- dequantizes with the HIP kernel and
    multiplies with torch, which autograd follows.  All paths use the same weights and fp32
    accumulation; the summation order differs, so the last bit of ``y`` may.
    """
    weight = module.weight
    qs = weight.quant_state
    qweight = weight.data
    dtype = qs.dtype
    N, K = int(module.out_features), int(module.in_features)
    if qweight.device.type == "cuda":
        _same_device(x, qweight)
    if x.shape[-1] != K:
        raise RuntimeError(f"nf4_linear_bnb: x has {x.shape[-1]} features, weight expects {K}")
    lead, M = _lead_rows(x, K)
    fused = (qweight.device.type == "cuda" and dtype in (torch.float16, torch.bfloat16)
             and 0 < M <= GEMM_MT_ROUTED_M and N % 64 == 0 and K % 128 == 0
             and qweight.dtype == torch.uint8 and qweight.numel() == N * K // 2
             and getattr(qs, "quant_type", None) == "nf4" and _bnb_gemm_blocksizes(qs)
             and not (torch.is_grad_enabled() and x.requires_grad))
    # above GEMM_MAX_M rows: the row-tiled entry, which takes blocksize 64 alone
    mt = fused and M > _lib.GEMM_MAX_M
    if mt and not (int(qs.blocksize) == 64 and N >= 64 and K >= 128 and qweight.data_ptr() % 16 == 0):
        fused = False  # (the entry loads 16 bytes at a time: a weight view at an odd offset dequantizes)
    if not fused:
        w = dequantize_nf4_bnb(module)
        y = x.to(w.dtype) @ w.t()
    else:
        dev = qweight.device
        xc = _rows(x, K, dtype, mt)  # the row-tiled entry alone loads 16 bytes at a time
        y = torch.empty((M, N), dtype=dtype, device=dev)
        L = _lib.lib()
        keep = []
        entry = "nf4_gemm_bnb_mt" if mt else "nf4_gemm_bnb"
        stats = _bnb_stats("nf4_linear_bnb", qs, dev, keep)
        if not _bnb_nested(qs):
            entry += "_single"
            stats = (stats[3], stats[4], stats[6])  # the single entries take (absmax, its count, blocksize) alone
        args = (xc.data_ptr(), M, *_operand(qweight, None, keep), *stats, y.data_ptr(), _dtype_code(dtype), N, K)
        _fused_call("nf4 fused bnb gemm", dev, getattr(L, entry), args,
                    L.nf4_gemm_bnb_mt_workspace_bytes if mt else L.nf4_gemm_bnb_workspace_bytes, (M, N, K, None))
        y = y.reshape(*lead, N)
    if bias is not None:
        y = y + bias.to(y.dtype)
    return y


def nf4_linear_grouped(x: torch.Tensor, modules: Sequence, biases: Optional[Sequence] = None) -> List[torch.Tensor]:
    """``[x @ W_i.t() (+ b_i)]`` for NF4 weights W_i that share the input x (q/k/v, gate/up).

    One fused launch for all of them (``nf4_gemm_ref_grouped``) when every
    weight meets ``nf4_linear``'s fused-path rules, has the same ``in_features``
    and output dtype, and there are at most ``GEMM_GROUP_MAX`` of them;
    otherwise each goes through ``nf4_linear``.  Results are the same values
    ``nf4_linear`` gives per weight (same dequantized weights, fp32
    accumulation; the summation order may differ).
    """
    modules = list(modules)
    biases = list(biases) if biases is not None else [None] * len(modules)
    if len(biases) != len(modules):
        raise ValueError("nf4_linear_grouped: one bias (or None) per module")
    if not modules:
        return []
    preps = [_prepare(mod) for mod in modules]
    K = x.shape[-1]
    lead, M = _lead_rows(x, K)
    dtype = preps[0][3]
    dev = preps[0][0].device
    grouped = 1 < len(modules) <= _lib.GEMM_GROUP_MAX and 0 < M <= _lib.GEMM_MAX_M and K % 128 == 0
    for (q, a1, _a2, dt, m, n) in preps:
        grouped = grouped and (dt == dtype and dt in (torch.float16, torch.bfloat16) and n == K and m % 64 == 0
                               and a1.dtype == torch.uint8 and q.dtype == torch.uint8 and q.device == dev
                               and q.numel() == m * K // 2)
    if not grouped:
        return [nf4_linear(x, mod, bias=b) for mod, b in zip(modules, biases)]
    _require_device(preps[0][0])
    _same_device(x, preps[0][0])
    xc = _rows(x, K, dtype, False)
    # keep: the contiguous copies (when q / a1 / a2 are strided views) must outlive the launch -- the
    # caching allocator would hand their blocks to the next torch.empty
    ys, keep = [], []
    mats = (_lib.GemmMat * len(modules))()
    for i, (q, a1, a2, _dt, m, _n) in enumerate(preps):
        _on_device(dev, a1, a2)
        y = torch.empty((M, m), dtype=dtype, device=dev)
        mats[i] = _lib.GemmMat(*_operand(q, None, keep), *_ref_stats(a1, a2, keep), y.data_ptr(), m)
        ys.append(y)
    L = _lib.lib()
    _fused_call("nf4 fused grouped gemm", dev, L.nf4_gemm_ref_grouped,
                (xc.data_ptr(), M, K, mats, len(modules), _dtype_code(dtype)),
                L.nf4_gemm_grouped_workspace_bytes, (M, K, mats, len(modules), None))
    out = []
    for y, b, (_q, _a1, _a2, _dt, m, _n) in zip(ys, biases, preps):
        if b is not None:
            y = y + b.to(y.dtype)
        out.append(y.reshape(*lead, m))
    return out


def nf4_linear_bnb_grouped(x: torch.Tensor, modules: Sequence,
                           biases: Optional[Sequence] = None) -> List[torch.Tensor]:
    """``[x @ W_i.t() (+ b_i)]`` for ``Linear4bit`` weights W_i in bitsandbytes semantics that
    share the input x (q/k/v, gate/up): what ``nf4_linear_bnb`` gives per weight, in ONE fused
    launch (``nf4_gemm_bnb_grouped``).

    The fused launch is taken when there are more than one and at most ``GEMM_GROUP_MAX``
    modules, every module meets ``nf4_linear_bnb``'s fused-path rules, all share
    ``in_features``, ``quant_state.dtype`` and the device, all have nested statistics or all
    plain fp32 ``absmax``, and no gradient is being recorded for ``x``.  Each weight keeps its
    own ``code2`` table, ``offset`` (read on the device: the call never synchronises with the
    host), ``blocksize`` and ``blocksize2``.  Otherwise every module goes through
    ``nf4_linear_bnb``, which keeps autograd and every odd shape working.  The weights are the
    same bit for bit on both routes; the summation order may differ.
    """
    modules = list(modules)
    biases = list(biases) if biases is not None else [None] * len(modules)
    if len(biases) != len(modules):
        raise ValueError("nf4_linear_bnb_grouped: one bias (or None) per module")
    if not modules:
        return []
    K = int(modules[0].in_features)
    lead = x.shape[:-1]
    M = x.numel() // K if K and x.shape[-1] == K else 0
    qs0 = modules[0].weight.quant_state
    dtype, dev = qs0.dtype, modules[0].weight.data.device
    nested = _bnb_nested(qs0)
    grouped = (1 < len(modules) <= _lib.GEMM_GROUP_MAX and dev.type == "cuda" and x.device == dev
               and dtype in (torch.float16, torch.bfloat16) and 0 < M <= _lib.GEMM_MAX_M and K % 128 == 0
               and not (torch.is_grad_enabled() and x.requires_grad))
    for mod in modules:
        if not grouped:
            break
        q, qs, N = mod.weight.data, mod.weight.quant_state, int(mod.out_features)
        grouped = (int(mod.in_features) == K and qs.dtype == dtype and q.device == dev and N % 64 == 0
                   and q.dtype == torch.uint8 and q.numel() == N * K // 2
                   and getattr(qs, "quant_type", None) == "nf4" and _bnb_gemm_blocksizes(qs)
                   and _bnb_nested(qs) == nested)
    if not grouped:
        return [nf4_linear_bnb(x, mod, b) for mod, b in zip(modules, biases)]
    xc = _rows(x, K, dtype, False)
    ys, keep = [], []  # keep: every temporary outlives the enqueue (the caching allocator reuses freed blocks)
    mats = (_lib.GemmBnbMat * len(modules))()
    for i, mod in enumerate(modules):
        ys.append(torch.empty((M, int(mod.out_features)), dtype=dtype, device=dev))
        mats[i] = _bnb_mat("nf4_linear_bnb_grouped", mod, dev, ys[i].data_ptr(), keep)
    L = _lib.lib()
    mp = ctypes.cast(mats, ctypes.c_void_p)
    single = 0 if nested else 1
    _fused_call("nf4 fused grouped bnb gemm", dev, L.nf4_gemm_bnb_grouped,
                (xc.data_ptr(), M, K, mp, len(modules), single, _dtype_code(dtype)),
                L.nf4_gemm_bnb_grouped_workspace_bytes, (M, K, mp, len(modules), single, None))
    del keep
    out = []
    for y, b, mod in zip(ys, biases, modules):
        if b is not None:
            y = y + b.to(y.dtype)
        out.append(y.reshape(*lead, int(mod.out_features)))
    return out


def _moe_fallback(x3: torch.Tensor, experts, ids: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """The per-expert loop over ``nf4_linear_bnb(x[idx], experts.expert(e))``.  It SYNCHRONISES
    with the host: ``nonzero`` reads the routing back once per expert, so this route cannot be
    captured in a graph.  Pairs whose id is outside ``0..E-1`` keep their rows of zeros."""
    T, k = ids.shape
    out.zero_()
    flat = out.view(T * k, out.shape[-1])
    xs = x3.expand(T, k, x3.shape[-1]).reshape(T * k, x3.shape[-1])
    idf = ids.reshape(-1)
    for e in range(experts.num_experts):
        idx = (idf == e).nonzero().reshape(-1)  # host synchronisation
        if idx.numel():
            flat[idx] = nf4_linear_bnb(xs[idx], experts.expert(e)).to(flat.dtype)
    return out


def _moe_args(name: str, x: torch.Tensor, experts, expert_ids: torch.Tensor):
    """The argument checks of the expert entries: ``(T, k, x_div, x as [T, 1 or k, K])``."""
    K = int(experts.in_features)
    dev = experts.weight.data.device
    if expert_ids.dim() != 2 or expert_ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: expert_ids must be int32 or int64 [T, k], got {expert_ids.dtype} "
                         f"{tuple(expert_ids.shape)}")
    T, k = int(expert_ids.shape[0]), int(expert_ids.shape[1])
    if x.dim() == 2 and tuple(x.shape) == (T, K):
        x_div, x3 = k, x.unsqueeze(1)
    elif x.dim() == 3 and tuple(x.shape) == (T, k, K):
        x_div, x3 = 1, x
    else:
        raise RuntimeError(f"{name}: x must be [{T}, {K}] or [{T}, {k}, {K}], got {tuple(x.shape)}")
    if x.device != dev or expert_ids.device != dev:
        raise _two_devices(dev, x.device if x.device != dev else expert_ids.device)
    return T, k, x_div, x3


def _moe_fusable(x: torch.Tensor, experts, P: int, max_pairs: int = _lib.MOE_MAX_PAIRS) -> bool:
    """The fused-route conditions of the expert entries on one ``Experts4bit`` (nf4_moe_linear_bnb's docstring);
    ``max_pairs``: the entry's pair bound."""
    N, K, E = int(experts.out_features), int(experts.in_features), int(experts.num_experts)
    q = experts.weight.data
    return (q.device.type == "cuda" and experts.dtype in (torch.float16, torch.bfloat16) and 1 <= P <= max_pairs
            and N % 64 == 0 and N >= 64 and K % 128 == 0 and K >= 128 and 1 <= E <= _lib.MOE_MAX_EXPERTS
            and int(experts.blocksize) == 64 and q.dtype == torch.uint8 and q.is_contiguous()
            and q.data_ptr() % 16 == 0 and (N * K // 2) % 16 == 0
            and not (torch.is_grad_enabled() and x.requires_grad))


def _moe_operands(x: torch.Tensor, expert_ids: torch.Tensor, dtype: torch.dtype):
    """x and the ids as the expert entries read them: the dtype, contiguous, x 16-byte aligned, int32 ids."""
    ids = expert_ids if expert_ids.dtype == torch.int32 else expert_ids.to(torch.int32)
    return _rows(x, x.shape[-1], dtype, True), ids.contiguous()


def _moe_desc(experts) -> "_lib.MoeExperts":
    """The nf4_moe_experts descriptor of an ``Experts4bit``: base pointers and strides."""
    N, K, E = int(experts.out_features), int(experts.in_features), int(experts.num_experts)
    q = experts.weight.data
    dev = q.device
    _on_device(dev, experts.absmax)
    am = experts.absmax
    if bool(experts.nested):
        _on_device(dev, experts.absmax2, experts.code2, experts.offset)
        return _lib.MoeExperts(q.data_ptr(), q.stride(0), am.data_ptr(), am.stride(0), experts.code2.data_ptr(), 0,
                               experts.absmax2.data_ptr(), experts.absmax2.stride(0), experts.offset.data_ptr(),
                               N, K, E, 0, 64, int(experts.blocksize2))
    return _lib.MoeExperts(q.data_ptr(), q.stride(0), None, 0, None, 0, am.data_ptr(), am.stride(0), None,
                           N, K, E, 1, 64, 0)


# (token, choice) pairs at which nf4_moe_linear_bnb takes the row-block launch (nf4_gemm_bnb_moe_rb)
# in place of nf4_gemm_bnb_moe, whose domain ends at MOE_MAX_PAIRS.  The range is the entry's
# CAPABILITY, as 1 .. MOE_MAX_PAIRS is nf4_gemm_bnb_moe's, not a measured win: past 128 pairs the
# alternative is the per-expert loop, which synchronises with the host once per expert and cannot be
# captured in a graph at all.  What the launch costs against that loop in its best case and against
# ceil(P / 128) nf4_gemm_bnb_moe launches is in profiles/gemm_moe_rb/ (tools/bench_moe_rb.py).
MOE_RB_ROUTED_MIN_P = 129
MOE_RB_ROUTED_MAX_P = 1024


def nf4_moe_linear_bnb(x: torch.Tensor, experts, expert_ids: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One projection of a mixture-of-experts block for all experts, in bitsandbytes semantics:
    ``y[t, j] = x[t] @ W_e.t()`` with ``e = expert_ids[t, j]`` and ``W_e`` what
    ``dequantize_nf4_bnb(experts.expert(e))`` returns, bit for bit.

    ``experts`` is an ``Experts4bit``; ``expert_ids`` is ``[T, k]``, int32 or int64, on x's
    device; ``x`` is ``[T, K]`` (the token's hidden state, shared by its k choices: Mixtral's w1
    and w3) or ``[T, k, K]`` (per-pair activations: w2).  Returns ``[T, k, N]`` in ``experts.dtype``
    (written into ``out`` when given: contiguous, that shape and dtype).  A pair whose id is
    outside ``0..E-1`` gets a row of zeros, as ``nf4_embedding_bnb`` treats an id outside the
    table; one token may name the same expert twice.

    The fused route -- GPU tensors, fp16 / bf16, ``1 <= T*k <= MOE_RB_ROUTED_MAX_P``, N % 64 == 0,
    K % 128 == 0 and no gradient being recorded for ``x`` -- is ONE launch plus at most a cast of
    the ids to int32: ``nf4_gemm_bnb_moe`` up to ``MOE_MAX_PAIRS`` pairs, ``nf4_gemm_bnb_moe_rb``
    (the same kernel over row blocks of 128 of an expert's pairs) for ``MOE_RB_ROUTED_MIN_P <= T*k
    <= MOE_RB_ROUTED_MAX_P``.  The ids and the offsets are
    read on the device, never by the host, so ``torch.cuda.graph`` captures the call and a replay
    follows whatever the router wrote into ``expert_ids`` since.  An expert without a pair costs
    no weight traffic.  Everything else (more than ``MOE_RB_ROUTED_MAX_P`` pairs, CPU tensors, a
    gradient for ``x``) takes the
    per-expert loop over ``nf4_linear_bnb(x[idx], experts.expert(e))``, which SYNCHRONISES with
    the host once per expert (it reads the routing back) and is therefore not capturable; autograd
    follows it to ``x``.  Both routes use the same weights and fp32 accumulation; the summation
    order differs, so the last bit of ``y`` may.
    """
    N, K = int(experts.out_features), int(experts.in_features)
    dtype = experts.dtype
    dev = experts.weight.data.device
    T, k, x_div, x3 = _moe_args("nf4_moe_linear_bnb", x, experts, expert_ids)
    _check_out("nf4_moe_linear_bnb", out, [T, k, N], dtype, dev)
    if out is None:
        out = torch.empty((T, k, N), dtype=dtype, device=dev)
    P = T * k
    if P == 0:
        return out
    row_blocks = MOE_RB_ROUTED_MIN_P <= P <= MOE_RB_ROUTED_MAX_P
    if not _moe_fusable(x, experts, P, _lib.MOE_RB_MAX_PAIRS if row_blocks else _lib.MOE_MAX_PAIRS):
        return _moe_fallback(x3, experts, expert_ids, out)
    xc, ids = _moe_operands(x, expert_ids, dtype)
    desc = _moe_desc(experts)
    L = _lib.lib()
    size, entry = ((L.nf4_gemm_bnb_moe_rb_workspace_bytes, L.nf4_gemm_bnb_moe_rb) if row_blocks
                   else (L.nf4_gemm_bnb_moe_workspace_bytes, L.nf4_gemm_bnb_moe))
    dp = ctypes.cast(ctypes.pointer(desc), ctypes.c_void_p)
    _fused_call("nf4 fused moe gemm", dev, entry,
                (xc.data_ptr(), ids.data_ptr(), P, x_div, dp, out.data_ptr(), _dtype_code(dtype)), size, (P, dp, None))
    return out


# Rows at which nf4_swiglu_bnb takes the fused launch (nf4_gemm_bnb_mt_swiglu): exactly those M
# of {1, 8, 32, 33, 48, 64, 96, 128} at which it measured faster than what a caller did before --
# nf4_linear_bnb_grouped, then F.silu(g) * u: one grouped launch up to 32 rows, two row-tiled
# launches above, two elementwise launches either way -- at 14336x4096 and at 11008x4096 by more
# than the run-to-run spread of the rounds (profiles/gemm_mt_swiglu/).  That holds
# from 33 rows up (1.42x - 1.64x at 48 .. 128 rows) and fails up to 32, where the grouped
# small-M launch and its two elementwise launches take half to two thirds of the fused launch's
# time: the row-tiled anatomy is the slower one there.  An empty range (MIN above MAX) would mean
# the fused launch is reached through the C entry alone.
SWIGLU_ROUTED_MIN_M = 33
SWIGLU_ROUTED_MAX_M = 128


def _swiglu_fused(x: torch.Tensor, gate_proj, up_proj, M: int, I: int, K: int) -> bool:
    """nf4_swiglu_bnb's fused-path rules (its docstring)."""
    qg, qu = gate_proj.weight.data, up_proj.weight.data
    sg, su = gate_proj.weight.quant_state, up_proj.weight.quant_state
    dev = qg.device
    if not (dev.type == "cuda" and qu.device == dev and x.device == dev and sg.dtype == su.dtype
            and sg.dtype in (torch.float16, torch.bfloat16)
            and SWIGLU_ROUTED_MIN_M <= M <= min(SWIGLU_ROUTED_MAX_M, _lib.GEMM_MT_MAX_M) and M >= 1
            and I % 64 == 0 and I >= 64 and K % 128 == 0 and K >= 128
            and getattr(gate_proj, "bias", None) is None and getattr(up_proj, "bias", None) is None
            and not (torch.is_grad_enabled() and x.requires_grad)):
        return False
    for q, qs in ((qg, sg), (qu, su)):
        if not (getattr(qs, "quant_type", None) == "nf4" and int(qs.blocksize) == 64 and _bnb_gemm_blocksizes(qs)
                and q.dtype == torch.uint8 and q.numel() == I * K // 2 and q.is_contiguous()
                and q.data_ptr() % 16 == 0):
            return False
    return _bnb_nested(sg) == _bnb_nested(su)


def nf4_swiglu_bnb(x: torch.Tensor, gate_proj, up_proj, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.silu(gate_proj(x)) * up_proj(x)`` -- the first half of a Llama-family MLP -- for two
    ``Linear4bit`` weights of one shape ``[I, K]`` in bitsandbytes semantics.  Returns ``[..., I]``
    in ``quant_state.dtype`` (written into ``out`` when given: that shape and dtype).

    The result is the rounding chain of the expression on 16-bit tensors: ``g`` and ``u`` rounded
    to the dtype as ``nf4_linear_bnb`` stores them, ``silu`` in fp32 rounded once, the product
    rounded once.  The fused route is ONE launch (``nf4_gemm_bnb_mt_swiglu``): neither ``g`` nor
    ``u`` makes a trip through memory, the offsets are read on the device, nothing synchronises
    with the host and ``torch.cuda.graph`` captures the call.  It is taken when the weights are
    on a GPU, the dtype is fp16 or bf16, both modules are nf4 with blocksize 64 and the same
    ``[I, K]`` (I % 64 == 0, K % 128 == 0), both have nested statistics or both plain fp32
    ``absmax``, neither has a bias, the packed data is uint8 of I * K / 2 bytes and 16-byte
    aligned, no gradient is being recorded for ``x`` and
    ``SWIGLU_ROUTED_MIN_M <= M <= SWIGLU_ROUTED_MAX_M`` rows.  Everything else -- CPU tensors,
    other row counts, a bias, other block sizes, a recorded gradient -- is
    ``F.silu(g) * u`` with ``g, u = nf4_linear_bnb_grouped(x, [gate_proj, up_proj], biases)``,
    which autograd follows and which has the same definition; the GEMMs' summation order may
    differ between the routes, so the last bit of ``g`` and ``u`` may.
    """
    I, K = int(gate_proj.out_features), int(gate_proj.in_features)
    if (int(up_proj.out_features), int(up_proj.in_features)) != (I, K):
        raise RuntimeError(f"nf4_swiglu_bnb: gate_proj is [{I}, {K}], up_proj "
                           f"[{int(up_proj.out_features)}, {int(up_proj.in_features)}]")
    if x.shape[-1] != K:
        raise RuntimeError(f"nf4_swiglu_bnb: x has {x.shape[-1]} features, the weights expect {K}")
    lead, M = _lead_rows(x, K)
    dtype = gate_proj.weight.quant_state.dtype
    dev = gate_proj.weight.data.device
    _check_out("nf4_swiglu_bnb", out, [*lead, I], dtype, x.device)
    if not _swiglu_fused(x, gate_proj, up_proj, M, I, K):
        g, u = nf4_linear_bnb_grouped(x, [gate_proj, up_proj],
                                      [getattr(gate_proj, "bias", None), getattr(up_proj, "bias", None)])
        return _into(out, torch.nn.functional.silu(g) * u)
    xc = _rows(x, K, dtype, True)
    h = out if out is not None else torch.empty((*lead, I), dtype=dtype, device=dev)
    keep = []  # every temporary outlives the enqueue (the caching allocator reuses freed blocks)
    # the descriptors of nf4_linear_bnb_grouped, without an output of their own
    mats = (_lib.GemmBnbMat * 2)(*[_bnb_mat("nf4_swiglu_bnb", mod, dev, None, keep) for mod in (gate_proj, up_proj)])
    L = _lib.lib()
    _fused_call("nf4 fused swiglu gemm", dev, L.nf4_gemm_bnb_mt_swiglu,
                (xc.data_ptr(), M, K, ctypes.cast(mats, ctypes.c_void_p),
                 0 if _bnb_nested(gate_proj.weight.quant_state) else 1, _lib.ACT_SILU, h.data_ptr(), _dtype_code(dtype)),
                L.nf4_gemm_bnb_mt_swiglu_workspace_bytes, (M, I, K, None))
    del keep
    return h


def nf4_mlp_bnb(x: torch.Tensor, gate_proj, up_proj, down_proj) -> torch.Tensor:
    """``down_proj(F.silu(gate_proj(x)) * up_proj(x))`` for ``Linear4bit`` weights in bitsandbytes
    semantics: ``nf4_linear_bnb(nf4_swiglu_bnb(x, gate_proj, up_proj), down_proj)`` and nothing else."""
    return nf4_linear_bnb(nf4_swiglu_bnb(x, gate_proj, up_proj), down_proj)


# (token, choice) pairs at which nf4_moe_swiglu_bnb takes the fused launch (nf4_gemm_bnb_moe_swiglu):
# the span of the T * k of {2, 8, 32, 128} at which it measured faster than what a caller did
# before -- two nf4_moe_linear_bnb launches, then F.silu(g) * u: four launches -- at Mixtral-8x7B's
# w1 / w3 (8 experts, top-2, 14336x4096, bf16, graph replay, weights from HBM) by more than the
# run-to-run spread of the rounds (profiles/gemm_moe_swiglu/, README).  It did at
# all four: 56 against 84 us at 2 pairs (1.49x), 140 / 174 at 8 (1.25x), 185 / 212 at 32 (1.15x),
# 357 / 410 at 128 (1.15x), the slower of two runs of the fused launch against the faster of two
# of the composite, where a route's rounds spread over 1 - 6 us.  One pair was not measured and is
# not routed.  An empty range (MIN above MAX) would mean the fused launch is reached through the C
# entry alone.
MOE_SWIGLU_ROUTED_MIN_P = 2
MOE_SWIGLU_ROUTED_MAX_P = 128


def nf4_moe_swiglu_bnb(x: torch.Tensor, gate_experts, up_experts, expert_ids: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The first half of a mixture-of-experts block, Mixtral's ``F.silu(w1(x)) * w3(x)`` per
    (token, choice) pair, in bitsandbytes semantics:
    ``F.silu(nf4_moe_linear_bnb(x, gate_experts, ids)) * nf4_moe_linear_bnb(x, up_experts, ids)``.

    ``gate_experts`` and ``up_experts`` are ``Experts4bit`` of one shape ``[I, K]``, one expert
    count, one dtype and both with nested statistics or both with fp32 ``absmax`` (else
    ``ValueError``); ``expert_ids`` is ``[T, k]``, int32 or int64; ``x`` is ``[T, K]`` or
    ``[T, k, K]`` -- all as in ``nf4_moe_linear_bnb``, with its checks and errors.  Returns
    ``[T, k, I]`` in the experts' dtype (written into ``out`` when given: contiguous, that shape
    and dtype).  A pair whose id is outside ``0..E-1`` gets a row of zeros.

    The fused route is ONE launch (``nf4_gemm_bnb_moe_swiglu``) plus at most a cast of the ids:
    the ids are balloted and x gathered and staged once for both weights, neither ``g`` nor ``u``
    makes a trip through memory, the ids and the offsets are read on the device, nothing
    synchronises with the host and ``torch.cuda.graph`` captures the call.  It is taken under
    ``nf4_moe_linear_bnb``'s fused-route conditions on both stacks and
    ``MOE_SWIGLU_ROUTED_MIN_P <= T*k <= MOE_SWIGLU_ROUTED_MAX_P``.  Everything else -- other pair
    counts, CPU tensors, a gradient being recorded for ``x`` -- is the expression above, which has
    the same definition and which autograd follows (up to ``MOE_RB_ROUTED_MAX_P`` pairs its two
    ``nf4_moe_linear_bnb`` calls are fused launches themselves, so it stays capturable); the
    GEMMs' summation order may differ between the routes, so the last bit of ``g`` and ``u`` may.
    """
    I, K, E = int(gate_experts.out_features), int(gate_experts.in_features), int(gate_experts.num_experts)
    if ((int(up_experts.out_features), int(up_experts.in_features), int(up_experts.num_experts)) != (I, K, E)
            or up_experts.dtype != gate_experts.dtype or bool(up_experts.nested) != bool(gate_experts.nested)):
        raise ValueError(f"nf4_moe_swiglu_bnb: gate_experts is {E} x [{I}, {K}] {gate_experts.dtype} "
                         f"{'nested' if gate_experts.nested else 'fp32 absmax'}, up_experts "
                         f"{int(up_experts.num_experts)} x [{int(up_experts.out_features)}, {int(up_experts.in_features)}] "
                         f"{up_experts.dtype} {'nested' if up_experts.nested else 'fp32 absmax'}")
    dtype = gate_experts.dtype
    dev = gate_experts.weight.data.device
    T, k, x_div, _ = _moe_args("nf4_moe_swiglu_bnb", x, gate_experts, expert_ids)
    if up_experts.weight.data.device != dev:
        raise _two_devices(dev, up_experts.weight.data.device)
    _check_out("nf4_moe_swiglu_bnb", out, [T, k, I], dtype, dev)
    P = T * k
    fused = (MOE_SWIGLU_ROUTED_MIN_P <= P <= MOE_SWIGLU_ROUTED_MAX_P and _moe_fusable(x, gate_experts, P)
             and _moe_fusable(x, up_experts, P))
    if not fused:
        return _into(out, torch.nn.functional.silu(nf4_moe_linear_bnb(x, gate_experts, expert_ids))
                     * nf4_moe_linear_bnb(x, up_experts, expert_ids))
    if out is None:
        out = torch.empty((T, k, I), dtype=dtype, device=dev)
    xc, ids = _moe_operands(x, expert_ids, dtype)
    descs = (_lib.MoeExperts * 2)(_moe_desc(gate_experts), _moe_desc(up_experts))
    L = _lib.lib()
    dp = ctypes.cast(descs, ctypes.c_void_p)
    _fused_call("nf4 fused moe swiglu gemm", dev, L.nf4_gemm_bnb_moe_swiglu,
                (xc.data_ptr(), ids.data_ptr(), P, x_div, dp, _lib.ACT_SILU, out.data_ptr(), _dtype_code(dtype)),
                L.nf4_gemm_bnb_moe_swiglu_workspace_bytes, (P, dp, None))
    return out


# (token, choice) pairs at which nf4_moe_down_bnb takes the fused launch (nf4_gemm_bnb_moe_down):
# those of the measured T * k in {2, 8, 32, 128} at which it was faster than the composite it
# replaces -- nf4_moe_linear_bnb, then the cast, the product and the sum in torch: four launches --
# at Mixtral-8x7B's w2 (8 experts, top-2, 4096x14336, bf16, graph replay, weights from HBM) by more
# than the run-to-run spread of the rounds (profiles/gemm_moe_down/, README).
# There is none: 65 against 51 us at 2 pairs (0.78x), 111 / 112 at 8 (1.01x, inside the rounds'
# spread of up to 5 us), 123 / 120 at 32 (0.97x), 218 / 215 at 128 (0.98x) -- the slower of two
# runs of the fused launch against the faster of two of the composite.  In a replayed graph the
# three elementwise launches cost about 6 us; the second ticket and the combine behind the last
# reducer cost as much or more.  So the range is EMPTY (MIN above MAX): the fused launch is
# reached through the C entry, or by a caller who sets these constants.
MOE_DOWN_ROUTED_MIN_P = 1
MOE_DOWN_ROUTED_MAX_P = 0

# The largest top-k at which nf4_moe_mlp_bnb calls nf4_moe_down_bnb in place of its last two
# lines: with two fp32 terms the sum is order-free, so the result is bit for bit the torch
# expression's; for k > 2 torch's reduction order is not promised and the last bit could move.
MOE_DOWN_MLP_MAX_K = 2


def _moe_down_chain(d: torch.Tensor, rw: torch.Tensor) -> torch.Tensor:
    """The combine as the fused launch defines it, on tensors: the products in d's dtype, then the
    fp32 sum from +0 in the order j = 0 .. k-1, rounded once.  Up to two terms ``sum`` is that sum
    whatever its order (it accumulates 16-bit inputs in fp32 from +0 and rounds once); beyond, the
    order is spelled out."""
    prod = d * rw.to(d.dtype).unsqueeze(-1)
    if d.shape[1] <= 2:
        return prod.sum(dim=1)
    acc = torch.zeros((d.shape[0], d.shape[2]), dtype=torch.float32, device=d.device)
    for j in range(d.shape[1]):
        acc = acc + prod[:, j].float()
    return acc.to(d.dtype)


def nf4_moe_down_bnb(h: torch.Tensor, experts, expert_ids: torch.Tensor, routing_weights: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The second half of a mixture-of-experts block, Mixtral's ``w2`` with the routed weighted
    sum, in bitsandbytes semantics: ``y[t] = sum_j routing_weights[t, j] * (h[t, j] @ W_e.t())``
    with ``e = expert_ids[t, j]``.

    ``experts``, ``expert_ids`` ``[T, k]`` and ``h`` (``[T, k, K]``, or ``[T, K]`` shared by the
    token's choices) are as in ``nf4_moe_linear_bnb``, with its checks and errors;
    ``routing_weights`` is ``[T, k]`` in any float dtype on the same device.  Returns ``[T, N]``
    in the experts' dtype (written into ``out`` when given: contiguous, that shape and dtype).

    The result is this chain, with ``rn`` the rounding to the experts' dtype: ``d =
    nf4_moe_linear_bnb(h, experts, expert_ids)`` (rows of zeros for ids outside ``0..E-1``),
    ``p[t, j] = rn(d[t, j] * rn(routing_weights[t, j]))`` (the fp32 product of two 16-bit values
    is exact), ``y[t] = rn(p[t, 0] + p[t, 1] + ...)`` summed in fp32 from +0 in the order
    ``j = 0 .. k-1``.  For ``k <= 2`` that equals
    ``(d * routing_weights.to(d.dtype).unsqueeze(-1)).sum(dim=1)`` bit for bit: a sum of two fp32
    terms is order-free.  For ``k > 2`` torch's reduction order is not promised, so the last bit
    may differ from that expression.

    The fused route is ONE launch (``nf4_gemm_bnb_moe_down``) plus at most casts of the ids and
    the weights: ``d`` never leaves the launch's workspace, nothing synchronises with the host and
    ``torch.cuda.graph`` captures the call.  fp32 weights and weights in the experts' dtype go to
    the kernel as they are; any other dtype is cast to the experts' dtype first.  It is taken
    exactly where ``nf4_moe_linear_bnb`` takes its fused route, when in addition the weights are
    on the device with no gradient being recorded for them and
    ``MOE_DOWN_ROUTED_MIN_P <= T*k <= MOE_DOWN_ROUTED_MAX_P``.  Everything else is the chain above
    on tensors, which autograd follows to ``h`` and to ``routing_weights``; the GEMM's summation
    order may differ between the routes, so the last bit of ``d`` may.
    """
    N = int(experts.out_features)
    dtype = experts.dtype
    dev = experts.weight.data.device
    T, k, x_div, _ = _moe_args("nf4_moe_down_bnb", h, experts, expert_ids)
    if tuple(routing_weights.shape) != (T, k) or not routing_weights.is_floating_point():
        raise ValueError(f"nf4_moe_down_bnb: routing_weights must be a float [{T}, {k}] tensor, got "
                         f"{routing_weights.dtype} {tuple(routing_weights.shape)}")
    if routing_weights.device != dev:
        raise _two_devices(dev, routing_weights.device)
    _check_out("nf4_moe_down_bnb", out, [T, N], dtype, dev)
    P = T * k
    fused = (MOE_DOWN_ROUTED_MIN_P <= P <= MOE_DOWN_ROUTED_MAX_P and _moe_fusable(h, experts, P)
             and not (torch.is_grad_enabled() and routing_weights.requires_grad))
    if not fused:
        if k == 0:
            y = torch.zeros((T, N), dtype=dtype, device=dev)
        else:
            y = _moe_down_chain(nf4_moe_linear_bnb(h, experts, expert_ids), routing_weights)
        return _into(out, y)
    if out is None:
        out = torch.empty((T, N), dtype=dtype, device=dev)
    hc, ids = _moe_operands(h, expert_ids, dtype)
    rw = routing_weights if routing_weights.dtype in (torch.float32, dtype) else routing_weights.to(dtype)
    rw = rw.contiguous()
    desc = _moe_desc(experts)
    L = _lib.lib()
    dp = ctypes.cast(ctypes.pointer(desc), ctypes.c_void_p)
    _fused_call("nf4 fused moe down gemm", dev, L.nf4_gemm_bnb_moe_down,
                (hc.data_ptr(), ids.data_ptr(), P, x_div, k, rw.data_ptr(),
                 _lib.F32 if rw.dtype == torch.float32 else _dtype_code(dtype), dp, out.data_ptr(), _dtype_code(dtype)),
                L.nf4_gemm_bnb_moe_down_workspace_bytes, (P, dp, None), workspace=_moe_down_workspace)
    return out


def nf4_moe_mlp_bnb(x: torch.Tensor, w1, w3, w2, expert_ids: torch.Tensor,
                    routing_weights: torch.Tensor) -> torch.Tensor:
    """A whole mixture-of-experts MLP block (Mixtral's) for ``Experts4bit`` stacks in bitsandbytes
    semantics: ``sum_j routing_weights[t, j] * w2_e(F.silu(w1_e(x[t])) * w3_e(x[t]))`` with
    ``e = expert_ids[t, j]``.  ``x`` is ``[T, H]``, ``expert_ids`` and ``routing_weights``
    ``[T, k]`` (the weights in any float dtype); returns ``[T, H]``.  It has no logic of its own:
    ``nf4_moe_swiglu_bnb``, then ``nf4_moe_down_bnb`` for ``k <= MOE_DOWN_MLP_MAX_K`` (bit for bit
    the two lines below) or ``nf4_moe_linear_bnb`` and the weighted combine in torch, so it is
    capturable in a graph whenever its parts are, and autograd follows it to ``x``."""
    h = nf4_moe_swiglu_bnb(x, w1, w3, expert_ids)
    if 1 <= expert_ids.shape[-1] <= MOE_DOWN_MLP_MAX_K and tuple(routing_weights.shape) == tuple(expert_ids.shape):
        return nf4_moe_down_bnb(h, w2, expert_ids, routing_weights)
    d = nf4_moe_linear_bnb(h, w2, expert_ids)
    return (d * routing_weights.to(d.dtype).unsqueeze(-1)).sum(dim=1)


# Rows at which nf4_linear_lora_bnb and nf4_linear_lora_bnb_grouped take the fused adapter launch
# (nf4_lora_add).  Set from tools/bench_lora.py's measurement and from nothing else: a row count is
# routed only where, at every shape and rank measured, the slower of the launch's two runs beats
# the faster of the composite's two runs by more than the spread of a route's rounds
# (profiles/lora/, README, DESIGN section 4b "The adapter tail").  Measured at 4096^2, 1024x4096,
# 14336x4096 and 4096x14336 with r = 16 and 64: the launch wins 3 of 8 tail cells at one row,
# 3 of 8 at 8, 0 of 8 at 32 and none at 64 or 128 (it wins at r = 16 with K = 4096 and loses at r = 64
# and at K = 14336), so no row count meets the rule: an empty range (MIN above MAX), the launch is
# reached through the C entry alone and both functions take the composite at every row count.
LORA_ROUTED_MIN_M = 1
LORA_ROUTED_MAX_M = 0


def _lora_composite(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scaling: float) -> torch.Tensor:
    """The definition of the adapter tail (PEFT's expression): what autograd follows."""
    t = torch.nn.functional.linear(x.to(A.dtype), A)
    u = torch.nn.functional.linear(t, B)
    return y + (u * scaling).to(y.dtype)


def _adapter_fusable(x: torch.Tensor, module, A: torch.Tensor, B: torch.Tensor, r: int, M: int, min_m: int,
                     max_m: int) -> bool:
    """The fused-path rules the adapter launches share (nf4_linear_lora_bnb's docstring): ``A`` and ``B``
    are an adapter or a stack of rank ``r``, ``min_m .. max_m`` the function's routed rows."""
    dtype = module.weight.quant_state.dtype
    dev = module.weight.data.device
    N, K = int(module.out_features), int(module.in_features)
    return (dev.type == "cuda" and x.device == dev and A.device == dev and B.device == dev
            and dtype in (torch.float16, torch.bfloat16) and A.dtype == dtype and B.dtype == dtype
            and max(1, min_m) <= M <= min(max_m, _lib.LORA_MAX_M)
            and r % 8 == 0 and 8 <= r <= _lib.LORA_MAX_R and K % 32 == 0 and K >= 32 and N % 16 == 0 and N >= 16
            and A.is_contiguous() and B.is_contiguous() and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
            and not (torch.is_grad_enabled() and (x.requires_grad or A.requires_grad or B.requires_grad)))


def _lora_fusable(x: torch.Tensor, module, A: torch.Tensor, B: torch.Tensor, M: int) -> bool:
    """nf4_linear_lora_bnb's fused-path rules (its docstring) for one adapter."""
    if A.dim() != 2 or B.dim() != 2:
        return False
    r = int(A.shape[0])
    return (tuple(A.shape) == (r, int(module.in_features)) and tuple(B.shape) == (int(module.out_features), r)
            and _adapter_fusable(x, module, A, B, r, M, LORA_ROUTED_MIN_M, LORA_ROUTED_MAX_M))


def _lora_add(x: torch.Tensor, M: int, K: int, dtype: torch.dtype, items) -> None:
    """ONE nf4_lora_add launch: ``items`` is [(y [.., N] contiguous, updated in place, A, B, scaling)]."""
    xc = _rows(x, K, dtype, True)
    mats = (_lib.LoraMat * len(items))()
    for i, (y, A, B, scaling) in enumerate(items):
        mats[i] = _lib.LoraMat(A.data_ptr(), B.data_ptr(), y.data_ptr(), y.data_ptr(), int(B.shape[0]),
                               int(A.shape[0]), float(scaling))
    _stream_call("nf4 fused lora add", x.device, _lib.lib().nf4_lora_add, xc.data_ptr(), M, K,
                 ctypes.cast(mats, ctypes.c_void_p), len(items), _dtype_code(dtype), None)


def _lora_base_in_place(y: torch.Tensor, dtype: torch.dtype) -> bool:
    return y.dtype == dtype and y.is_contiguous() and y.data_ptr() % 16 == 0 and not y.requires_grad


def _adapters_grouped(x: torch.Tensor, modules: list, entries: list, biases, fusable, add, composite) -> List[torch.Tensor]:
    """The skeleton of the grouped adapter functions, ``entries[i]`` being module i's adapter or stack
    (None: it has none): the base through ``nf4_linear_bnb_grouped``, then ONE launch -- ``add(M, K, dtype,
    [(y, *entry)])`` -- for all entries that are ``fusable(mod, entry, M)`` and whose base result can
    be updated in place, when there are 1 .. ``LORA_GROUP_MAX`` of them; ``composite(y, entry)`` for
    every other one."""
    ys = nf4_linear_bnb_grouped(x, modules, biases)
    if not modules:
        return ys
    K = int(modules[0].in_features)
    M = x.numel() // K if K and x.shape[-1] == K else 0
    dtype = modules[0].weight.quant_state.dtype
    fused = [e is not None and int(mod.in_features) == K and mod.weight.quant_state.dtype == dtype
             and fusable(mod, e, M) and _lora_base_in_place(y, dtype) for mod, e, y in zip(modules, entries, ys)]
    if not 1 <= sum(fused) <= _lib.LORA_GROUP_MAX:
        fused = [False] * len(modules)
    items = [(y, e[0], e[1], e[2]) for y, e, f in zip(ys, entries, fused) if f]
    if items:
        add(M, K, dtype, items)
    return [y if f or e is None else composite(y, e) for y, e, f in zip(ys, entries, fused)]


def nf4_linear_lora_bnb(x: torch.Tensor, module, lora_A: torch.Tensor, lora_B: torch.Tensor, scaling: float,
                        bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``W x + b + scaling * B (A x)``: a ``Linear4bit`` in bitsandbytes semantics with a low-rank
    (LoRA) adapter, ``lora_A`` ``[r, K]`` and ``lora_B`` ``[N, r]`` (PEFT's ``lora_A.weight`` and
    ``lora_B.weight``).  Its definition, which is also its fallback, is PEFT's expression::

        y = nf4_linear_bnb(x, module, bias)
        t = F.linear(x.to(A.dtype), A)
        u = F.linear(t, B)
        y + (u * scaling).to(y.dtype)

    The fused route runs the base through ``nf4_linear_bnb`` and the whole tail as ONE launch
    (``nf4_lora_add``) that updates the base's result in place, with the rounding chain of the
    expression on 16-bit tensors (``t``, ``u``, the scaled ``u`` and the sum each rounded once);
    nothing synchronises with the host and ``torch.cuda.graph`` captures the call.  It is taken
    when the tensors are on the GPU, the adapter's dtype equals ``quant_state.dtype`` and is fp16
    or bf16, ``K % 32 == 0``, ``N % 16 == 0``, ``r % 8 == 0`` with ``8 <= r <= 128``, the adapter
    is contiguous and 16-byte aligned, ``LORA_ROUTED_MIN_M <= M <= LORA_ROUTED_MAX_M`` rows and no
    gradient is being recorded for ``x``, ``lora_A`` or ``lora_B``.  Everything else -- fp32
    adapters (PEFT's default unless cast), training, CPU tensors, other ranks and row counts --
    takes the composite, which autograd follows.  The summation order of the two products may
    differ between the routes, so the last bits may.
    """
    y = nf4_linear_bnb(x, module, bias)
    K = int(module.in_features)
    M = x.numel() // K if K else 0
    dtype = module.weight.quant_state.dtype
    if not (_lora_fusable(x, module, lora_A, lora_B, M) and _lora_base_in_place(y, dtype)):
        return _lora_composite(y, x, lora_A, lora_B, scaling)
    _lora_add(x, M, K, dtype, [(y, lora_A, lora_B, scaling)])
    return y


def nf4_linear_lora_bnb_grouped(x: torch.Tensor, modules: Sequence, adapters: Sequence,
                                biases: Optional[Sequence] = None) -> List[torch.Tensor]:
    """``nf4_linear_lora_bnb`` for ``Linear4bit`` weights that share the input x (q/k/v, gate/up):
    ``adapters[i]`` is ``(lora_A, lora_B, scaling)`` or ``None`` for a module without one.  The
    base goes through ``nf4_linear_bnb_grouped``; ALL adapters that meet ``nf4_linear_lora_bnb``'s
    fused-path rules go in ONE ``nf4_lora_add`` launch when there are at most ``LORA_GROUP_MAX``
    of them (each updates its module's result in place), every other adapter takes the composite.
    """
    modules = list(modules)
    adapters = list(adapters)
    if len(adapters) != len(modules):
        raise ValueError("nf4_linear_lora_bnb_grouped: one adapter (or None) per module")
    return _adapters_grouped(x, modules, adapters, biases,
                             lambda mod, ad, M: _lora_fusable(x, mod, ad[0], ad[1], M),
                             lambda M, K, dtype, items: _lora_add(x, M, K, dtype, items),
                             lambda y, ad: _lora_composite(y, x, ad[0], ad[1], ad[2]))


# Rows at which nf4_linear_multilora_bnb and nf4_linear_multilora_bnb_grouped take the routed
# adapter launch (nf4_lora_add_routed).  Set from tools/bench_multilora.py's measurement and from
# nothing else, by LORA_ROUTED_*'s rule: a row count is routed only where, at every shape, rank
# and routing measured, the slower of the launch's two runs beats the faster of the composite's
# two runs by more than the spread of a route's rounds (profiles/multilora/, README, DESIGN
# section 4b "The multi-adapter tail").  Measured at 4096^2, 14336x4096 and 4096x14336 with r = 16
# and 64 under three routings (every row its own adapter, 4 adapters uniform, one adapter of 64):
# the launch wins all 18 tail cells and all 18 base-plus-tail cells at each of 1, 8, 32, 64 and 128
# rows (by 1.10x at the least: one row, r = 64, K = 14336), so every row count the entry takes is routed.
MULTILORA_ROUTED_MIN_M = 1
MULTILORA_ROUTED_MAX_M = 128
MULTILORA_CHUNK_ROWS = 32  # rows per gather of the composite: bounds its [rows, r, K] temporary


def _multilora_scaling(scaling, S: int, device) -> torch.Tensor:
    """``scaling`` as an fp32 tensor [S] on ``device`` (a sequence of floats is copied there)."""
    if not isinstance(scaling, torch.Tensor):
        scaling = torch.tensor([float(s) for s in scaling], dtype=torch.float32, device=device)
    if scaling.dim() != 1 or scaling.numel() != S:
        raise ValueError(f"nf4_linear_multilora_bnb: scaling must hold one value per adapter ({S}), got "
                         f"{tuple(scaling.shape)}")
    return scaling


def _multilora_check(x: torch.Tensor, module, A: torch.Tensor, B: torch.Tensor, ids: torch.Tensor) -> int:
    """The argument rules of nf4_linear_multilora_bnb; returns the row count M."""
    N, K = int(module.out_features), int(module.in_features)
    if A.dim() != 3 or B.dim() != 3 or A.shape[0] != B.shape[0] or A.shape[0] < 1:
        raise ValueError(f"nf4_linear_multilora_bnb: lora_A must be [S, r, K] and lora_B [S, N, r], got "
                         f"{tuple(A.shape)} and {tuple(B.shape)}")
    S, r = int(A.shape[0]), int(A.shape[1])
    if tuple(A.shape) != (S, r, K) or tuple(B.shape) != (S, N, r):
        raise ValueError(f"nf4_linear_multilora_bnb: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not fit a "
                         f"[{N}, {K}] weight with {S} adapters of rank {r}")
    if x.shape[-1] != K:
        raise ValueError(f"nf4_linear_multilora_bnb: x has {x.shape[-1]} features, the weight takes {K}")
    M = x.numel() // K
    if ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"nf4_linear_multilora_bnb: adapter_ids must be int32 or int64, got {ids.dtype}")
    if ids.numel() != M:
        raise ValueError(f"nf4_linear_multilora_bnb: {ids.numel()} adapter ids for {M} rows of x")
    return M


def _multilora_composite(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scaling: torch.Tensor,
                         ids: torch.Tensor) -> torch.Tensor:
    """The definition of the multi-adapter tail: what autograd follows.  No host read."""
    S, K, N = int(A.shape[0]), int(A.shape[2]), int(B.shape[1])
    x2 = x.reshape(-1, K).to(A.dtype)
    y2 = y.reshape(-1, N)
    ids = ids.reshape(-1)
    scaling = scaling.to(device=ids.device, dtype=torch.float32)
    valid = (ids >= 0) & (ids < S)
    idc = ids.clamp(0, S - 1).long()
    outs = []
    for i in range(0, x2.shape[0], MULTILORA_CHUNK_ROWS):
        sl = slice(i, i + MULTILORA_CHUNK_ROWS)
        t = torch.bmm(A[idc[sl]], x2[sl].unsqueeze(-1))
        u = torch.bmm(B[idc[sl]], t).squeeze(-1)
        v = (u * scaling[idc[sl]].unsqueeze(-1)).to(y.dtype)  # fp32 product, one rounding
        outs.append(torch.where(valid[sl].unsqueeze(-1), y2[sl] + v, y2[sl]))
    if not outs:
        return y
    return (outs[0] if len(outs) == 1 else torch.cat(outs)).reshape(y.shape)


def _multilora_fusable(x: torch.Tensor, module, A: torch.Tensor, B: torch.Tensor, scaling: torch.Tensor,
                       ids: torch.Tensor, M: int) -> bool:
    """nf4_linear_multilora_bnb's fused-path rules (its docstring) for one stack: _lora_fusable's,
    on [S, r, K] / [S, N, r]."""
    dev = module.weight.data.device
    return (ids.device == dev and scaling.device == dev and scaling.dtype == torch.float32 and scaling.is_contiguous()
            and scaling.data_ptr() % 4 == 0 and 1 <= int(A.shape[0]) <= _lib.LORA_MAX_ADAPTERS
            and not (torch.is_grad_enabled() and scaling.requires_grad)
            and _adapter_fusable(x, module, A, B, int(A.shape[1]), M, MULTILORA_ROUTED_MIN_M, MULTILORA_ROUTED_MAX_M))


def _multilora_ids32(ids: torch.Tensor, S: int) -> torch.Tensor:
    """The ids as the entry takes them: int32, contiguous.  int64 ids are clamped to [-1, S] first,
    so that a value beyond 32 bits stays "no adapter" instead of wrapping into range."""
    ids = ids.reshape(-1)
    if ids.dtype != torch.int32:
        ids = ids.clamp(-1, S).to(torch.int32)
    return ids.contiguous()


def _multilora_add(x: torch.Tensor, M: int, K: int, dtype: torch.dtype, ids32: torch.Tensor, S: int, items) -> None:
    """ONE nf4_lora_add_routed launch: ``items`` is [(y [.., N] contiguous, updated in place, A [S, r, K],
    B [S, N, r], scaling fp32 [S])]."""
    xc = _rows(x, K, dtype, True)
    stacks = (_lib.LoraStack * len(items))()
    for i, (y, A, B, scaling) in enumerate(items):
        r, N = int(A.shape[1]), int(B.shape[1])
        stacks[i] = _lib.LoraStack(A.data_ptr(), B.data_ptr(), scaling.data_ptr(), y.data_ptr(), y.data_ptr(), N,
                                   r * K, N * r, r)
    _stream_call("nf4 routed lora add", x.device, _lib.lib().nf4_lora_add_routed, xc.data_ptr(), ids32.data_ptr(), M, K,
                 S, ctypes.cast(stacks, ctypes.c_void_p), len(items), _dtype_code(dtype), None)


def nf4_linear_multilora_bnb(x: torch.Tensor, module, lora_A: torch.Tensor, lora_B: torch.Tensor, scaling,
                             adapter_ids: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A ``Linear4bit`` in bitsandbytes semantics whose batch rows belong to DIFFERENT low-rank
    adapters (one NF4 base, many LoRA adapters): row m gets ``W x + b + scaling[a] * B[a] (A[a] x)``
    with ``a = adapter_ids[m]``.  ``lora_A`` is ``[S, r, K]`` and ``lora_B`` ``[S, N, r]`` (an adapter
    of a smaller rank zero-padded to r), ``scaling`` an fp32 tensor ``[S]`` or a sequence of S
    floats, ``adapter_ids`` int32 or int64 with one id per row of x (x's leading dims flattened);
    an id outside ``0..S-1`` (-1, say) means the row has no adapter and gets the base alone, bit
    for bit.  Its definition, which is also its fallback and what autograd follows::

        y = nf4_linear_bnb(x, module, bias)
        valid = (ids >= 0) & (ids < S)
        idc = ids.clamp(0, S - 1)
        t = torch.bmm(lora_A[idc], x2.to(lora_A.dtype).unsqueeze(-1))
        u = torch.bmm(lora_B[idc], t).squeeze(-1)
        v = (u * scaling[idc].unsqueeze(-1)).to(y.dtype)     # fp32 product, one rounding
        torch.where(valid.unsqueeze(-1), y + v, y)

    in chunks of ``MULTILORA_CHUNK_ROWS`` rows, which bound the gathered ``[rows, r, K]`` tensor.  It
    reads nothing on the host, so it is itself capturable in a graph.

    The fused route runs the base through ``nf4_linear_bnb`` and the whole tail as ONE launch
    (``nf4_lora_add_routed``) that finds the adapters present on the device and updates the base's
    result in place, with ``nf4_lora_add``'s rounding chain per row; a captured graph follows
    whatever ids the buffer holds at replay.  It is taken under ``nf4_linear_lora_bnb``'s rules --
    tensors on the GPU, the adapters' dtype equal to ``quant_state.dtype`` (fp16 or bf16),
    ``K % 32 == 0``, ``N % 16 == 0``, ``r % 8 == 0`` with ``8 <= r <= 128``, contiguous and 16-byte
    aligned stacks, no gradient being recorded -- with ``S <= 64``, ``scaling`` an fp32 tensor on the
    device (a sequence is copied there first) and ``MULTILORA_ROUTED_MIN_M <= M <=
    MULTILORA_ROUTED_MAX_M`` rows.  int64 ids cost one clamp and one cast.  Everything else takes
    the composite.  The summation order of the two products may differ between the routes, so the
    last bits may.
    """
    M = _multilora_check(x, module, lora_A, lora_B, adapter_ids)
    S, K = int(lora_A.shape[0]), int(module.in_features)
    scaling = _multilora_scaling(scaling, S, lora_A.device)
    y = nf4_linear_bnb(x, module, bias)
    dtype = module.weight.quant_state.dtype
    if not (_multilora_fusable(x, module, lora_A, lora_B, scaling, adapter_ids, M) and _lora_base_in_place(y, dtype)):
        return _multilora_composite(y, x, lora_A, lora_B, scaling, adapter_ids)
    _multilora_add(x, M, K, dtype, _multilora_ids32(adapter_ids, S), S, [(y, lora_A, lora_B, scaling)])
    return y


def nf4_linear_multilora_bnb_grouped(x: torch.Tensor, modules: Sequence, stacks: Sequence, adapter_ids: torch.Tensor,
                                     biases: Optional[Sequence] = None) -> List[torch.Tensor]:
    """``nf4_linear_multilora_bnb`` for ``Linear4bit`` weights that share the input x and the ids
    (q/k/v, gate/up): ``stacks[i]`` is ``(lora_A [S, r_i, K], lora_B [S, N_i, r_i], scaling)`` or
    ``None`` for a module without adapters.  The base goes through ``nf4_linear_bnb_grouped``; ALL
    stacks that meet the fused-path rules and hold the same number of adapters go in ONE
    ``nf4_lora_add_routed`` launch when there are at most ``LORA_GROUP_MAX`` of them (each updates
    its module's result in place), every other stack takes the composite.
    """
    modules = list(modules)
    stacks = list(stacks)
    if len(stacks) != len(modules):
        raise ValueError("nf4_linear_multilora_bnb_grouped: one stack (or None) per module")
    checked = []
    for mod, st in zip(modules, stacks):
        if st is None:
            checked.append(None)
            continue
        _multilora_check(x, mod, st[0], st[1], adapter_ids)
        checked.append((st[0], st[1], _multilora_scaling(st[2], int(st[0].shape[0]), st[0].device)))
    S = next((int(st[0].shape[0]) for st in checked if st is not None), 0)  # the launch takes stacks of one size
    return _adapters_grouped(
        x, modules, checked, biases,
        lambda mod, st, M: int(st[0].shape[0]) == S and _multilora_fusable(x, mod, st[0], st[1], st[2], adapter_ids, M),
        lambda M, K, dtype, items: _multilora_add(x, M, K, dtype, _multilora_ids32(adapter_ids, S), S, items),
        lambda y, st: _multilora_composite(y, x, st[0], st[1], st[2], adapter_ids))
