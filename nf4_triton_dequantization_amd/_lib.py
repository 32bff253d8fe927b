"""ctypes binding of the C ABI in include/nf4_dequant.h (libnf4dq.so, gfx950).

The library is loaded after ``import torch`` so that it binds to the HIP runtime
torch already mapped (same SONAME ``libamdhip64.so.7``): one HIP runtime per
process.  There is no fallback: if the library is missing or fails to load,
``lib()`` raises, and so does every product entry point that needs it.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  -- must precede the CDLL load (shared HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NF4DQ_LIB_PATH: load a diagnostic build of the same library instead (tools/Makefile);
# unset in every product / test / bench run (when set, the tensor-level entry is not
# loaded, so every call goes to that build)
LIB_PATH = os.environ.get("NF4DQ_LIB_PATH") or os.path.join(_HERE, "_lib", "libnf4dq.so")
EXT_PATH = os.path.join(_HERE, "_lib", "nf4ext.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nf4_dequant.h")

F16 = 0
BF16 = 1
F32 = 2

OK = 0
ERR_ARG = 1
ERR_SHAPE = 2
ERR_TOO_LARGE = 3
ERR_SPLITK_TIMEOUT = 4
ERR_HIP_BASE = 1000

BATCH_MAX = 24
IDS_I32 = 0
IDS_I64 = 1
GEMM_MAX_M = 32
GEMM_MT_MAX_M = 128  # NF4DQ_GEMM_MT_MAX_M: rows of the row-tiled entries (nf4_gemm_bnb_mt*)


class MatrixDesc(ctypes.Structure):
    """nf4_matrix_desc (include/nf4_dequant.h)."""

    _fields_ = [
        ("packed", ctypes.c_void_p),
        ("packed_len", ctypes.c_int64),
        ("absmax_q", ctypes.c_void_p),
        ("nb", ctypes.c_int64),
        ("absmax2", ctypes.c_void_p),
        ("n2", ctypes.c_int64),
        ("out", ctypes.c_void_p),
        ("m", ctypes.c_int64),
        ("n", ctypes.c_int64),
    ]


class LaunchCfg(ctypes.Structure):
    """nf4_launch_cfg (include/nf4_dequant.h)."""

    _fields_ = [
        ("tile_dwords", ctypes.c_int32),
        ("blocks_per_cu", ctypes.c_int32),
        ("nontemporal", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


CFG_ROWS = 1    # NF4DQ_CFG_ROWS: the one-thread-per-byte general kernel
CFG_CHUNKS = 2  # NF4DQ_CFG_CHUNKS: the chunk / piece kernels' path, even for a flat-eligible matrix


GEMM_K128 = 1
GEMM_STREAM = 2
GEMM_PERSIST = 3
GEMM_XS = 4
GEMM_XR = 5
GEMM_SK = 6  # retired in round 6: rejected with ERR_ARG
GEMM_GEMV = 7  # the decode GEMV (M = 1, K % 2048 == 0)
GEMM_MT = 8  # the row-tiled family (nf4_gemm_bnb_mt*: up to 128 rows); its own entries only
GEMM_MOE = 9  # the expert GEMM of a mixture-of-experts block (nf4_gemm_bnb_moe); its own entry only
GEMM_MT_SWIGLU = 10  # the fused gate/up SwiGLU launch (nf4_gemm_bnb_mt_swiglu); its own entry only
GEMM_MOE_SWIGLU = 11  # the fused expert SwiGLU launch (nf4_gemm_bnb_moe_swiglu); its own entry only
GEMM_MOE_DOWN = 12  # the fused expert down projection with the routed sum (nf4_gemm_bnb_moe_down); its own entry only
GEMM_MOE_RB = 13  # the expert GEMM in row blocks, up to MOE_RB_MAX_PAIRS pairs (nf4_gemm_bnb_moe_rb); its own entry only
ACT_SILU = 0  # NF4DQ_ACT_SILU: the activation of nf4_gemm_bnb_mt_swiglu and nf4_gemm_bnb_moe_swiglu
MOE_MAX_PAIRS = 128    # NF4DQ_MOE_MAX_PAIRS: (token, choice) pairs of one nf4_gemm_bnb_moe launch
MOE_RB_MAX_PAIRS = 1024  # NF4DQ_MOE_RB_MAX_PAIRS: (token, choice) pairs of one nf4_gemm_bnb_moe_rb launch
MOE_MAX_EXPERTS = 256  # NF4DQ_MOE_MAX_EXPERTS


GEMM_GROUP_MAX = 8


class GemmMat(ctypes.Structure):
    """nf4_gemm_mat (include/nf4_dequant.h)."""

    _fields_ = [("packed", ctypes.c_void_p), ("packed_len", ctypes.c_int64), ("absmax_q", ctypes.c_void_p),
                ("nb", ctypes.c_int64), ("absmax2", ctypes.c_void_p), ("n2", ctypes.c_int64),
                ("y", ctypes.c_void_p), ("N", ctypes.c_int64)]


class GemmBnbMat(ctypes.Structure):
    """nf4_gemm_bnb_mat (include/nf4_dequant.h): one weight of nf4_gemm_bnb_grouped."""

    _fields_ = [("packed", ctypes.c_void_p), ("packed_len", ctypes.c_int64), ("absmax_q", ctypes.c_void_p),
                ("nb", ctypes.c_int64), ("code2", ctypes.c_void_p), ("absmax2", ctypes.c_void_p),
                ("n2", ctypes.c_int64), ("offset", ctypes.c_void_p), ("blocksize", ctypes.c_int32),
                ("blocksize2", ctypes.c_int32), ("y", ctypes.c_void_p), ("N", ctypes.c_int64)]


class MoeExperts(ctypes.Structure):
    """nf4_moe_experts (include/nf4_dequant.h): the stacked experts of nf4_gemm_bnb_moe."""

    _fields_ = [("packed", ctypes.c_void_p), ("packed_stride", ctypes.c_int64), ("absmax_q", ctypes.c_void_p),
                ("nb_stride", ctypes.c_int64), ("code2", ctypes.c_void_p), ("code2_stride", ctypes.c_int64),
                ("absmax2", ctypes.c_void_p), ("n2_stride", ctypes.c_int64), ("offset", ctypes.c_void_p),
                ("N", ctypes.c_int64), ("K", ctypes.c_int64), ("experts", ctypes.c_int32), ("single", ctypes.c_int32),
                ("blocksize", ctypes.c_int32), ("blocksize2", ctypes.c_int32)]


LORA_MAX_M = 128     # NF4DQ_LORA_MAX_M: rows of one nf4_lora_add launch
LORA_MAX_R = 128     # NF4DQ_LORA_MAX_R: the largest adapter rank
LORA_GROUP_MAX = 8   # NF4DQ_LORA_GROUP_MAX: adapters of one nf4_lora_add launch
LORA_TILES = (16, 32, 64, 128, 256)  # nf4_lora_cfg.tile_n
LORA_WAVES = (1, 2, 4)               # nf4_lora_cfg.waves


class LoraMat(ctypes.Structure):
    """nf4_lora_mat (include/nf4_dequant.h): one adapter of nf4_lora_add."""

    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("base", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("N", ctypes.c_int64), ("r", ctypes.c_int32), ("scale", ctypes.c_float)]


LORA_MAX_ADAPTERS = 64  # NF4DQ_LORA_MAX_ADAPTERS: adapters of one stack of nf4_lora_add_routed


class LoraStack(ctypes.Structure):
    """nf4_lora_stack (include/nf4_dequant.h): one stack of adapters of nf4_lora_add_routed."""

    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("base", ctypes.c_void_p),
                ("y", ctypes.c_void_p), ("N", ctypes.c_int64), ("a_stride", ctypes.c_int64), ("b_stride", ctypes.c_int64),
                ("r", ctypes.c_int32)]


class LoraCfg(ctypes.Structure):
    """nf4_lora_cfg (include/nf4_dequant.h)."""

    _fields_ = [("tile_n", ctypes.c_int32), ("waves", ctypes.c_int32)]


class GemmCfg(ctypes.Structure):
    """nf4_gemm_cfg (include/nf4_dequant.h)."""

    _fields_ = [("kernel", ctypes.c_int32), ("waves", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("ksplit", ctypes.c_int32), ("strips", ctypes.c_int32)]


# name -> (restype, argtypes); every symbol include/nf4_dequant.h declares.
_P, _I64, _I32, _F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
SIGNATURES = {
    "nf4_dequant_ref": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I32, _I64, _I64, _P]),
    "nf4_dequant_single": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I32, _I64, _I64, _P]),
    "nf4_dequant_ref_cpu": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I32, _I64, _I64, _I32]),
    "nf4_dequant_single_cpu": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I32, _I64, _I64, _I32]),
    "nf4_dequant_ref_batched": (ctypes.c_int, [ctypes.POINTER(MatrixDesc), _I32, _I32, _P]),
    "nf4_dequant_bnb": (ctypes.c_int, [_P, _P, _I64, _P, _P, _I64, _F, _P, _I32, _I64, _I32, _I32, _P]),
    "nf4_dequant_bnb_single": (ctypes.c_int, [_P, _P, _I64, _P, _I32, _I64, _I32, _P]),
    "nf4_embedding_bnb": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _P, _I32, _I64,
                                         _I64, _P]),
    "nf4_embedding_bnb_single": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _I64, _I32, _P, _I32, _I64, _I64, _P]),
    "nf4_embedding_bnb_cpu": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _P, _I32,
                                             _I64, _I64, _I32]),
    "nf4_embedding_bnb_single_cpu": (ctypes.c_int, [_P, _I32, _I64, _P, _P, _I64, _I32, _P, _I32, _I64, _I64, _I32]),
    "nf4_dequant_ref_cfg": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I32, _I64, _I64,
                                           ctypes.POINTER(LaunchCfg), _P]),
    "nf4_quant_workspace_bytes": (ctypes.c_size_t, [_I64, _I32]),
    "nf4_quant_bnb": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _P]),
    "nf4_quant_bnb_nested": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _I32, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "nf4_quant_bnb_cpu": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _P, _I32]),
    "nf4_quant_bnb_nested_cpu": (ctypes.c_int, [_P, _I32, _I64, _I32, _P, _I32, _P, _P, _P, _P, _I32]),
    "nf4_gemm_workspace_bytes": (ctypes.c_size_t, [_I64, _I64, _I64]),
    "nf4_gemm_ref": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _I64, _I64, _P, ctypes.c_size_t,
                                    _P]),
    "nf4_gemm_workspace_bytes_cfg": (ctypes.c_size_t, [_I64, _I64, _I64, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_ref_cfg": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _I64, _I64, _P,
                                        ctypes.c_size_t, ctypes.POINTER(GemmCfg), _P]),
    "nf4_gemm_grouped_workspace_bytes": (ctypes.c_size_t, [_I64, _I64, ctypes.POINTER(GemmMat), _I32,
                                                           ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_ref_grouped": (ctypes.c_int, [_P, _I64, _I64, ctypes.POINTER(GemmMat), _I32, _I32, _P, ctypes.c_size_t,
                                            ctypes.POINTER(GemmCfg), _P]),
    "nf4_gemm_bnb_workspace_bytes": (ctypes.c_size_t, [_I64, _I64, _I64, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _P, _I32, _I64, _I64,
                                    _P, ctypes.c_size_t, ctypes.POINTER(GemmCfg), _P]),
    "nf4_gemm_bnb_single": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _I32, _P, _I32, _I64, _I64, _P,
                                           ctypes.c_size_t, ctypes.POINTER(GemmCfg), _P]),
    # `mats`: const void* in the header, pointing at GemmBnbMat[count]
    "nf4_gemm_bnb_grouped_workspace_bytes": (ctypes.c_size_t, [_I64, _I64, _P, _I32, _I32, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_grouped": (ctypes.c_int, [_P, _I64, _I64, _P, _I32, _I32, _I32, _P, ctypes.c_size_t,
                                            ctypes.POINTER(GemmCfg), _P]),
    "nf4_gemm_bnb_mt_workspace_bytes": (ctypes.c_size_t, [_I64, _I64, _I64, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_mt": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _P, _I32, _I64, _I64,
                                       _P, ctypes.c_size_t, ctypes.POINTER(GemmCfg), _P]),
    "nf4_gemm_bnb_mt_single": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _I32, _P, _I32, _I64, _I64, _P,
                                              ctypes.c_size_t, ctypes.POINTER(GemmCfg), _P]),
    # `experts`: const void* in the header, pointing at ONE MoeExperts; `expert_ids`: int32 on the device
    "nf4_gemm_bnb_moe_workspace_bytes": (ctypes.c_size_t, [_I64, _P, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_moe": (ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _I32, _P, ctypes.c_size_t,
                                        ctypes.POINTER(GemmCfg), _P]),
    "nf4_gemm_bnb_moe_rb_workspace_bytes": (ctypes.c_size_t, [_I64, _P, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_moe_rb": (ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _I32, _P, ctypes.c_size_t,
                                           ctypes.POINTER(GemmCfg), _P]),
    # `gate_up`: const void* in the header, pointing at GemmBnbMat[2] (gate, up)
    "nf4_gemm_bnb_mt_swiglu_workspace_bytes": (ctypes.c_size_t, [_I64, _I64, _I64, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_mt_swiglu": (ctypes.c_int, [_P, _I64, _I64, _P, _I32, _I32, _P, _I32, _P, ctypes.c_size_t,
                                              ctypes.POINTER(GemmCfg), _P]),
    # `gate_up`: const void* in the header, pointing at MoeExperts[2] (gate stack, up stack)
    "nf4_gemm_bnb_moe_swiglu_workspace_bytes": (ctypes.c_size_t, [_I64, _P, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_moe_swiglu": (ctypes.c_int, [_P, _P, _I64, _I32, _P, _I32, _P, _I32, _P, ctypes.c_size_t,
                                               ctypes.POINTER(GemmCfg), _P]),
    # `experts`: const void* in the header, pointing at ONE MoeExperts; ids and routing weights on the device
    "nf4_gemm_bnb_moe_down_workspace_bytes": (ctypes.c_size_t, [_I64, _P, ctypes.POINTER(GemmCfg)]),
    "nf4_gemm_bnb_moe_down": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, _I32, _P, _P, _I32, _P, ctypes.c_size_t,
                                             ctypes.POINTER(GemmCfg), _P]),
    # `mats`: const void* in the header, pointing at LoraMat[count]; `cfg`: NULL or one LoraCfg
    "nf4_lora_add": (ctypes.c_int, [_P, _I64, _I64, _P, _I32, _I32, _P, _P]),
    # `adapter_ids`: int32 on the device; `stacks`: const void* in the header, pointing at LoraStack[count]
    "nf4_lora_add_routed": (ctypes.c_int, [_P, _P, _I64, _I64, _I32, _P, _I32, _I32, _P, _P]),
    "nf4_gemm_check_workspace": (ctypes.c_int, [_P, ctypes.c_size_t, _P]),
    "nf4_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "nf4_version": (ctypes.c_char_p, []),
}

_lock = threading.Lock()
_lib = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"nf4 HIP library not built: {LIB_PATH} is missing "
                    "(run `python __graft_entry__.py build` or `make -C nf4_triton_dequantization_amd`)")
            handle = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


_ext = None
_ext_tried = False


def ext():
    """The tensor-level fast entry (``_lib/nf4ext.so``, csrc/nf4_torch_ext.cpp), or None:
    callers then take the ctypes route to the same kernels.

    None when the extension is not built, when it fails to load (a stale build or a
    torch ABI mismatch: a warning names the error), and when ``NF4DQ_LIB_PATH``
    selects another build of the C ABI -- the extension links the product
    ``_lib/libnf4dq.so`` through its rpath, so loading it then would put two copies
    of the library in the process and the drop-in would run the other one.
    Raises like ``lib()`` when the C ABI itself is missing.
    """
    global _ext, _ext_tried
    if not _ext_tried:
        lib()  # the C ABI first (the extension links it; one copy per process); takes _lock itself
        with _lock:
            if not _ext_tried:
                if os.path.exists(EXT_PATH) and not os.environ.get("NF4DQ_LIB_PATH"):
                    import importlib.util

                    try:
                        spec = importlib.util.spec_from_file_location("nf4ext", EXT_PATH)
                        mod = importlib.util.module_from_spec(spec)
                        spec.loader.exec_module(mod)
                        _ext = mod
                    except (ImportError, OSError) as e:
                        import warnings

                        warnings.warn(f"nf4ext.so did not load ({e}); the drop-in uses the ctypes route "
                                      f"to the same kernels", RuntimeWarning, stacklevel=2)
                        _ext = None
                _ext_tried = True
    return _ext


def strerror(code: int) -> str:
    return lib().nf4_strerror(int(code)).decode()


def check(code: int, what: str) -> None:
    if code != OK:
        raise RuntimeError(f"{what} failed: {strerror(code)} (code {code})")
