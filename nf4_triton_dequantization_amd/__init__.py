"""MI355X-native NF4 double-dequantization (gfx950 HIP kernels behind a C ABI).

Public API mirrors the reference package ``nf4_triton_dequantization``
(/root/reference/nf4_triton_dequantization/__init__.py:7-12):

    from nf4_triton_dequantization_amd import triton_dequantize_nf4, reset_triton_dequantize_state

The alias package ``nf4_triton_dequantization`` (repo root) re-exports the same
names so existing callers (benchmark.py:11) import it unchanged.
"""
from .kernel import (  # noqa: F401
    check_gemm_workspaces,
    dequantize_nf4_bnb,
    dequantize_nf4_into,
    dequantize_nf4_many,
    nf4_embedding_bnb,
    nf4_linear,
    nf4_linear_bnb,
    nf4_linear_bnb_grouped,
    nf4_linear_grouped,
    nf4_linear_lora_bnb,
    nf4_linear_lora_bnb_grouped,
    nf4_linear_multilora_bnb,
    nf4_linear_multilora_bnb_grouped,
    nf4_mlp_bnb,
    nf4_moe_down_bnb,
    nf4_moe_linear_bnb,
    nf4_moe_mlp_bnb,
    nf4_moe_swiglu_bnb,
    nf4_swiglu_bnb,
    release_gemm_workspaces,
    reset_triton_dequantize_state,
    triton_dequantize_nf4,
)
from .bnb_layout import Embedding4bit, Experts4bit, Linear4bit, LoraLinear4bit, MultiLoraLinear4bit, Params4bit, QuantState, quantize_nf4  # noqa: F401
from .checkpoint import load_nf4_safetensors, save_nf4_safetensors  # noqa: F401
from .quantize import nf4_quantize  # noqa: F401

__all__ = ["triton_dequantize_nf4", "reset_triton_dequantize_state", "dequantize_nf4_many",
           "dequantize_nf4_bnb", "dequantize_nf4_into", "nf4_linear", "nf4_linear_bnb", "nf4_linear_bnb_grouped", "nf4_linear_grouped", "nf4_linear_lora_bnb", "nf4_linear_lora_bnb_grouped", "LoraLinear4bit", "nf4_linear_multilora_bnb", "nf4_linear_multilora_bnb_grouped", "MultiLoraLinear4bit", "check_gemm_workspaces",
           "release_gemm_workspaces", "nf4_embedding_bnb", "nf4_moe_linear_bnb", "nf4_moe_down_bnb", "nf4_moe_swiglu_bnb", "nf4_moe_mlp_bnb", "nf4_swiglu_bnb", "nf4_mlp_bnb", "Embedding4bit", "Experts4bit", "Linear4bit",
           "Params4bit", "QuantState", "quantize_nf4", "nf4_quantize", "load_nf4_safetensors", "save_nf4_safetensors"]
__version__ = "0.1.0"
