"""bitsandbytes ``Linear4bit`` / ``Params4bit`` / ``QuantState`` layout stand-in + NF4 quantizer.

bitsandbytes is not installed here, yet the drop-in boundary is
defined by its layout: the reference reads ``module.weight.data``
(uint8 ``[numel/2, 1]``), ``weight.quant_state.absmax`` (uint8),
``quant_state.state2.absmax`` (fp32), ``quant_state.dtype`` and
``module.out_features / in_features``; its harness additionally asserts the
fields checked by ``assert_correct_bnb`` (reference benchmark.py:18-28):
``quant_state.code`` fp32, ``offset`` fp32, ``blocksize == 64``,
``state2.code`` fp32, ``state2.blocksize == 256``.

This module supplies objects with exactly that layout, plus the producer side
(SURVEY §8f row 3): ``quantize_nf4`` restates bitsandbytes' published NF4
quantizer (blockwise absmax, nearest NF4 code, high nibble first) and its
nested 8-bit "dynamic map" compression of the absmax (``compress_statistics``).
Being a restatement of an absent library, its bit-level agreement with real
bitsandbytes is unpinned; what the tests pin is the layout and that the
``semantics="bnb"`` dequant inverts it.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

# NF4 code points (the same 16 fp32 values as kernel_optimized.py:234-239).
NF4_CODE = torch.tensor(
    [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
     -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
     0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
     0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], dtype=torch.float32)


def dynamic_map(signed: bool = True, max_exponent_bits: int = 7, total_bits: int = 8) -> torch.Tensor:
    """The 256-entry dynamic (exponent + linear fraction) code book bitsandbytes uses
    for the nested absmax.  Each decade 10^(e-6), e = 0..6, contributes the
    midpoints of a linear partition of [0.1, 1]; then 0 and 1 are added, the
    list is padded with zeros to 256 and sorted."""
    vals = []
    frac_bits = total_bits - 1 - max_exponent_bits
    for e in range(max_exponent_bits):
        count = 2 ** (e + frac_bits) + 1 if signed else 2 ** (e + frac_bits + 1) + 1
        edges = torch.linspace(0.1, 1.0, count, dtype=torch.float32)
        mids = (edges[:-1] + edges[1:]) / 2.0
        scale = 10.0 ** (-(max_exponent_bits - 1) + e)
        vals += (scale * mids).tolist()
        if signed:
            vals += (-scale * mids).tolist()
    extra = 2 ** frac_bits - 1
    if extra > 0:
        edges = torch.linspace(0.1, 1.0, extra + 1, dtype=torch.float32)
        mids = (edges[:-1] + edges[1:]) / 2.0
        scale = 10.0 ** (-(max_exponent_bits - 1) + max_exponent_bits - 1)
        vals += (scale * mids).tolist()
        if signed:
            vals += (-scale * mids).tolist()
    vals += [0.0, 1.0]
    vals += [0.0] * (2 ** total_bits - len(vals))
    vals.sort()
    return torch.tensor(vals, dtype=torch.float32)


class QuantState:
    """Field layout of ``bitsandbytes.functional.QuantState`` (what the boundary reads)."""

    def __init__(self, absmax, shape=None, code=None, blocksize=None, quant_type=None, dtype=None,
                 offset=None, state2: Optional["QuantState"] = None):
        self.absmax = absmax
        self.shape = shape
        self.code = code
        self.blocksize = blocksize
        self.quant_type = quant_type
        self.dtype = dtype
        self.offset = offset
        self.state2 = state2
        self.nested = state2 is not None

    def to(self, device):
        self.absmax = self.absmax.to(device)
        if self.code is not None:
            self.code = self.code.to(device)
        if self.offset is not None:
            self.offset = self.offset.to(device)
        if self.state2 is not None:
            self.state2.to(device)
        return self


def _nearest_code(x: torch.Tensor, code: torch.Tensor) -> torch.Tensor:
    """Index of the nearest entry of a sorted code book (ties to the lower index)."""
    mids = (code[1:] + code[:-1]) / 2.0
    return torch.bucketize(x, mids, right=False)


def quantize_blockwise_8bit(a: torch.Tensor, code: torch.Tensor, blocksize: int = 256):
    """Blockwise absmax 8-bit quantization of a flat fp32 vector with a code book."""
    n = a.numel()
    nblk = (n + blocksize - 1) // blocksize
    pad = nblk * blocksize - n
    ap = torch.nn.functional.pad(a.reshape(-1), (0, pad)).view(nblk, blocksize)
    amax = ap.abs().amax(dim=1).clamp_min(torch.finfo(torch.float32).tiny)
    q = _nearest_code((ap / amax[:, None]).reshape(-1), code.to(a.device))[:n]
    return q.to(torch.uint8), amax.to(torch.float32)


def quantize_nf4(w: torch.Tensor, blocksize: int = 64, compress_statistics: bool = True,
                 blocksize2: int = 256, quant_storage=torch.uint8):
    """NF4-quantize ``w`` ([out, in] float) into the bitsandbytes Params4bit layout.

    Returns ``(packed uint8 [numel/2, 1], QuantState)``.  ``quant_state.dtype`` is
    ``w.dtype``.
    """
    shape = w.shape
    dev = w.device
    flat = w.detach().reshape(-1).to(torch.float32)
    n = flat.numel()
    if n % 2:
        flat = torch.nn.functional.pad(flat, (0, 1))
    nblk = (n + blocksize - 1) // blocksize
    pad = nblk * blocksize - flat.numel()
    blocks = torch.nn.functional.pad(flat, (0, pad)).view(nblk, blocksize)
    absmax = blocks.abs().amax(dim=1).to(torch.float32)
    safe = torch.where(absmax > 0, absmax, torch.ones_like(absmax))
    idx = _nearest_code((blocks / safe[:, None]).reshape(-1), NF4_CODE.to(dev))[: flat.numel()]
    idx = idx.to(torch.uint8)
    packed = ((idx[0::2] << 4) | idx[1::2]).to(torch.uint8).view(-1, 1)
    if quant_storage != torch.uint8:
        packed = packed.view(quant_storage)
    code = NF4_CODE.to(dev)
    if compress_statistics:
        offset = absmax.mean()
        c2 = dynamic_map(signed=True).to(dev)
        qabs, abs2 = quantize_blockwise_8bit(absmax - offset, c2, blocksize2)
        state2 = QuantState(absmax=abs2, code=c2, blocksize=blocksize2, quant_type=None, dtype=torch.float32)
        qs = QuantState(absmax=qabs, shape=shape, code=code, blocksize=blocksize, quant_type="nf4",
                        dtype=w.dtype, offset=offset.reshape(()), state2=state2)
    else:
        qs = QuantState(absmax=absmax, shape=shape, code=code, blocksize=blocksize, quant_type="nf4",
                        dtype=w.dtype)
    return packed, qs


class Params4bit(nn.Parameter):
    """uint8 packed NF4 storage with an attached ``quant_state`` (bnb ``Params4bit`` layout)."""

    def __new__(cls, data: torch.Tensor, quant_state: Optional[QuantState] = None):
        self = super().__new__(cls, data, requires_grad=False)
        self.quant_state = quant_state
        return self

    def to(self, *args, **kwargs):
        moved = super().to(*args, **kwargs)
        out = Params4bit(moved.data, self.quant_state)
        if self.quant_state is not None:
            dev = moved.device
            self.quant_state.to(dev)
        return out


_FROM_SOURCE = object()  # Linear4bit.from_float(bias=...): take the source module's bias


class Linear4bit(nn.Module):
    """Minimal ``bitsandbytes.nn.Linear4bit`` stand-in (NF4, optional nested absmax).

    ``Linear4bit(in_features, out_features, bias=None, compute_dtype=..., compress_statistics=True,
    quant_type="nf4")`` quantizes a kaiming-uniform fp32 weight at construction (bnb
    quantizes on ``.to("cuda")``; the resulting layout is the same).  ``forward`` uses
    bitsandbytes semantics through the HIP kernel.
    """

    def __init__(self, input_features: int, output_features: int, bias=None, compute_dtype=None,
                 compress_statistics: bool = True, quant_type: str = "nf4", device=None,
                 weight: Optional[torch.Tensor] = None, blocksize: int = 64):
        super().__init__()
        if quant_type != "nf4":
            raise ValueError("only quant_type='nf4' is supported")
        self.in_features = input_features
        self.out_features = output_features
        self.compute_dtype = compute_dtype
        if weight is None:
            weight = torch.empty(output_features, input_features, dtype=torch.float32, device=device)
            nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
        packed, qs = quantize_nf4(weight.to(torch.float32), blocksize=blocksize,
                                  compress_statistics=compress_statistics)
        qs.dtype = compute_dtype if compute_dtype is not None else weight.dtype
        qs.shape = torch.Size((output_features, input_features))
        self.weight = Params4bit(packed, qs)
        self.bias = None if not bias else nn.Parameter(torch.zeros(output_features, device=device))

    @classmethod
    def from_float(cls, linear_or_weight, compute_dtype=None, compress_statistics: bool = True, bias=_FROM_SOURCE,
                   blocksize: int = 64):
        """Build the module from an ``nn.Linear`` or an ``[out, in]`` float weight through the
        HIP quantizer (``quantize.nf4_quantize``), on the weight's device: no kaiming init, no
        torch-op quantization.  ``bias``: by default an ``nn.Linear``'s own bias is carried over
        (a bare weight has none); ``None`` / ``False`` drops it, a tensor replaces it.
        ``quant_state.dtype`` is ``compute_dtype`` if given, else the weight's dtype."""
        from .quantize import nf4_quantize

        if isinstance(linear_or_weight, nn.Module):
            weight = linear_or_weight.weight
            if bias is _FROM_SOURCE:
                bias = getattr(linear_or_weight, "bias", None)
        else:
            weight = linear_or_weight
            if bias is _FROM_SOURCE:
                bias = None
        if weight.dim() != 2:
            raise ValueError(f"Linear4bit.from_float: expected an [out_features, in_features] weight, got "
                             f"{tuple(weight.shape)}")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.out_features, self.in_features = int(weight.shape[0]), int(weight.shape[1])
        self.compute_dtype = compute_dtype
        packed, qs = nf4_quantize(weight, blocksize=blocksize, compress_statistics=compress_statistics)
        if compute_dtype is not None:
            qs.dtype = compute_dtype
        qs.shape = torch.Size((self.out_features, self.in_features))
        self.weight = Params4bit(packed, qs)
        if bias is None or bias is False:
            self.bias = None
        else:
            self.bias = nn.Parameter(bias.detach().clone().to(weight.device), requires_grad=bias.requires_grad)
        return self

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if self.weight.quant_state is not None:
            self.weight.quant_state.to(self.weight.device)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """``x @ W.t() + bias`` with W = ``dequantize_nf4_bnb(self)`` (``kernel.nf4_linear_bnb``).
        Decode-shaped inputs (at most 32 rows, N % 64 == 0, K % 128 == 0, no gradient recorded
        for ``x``) run one fused dequant + GEMM launch with no host synchronisation; anything
        else dequantizes and multiplies with torch, as every input did before.  The weights
        are the same bit for bit and both accumulate in fp32; the last bit of ``y`` may differ
        between the two paths (summation order), as documented for ``nf4_linear``."""
        from .kernel import nf4_linear_bnb

        return nf4_linear_bnb(x, self, self.bias)


class LoraLinear4bit(nn.Module):
    """A ``Linear4bit`` with a low-rank (LoRA) adapter, the inference form of PEFT's wrapper:
    ``base_layer(x) + lora_B(lora_A(x)) * scaling``.  There is NO dropout (PEFT's ``lora_dropout``
    is the identity at inference) and one adapter.

    ``base_layer`` is the wrapped ``Linear4bit``; ``lora_A`` (``[r, in_features]``) and ``lora_B``
    (``[out_features, r]``) are bias-free ``nn.Linear``, so the parameter names ``lora_A.weight``
    and ``lora_B.weight`` are PEFT's and an adapter state dict loads once its prefix (and the
    adapter name) is stripped; ``scaling`` is a float (``lora_alpha / r``).  ``forward`` is
    ``kernel.nf4_linear_lora_bnb``: one fused launch for the whole tail where that is routed, the
    composite -- which autograd follows to ``lora_A`` and ``lora_B`` -- everywhere else.
    """

    def __init__(self, base_layer: Linear4bit, lora_A: nn.Linear, lora_B: nn.Linear, scaling: float):
        super().__init__()
        self.base_layer = base_layer
        self.lora_A = lora_A
        self.lora_B = lora_B
        self.scaling = float(scaling)
        self.in_features, self.out_features = base_layer.in_features, base_layer.out_features
        self.r = int(lora_A.out_features)

    @classmethod
    def from_linear4bit(cls, base: Linear4bit, r: int, lora_alpha: float, dtype=None):
        """A fresh adapter of rank ``r`` on ``base`` with PEFT's initialisation: kaiming-uniform
        ``lora_A`` (``a = sqrt(5)``), zero ``lora_B`` -- so the module starts as ``base`` exactly
        -- and ``scaling = lora_alpha / r``.  ``dtype`` defaults to ``quant_state.dtype`` (the
        fused route needs the two equal); the adapter lives on the weight's device."""
        if r < 1:
            raise ValueError("LoraLinear4bit.from_linear4bit: r must be positive")
        dev = base.weight.data.device
        dtype = dtype if dtype is not None else base.weight.quant_state.dtype
        lora_A = nn.Linear(base.in_features, r, bias=False, device=dev, dtype=dtype)
        lora_B = nn.Linear(r, base.out_features, bias=False, device=dev, dtype=dtype)
        nn.init.kaiming_uniform_(lora_A.weight, a=math.sqrt(5))
        nn.init.zeros_(lora_B.weight)
        return cls(base, lora_A, lora_B, lora_alpha / r)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .kernel import nf4_linear_lora_bnb

        return nf4_linear_lora_bnb(x, self.base_layer, self.lora_A.weight, self.lora_B.weight, self.scaling,
                                   self.base_layer.bias)


class MultiLoraLinear4bit(nn.Module):
    """One ``Linear4bit`` serving MANY low-rank adapters at once: row m of a batch takes adapter
    ``adapter_ids[m]``, a row whose id is outside ``0..S-1`` (-1, say) the base alone.  Inference
    form, no dropout, as ``LoraLinear4bit``.

    ``base_layer`` is the wrapped ``Linear4bit``; ``lora_A`` (``[S, r, in_features]``) and ``lora_B``
    (``[S, out_features, r]``) are parameters holding the S adapters stacked, each zero-padded to
    the stack's rank r; ``scaling`` is an fp32 buffer ``[S]`` and ``ranks`` the adapters' own ranks.
    ``forward(x, adapter_ids)`` is ``kernel.nf4_linear_multilora_bnb``: one routed launch for the
    whole tail where that is routed -- capturable in a graph, the ids read at replay -- and the
    composite, which autograd follows to ``lora_A`` and ``lora_B``, everywhere else.
    """

    def __init__(self, base_layer: Linear4bit, lora_A: torch.Tensor, lora_B: torch.Tensor, scaling: torch.Tensor,
                 ranks=None):
        super().__init__()
        if lora_A.dim() != 3 or lora_B.dim() != 3 or lora_A.shape[0] != lora_B.shape[0] \
                or tuple(lora_A.shape[1:]) != (lora_B.shape[2], base_layer.in_features) \
                or lora_B.shape[1] != base_layer.out_features:
            raise ValueError(f"MultiLoraLinear4bit: lora_A must be [S, r, {base_layer.in_features}] and lora_B "
                             f"[S, {base_layer.out_features}, r], got {tuple(lora_A.shape)} and {tuple(lora_B.shape)}")
        self.base_layer = base_layer
        self.lora_A = nn.Parameter(lora_A, requires_grad=lora_A.requires_grad)
        self.lora_B = nn.Parameter(lora_B, requires_grad=lora_B.requires_grad)
        scaling = torch.as_tensor(scaling, dtype=torch.float32, device=lora_A.device).reshape(-1)
        if scaling.numel() != lora_A.shape[0]:
            raise ValueError(f"MultiLoraLinear4bit: {scaling.numel()} scalings for {lora_A.shape[0]} adapters")
        self.register_buffer("scaling", scaling.contiguous())
        self.in_features, self.out_features = base_layer.in_features, base_layer.out_features
        self.num_adapters, self.r = int(lora_A.shape[0]), int(lora_A.shape[1])
        self.ranks = [self.r] * self.num_adapters if ranks is None else [int(v) for v in ranks]

    @classmethod
    def from_linear4bit(cls, base: Linear4bit, adapters, dtype=None):
        """Stack ``adapters``, a list of ``(lora_A [r_i, K], lora_B [N, r_i], scaling_i)``, on ``base``:
        each is zero-padded to the largest ``r_i`` rounded up to a multiple of 8 (exact zeros add
        nothing to a sum, so an adapter's results do not depend on the padding).  ``dtype``
        defaults to ``quant_state.dtype`` (the fused route needs the two equal); the stacks live on
        the weight's device and record no gradient."""
        adapters = list(adapters)
        if not adapters:
            raise ValueError("MultiLoraLinear4bit.from_linear4bit: at least one adapter")
        N, K = int(base.out_features), int(base.in_features)
        for i, (A, B, _) in enumerate(adapters):
            if A.dim() != 2 or B.dim() != 2 or A.shape[0] < 1 or tuple(A.shape) != (A.shape[0], K) \
                    or tuple(B.shape) != (N, A.shape[0]):
                raise ValueError(f"MultiLoraLinear4bit.from_linear4bit: adapter {i} must be ([r, {K}], [{N}, r], scaling), "
                                 f"got {tuple(A.shape)} and {tuple(B.shape)}")
        dev = base.weight.data.device
        dtype = dtype if dtype is not None else base.weight.quant_state.dtype
        ranks = [int(A.shape[0]) for A, _, _ in adapters]
        r = -(-max(ranks) // 8) * 8
        lora_A = torch.zeros(len(adapters), r, K, dtype=dtype, device=dev)
        lora_B = torch.zeros(len(adapters), N, r, dtype=dtype, device=dev)
        for s, (A, B, _) in enumerate(adapters):
            lora_A[s, :ranks[s]] = A.detach().to(device=dev, dtype=dtype)
            lora_B[s, :, :ranks[s]] = B.detach().to(device=dev, dtype=dtype)
        scaling = torch.tensor([float(sc) for _, _, sc in adapters], dtype=torch.float32, device=dev)
        return cls(base, lora_A, lora_B, scaling, ranks)

    def adapter(self, s: int) -> "LoraLinear4bit":
        """Adapter ``s`` alone as a ``LoraLinear4bit`` over the same base: its ``lora_A`` / ``lora_B``
        weights are VIEWS of this module's stacks (the adapter's own rank, without the padding)."""
        if not 0 <= s < self.num_adapters:
            raise IndexError(f"MultiLoraLinear4bit.adapter: {s} is outside 0..{self.num_adapters - 1}")
        r = self.ranks[s]
        A, B = self.lora_A.detach()[s, :r], self.lora_B.detach()[s, :, :r]
        la = nn.Linear(self.in_features, r, bias=False, device="meta")
        lb = nn.Linear(r, self.out_features, bias=False, device="meta")
        la.weight = nn.Parameter(A, requires_grad=False)
        lb.weight = nn.Parameter(B, requires_grad=False)
        return LoraLinear4bit(self.base_layer, la, lb, float(self.scaling[s]))

    def forward(self, x: torch.Tensor, adapter_ids: torch.Tensor) -> torch.Tensor:
        from .kernel import nf4_linear_multilora_bnb

        return nf4_linear_multilora_bnb(x, self.base_layer, self.lora_A, self.lora_B, self.scaling, adapter_ids,
                                        self.base_layer.bias)


class Embedding4bit(nn.Module):
    """``bitsandbytes.nn.Embedding4bit`` / ``EmbeddingNF4`` stand-in: a token embedding whose
    ``[num_embeddings, embedding_dim]`` table is NF4 storage (a ``Params4bit``).

    ``forward(ids)`` gathers and dequantizes only the rows named (``kernel.nf4_embedding_bnb``:
    one HIP launch, no host synchronisation, capturable in a graph); the table is never
    dequantized as a whole.  The weight is frozen: no gradient, and ``padding_idx`` /
    ``max_norm`` are not interpreted (a padding row returns what is stored).  ``as_linear()``
    gives the tied ``lm_head`` over the same storage.
    """

    def __init__(self, num_embeddings: int, embedding_dim: int, weight: Params4bit):
        super().__init__()
        self.num_embeddings = int(num_embeddings)
        self.embedding_dim = int(embedding_dim)
        self.weight = weight

    @classmethod
    def from_float(cls, embedding_or_weight, dtype=None, compress_statistics: bool = True, blocksize: int = 64):
        """Build the module from an ``nn.Embedding`` or a ``[num_embeddings, embedding_dim]`` float
        weight through the HIP quantizer (``quantize.nf4_quantize``) on the weight's device, as
        ``Linear4bit.from_float`` does.  ``quant_state.dtype`` (the dtype ``forward`` returns) is
        ``dtype`` if given, else the weight's."""
        from .quantize import nf4_quantize

        weight = embedding_or_weight.weight if isinstance(embedding_or_weight, nn.Module) else embedding_or_weight
        if weight.dim() != 2:
            raise ValueError(f"Embedding4bit.from_float: expected a [num_embeddings, embedding_dim] weight, got "
                             f"{tuple(weight.shape)}")
        rows, dim = int(weight.shape[0]), int(weight.shape[1])
        packed, qs = nf4_quantize(weight, blocksize=blocksize, compress_statistics=compress_statistics)
        if dtype is not None:
            qs.dtype = dtype
        qs.shape = torch.Size((rows, dim))
        return cls(rows, dim, Params4bit(packed, qs))

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if self.weight.quant_state is not None:
            self.weight.quant_state.to(self.weight.device)
        return self

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        from .kernel import nf4_embedding_bnb

        return nf4_embedding_bnb(ids, self)

    def as_linear(self) -> "Linear4bit":
        """The tied output projection: a bias-free ``Linear4bit`` with ``out_features =
        num_embeddings`` and ``in_features = embedding_dim`` that holds this module's own
        ``Params4bit`` object, so ``lm_head`` runs ``nf4_linear_bnb`` on the embedding's storage."""
        lin = Linear4bit.__new__(Linear4bit)
        nn.Module.__init__(lin)
        lin.in_features, lin.out_features = self.embedding_dim, self.num_embeddings
        lin.compute_dtype = self.weight.quant_state.dtype if self.weight.quant_state is not None else None
        lin.weight = self.weight
        lin.bias = None
        return lin


class Experts4bit(nn.Module):
    """The experts of one projection of a mixture-of-experts block (Mixtral's w1, w2 or w3 over
    all experts) as stacked NF4 storage: E weights of one shape ``[out_features, in_features]``,
    blocksize 64, all with nested statistics or all with fp32 ``absmax``.

    Storage (what ``kernel.nf4_moe_linear_bnb`` hands to the ``nf4_gemm_bnb_moe`` entry as base
    pointers and strides), every expert's part exactly the bytes of its own
    ``Linear4bit.from_float`` -- own absmax2 groups, own offset:

    * ``weight``  uint8 ``[E, N*K/2]`` (a frozen parameter);
    * ``absmax``  ``[E, N*K/64]``, uint8 (nested) or fp32 (``compress_statistics=False``);
    * ``absmax2`` fp32 ``[E, ceil(N*K/64 / 256)]``, ``code2`` fp32 ``[256]`` shared by all
      experts and ``offset`` fp32 ``[E]`` (nested; None otherwise).

    ``expert(e)`` is a bias-free ``Linear4bit`` over views of that storage, so
    ``dequantize_nf4_bnb(experts.expert(e))`` and ``nf4_linear_bnb(x, experts.expert(e))`` are
    the reference for ``forward``.  The weights are frozen: no gradient reaches them.
    """

    def __init__(self, in_features: int, out_features: int, packed: torch.Tensor, absmax: torch.Tensor,
                 absmax2: Optional[torch.Tensor], code2: Optional[torch.Tensor], offset: Optional[torch.Tensor],
                 dtype: torch.dtype, blocksize2: int = 256):
        super().__init__()
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.num_experts = int(packed.shape[0])
        self.blocksize, self.blocksize2 = 64, int(blocksize2)
        self.dtype = dtype
        N, K, E = self.out_features, self.in_features, self.num_experts
        nblk = N * K // 64
        self.nested = absmax.dtype == torch.uint8
        if N * K % 64 or tuple(packed.shape) != (E, N * K // 2) or packed.dtype != torch.uint8:
            raise ValueError(f"Experts4bit: packed must be uint8 [{E}, {N * K // 2}], got {packed.dtype} "
                             f"{tuple(packed.shape)}")
        if tuple(absmax.shape) != (E, nblk) or absmax.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"Experts4bit: absmax must be uint8 or float32 [{E}, {nblk}], got {absmax.dtype} "
                             f"{tuple(absmax.shape)}")
        if self.nested:
            n2 = (nblk + self.blocksize2 - 1) // self.blocksize2
            if absmax2 is None or code2 is None or offset is None:
                raise ValueError("Experts4bit: nested statistics need absmax2, code2 and offset")
            if tuple(absmax2.shape) != (E, n2) or code2.numel() != 256 or offset.numel() != E:
                raise ValueError(f"Experts4bit: expected absmax2 [{E}, {n2}], code2 [256] and offset [{E}], got "
                                 f"{tuple(absmax2.shape)}, {tuple(code2.shape)}, {tuple(offset.shape)}")
        else:
            absmax2 = code2 = offset = None
        self.weight = nn.Parameter(packed.contiguous(), requires_grad=False)
        self.absmax = absmax.contiguous()
        self.absmax2 = None if absmax2 is None else absmax2.to(torch.float32).contiguous()
        self.code2 = None if code2 is None else code2.to(torch.float32).contiguous().view(256)
        self.offset = None if offset is None else offset.to(torch.float32).contiguous().view(E)

    @classmethod
    def from_modules(cls, modules) -> "Experts4bit":
        """Stack existing ``Linear4bit`` modules (copies).  They must have one shape, one
        ``quant_state.dtype``, blocksize 64, no bias in use here (a bias is not carried), and all
        nested statistics (one blocksize2, one code2 table) or all fp32 ones: else ``ValueError``."""
        mods = list(modules)
        if not mods:
            raise ValueError("Experts4bit.from_modules: no modules")
        first = mods[0]
        qs0 = first.weight.quant_state
        N, K = int(first.out_features), int(first.in_features)
        nested0 = getattr(qs0, "state2", None) is not None and qs0.absmax.dtype == torch.uint8
        for i, m in enumerate(mods):
            qs = m.weight.quant_state
            nested = getattr(qs, "state2", None) is not None and qs.absmax.dtype == torch.uint8
            if (int(m.out_features), int(m.in_features)) != (N, K):
                raise ValueError(f"Experts4bit.from_modules: expert {i} is {int(m.out_features)} x {int(m.in_features)}, "
                                 f"expert 0 is {N} x {K}")
            if qs.dtype != qs0.dtype:
                raise ValueError(f"Experts4bit.from_modules: expert {i} has dtype {qs.dtype}, expert 0 {qs0.dtype}")
            if int(qs.blocksize) != 64:
                raise ValueError(f"Experts4bit.from_modules: expert {i} has blocksize {int(qs.blocksize)}, expected 64")
            if nested != nested0:
                raise ValueError("Experts4bit.from_modules: nested and fp32 statistics mixed")
            if m.weight.data.dtype != torch.uint8 or m.weight.data.numel() != N * K // 2 or N * K % 64:
                raise ValueError(f"Experts4bit.from_modules: expert {i}'s packed weight is not uint8 of N*K/2 bytes")
            if nested and (int(qs.state2.blocksize) != int(qs0.state2.blocksize)
                           or not torch.equal(qs.state2.code.to(qs0.state2.code.device), qs0.state2.code)):
                raise ValueError(f"Experts4bit.from_modules: expert {i} has another blocksize2 or code2 table")
        packed = torch.stack([m.weight.data.reshape(-1) for m in mods])
        absmax = torch.stack([m.weight.quant_state.absmax.reshape(-1) for m in mods])
        if not nested0:
            return cls(K, N, packed, absmax.to(torch.float32), None, None, None, qs0.dtype)
        dev = packed.device
        absmax2 = torch.stack([m.weight.quant_state.state2.absmax.reshape(-1).to(torch.float32) for m in mods])
        offs = []
        for m in mods:
            off = m.weight.quant_state.offset
            if off is None:
                off = 0.0
            offs.append(off.reshape(()).to(device=dev, dtype=torch.float32) if torch.is_tensor(off)
                        else torch.tensor(float(off), dtype=torch.float32, device=dev))
        return cls(K, N, packed, absmax, absmax2, qs0.state2.code.clone(), torch.stack(offs), qs0.dtype,
                   int(qs0.state2.blocksize))

    @classmethod
    def from_float(cls, weights, compute_dtype=None, compress_statistics: bool = True) -> "Experts4bit":
        """Quantize an ``[E, N, K]`` float tensor, or a list of ``nn.Linear`` modules / ``[N, K]``
        weights, one expert at a time through the HIP quantizer (``quantize.nf4_quantize``): the
        stacked bytes are those of E separate ``Linear4bit.from_float`` calls.  ``dtype`` (what
        ``forward`` returns) is ``compute_dtype`` if given, else the weights' dtype."""
        if torch.is_tensor(weights):
            if weights.dim() != 3:
                raise ValueError(f"Experts4bit.from_float: expected an [E, out_features, in_features] tensor, got "
                                 f"{tuple(weights.shape)}")
            items = list(weights.unbind(0))
        else:
            items = [w.weight if isinstance(w, nn.Module) else w for w in weights]
        return cls.from_modules([Linear4bit.from_float(w, compute_dtype=compute_dtype,
                                                       compress_statistics=compress_statistics, bias=None)
                                 for w in items])

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        dev = self.weight.device
        for name in ("absmax", "absmax2", "code2", "offset"):
            t = getattr(self, name)
            if t is not None and t.device != dev:
                setattr(self, name, t.to(dev))
        return self

    def expert(self, e: int) -> Linear4bit:
        """Expert ``e`` as a bias-free ``Linear4bit`` over VIEWS of this module's storage (no
        copy), as ``Embedding4bit.as_linear()`` gives the tied head."""
        e = int(e)
        if not 0 <= e < self.num_experts:
            raise IndexError(f"Experts4bit.expert: {e} outside 0..{self.num_experts - 1}")
        N, K = self.out_features, self.in_features
        if self.nested:
            state2 = QuantState(absmax=self.absmax2[e], code=self.code2, blocksize=self.blocksize2, quant_type=None,
                                dtype=torch.float32)
            qs = QuantState(absmax=self.absmax[e], shape=torch.Size((N, K)), code=NF4_CODE.to(self.weight.device),
                            blocksize=64, quant_type="nf4", dtype=self.dtype, offset=self.offset[e], state2=state2)
        else:
            qs = QuantState(absmax=self.absmax[e], shape=torch.Size((N, K)), code=NF4_CODE.to(self.weight.device),
                            blocksize=64, quant_type="nf4", dtype=self.dtype)
        lin = Linear4bit.__new__(Linear4bit)
        nn.Module.__init__(lin)
        lin.in_features, lin.out_features = K, N
        lin.compute_dtype = self.dtype
        lin.weight = Params4bit(self.weight.data[e].view(-1, 1), qs)
        lin.bias = None
        return lin

    def forward(self, x: torch.Tensor, expert_ids: torch.Tensor) -> torch.Tensor:
        """``y[t, j] = x[t] @ W_{expert_ids[t, j]}.t()`` (``x`` ``[T, K]``) or ``x[t, j] @ ...``
        (``x`` ``[T, k, K]``): ``kernel.nf4_moe_linear_bnb``."""
        from .kernel import nf4_moe_linear_bnb

        return nf4_moe_linear_bnb(x, self, expert_ids)
