"""The fused routes of the Python API as a list of calls, and a recording proxy around the loaded
library that notes what each call hands to the C ABI.  ``CASES[name](gpu, variant)`` builds one
call: the function, its arguments, the tensors whose pointers the entry must receive as they are,
the launch entries it must make and the routing constants it needs.  A ``variant`` replaces one
operand by one the host layer has to prepare (fp32 x, a strided x, x two bytes off alignment, int64
ids, an fp16 code2): same values, so the result is the clean call's bit for bit."""
import ctypes
from types import SimpleNamespace

import torch

from _gemm_bnb_cases import drawn_weight_bnb, single_weight_bnb

from nf4_triton_dequantization_amd import _lib

BF16, F32 = torch.bfloat16, torch.float32
K = 128
_CFG_TYPES = (ctypes.POINTER(_lib.GemmCfg),)
# (entry, argument index) -> (the structure the argument points to, how many: a number or the index of the count)
DESCRIPTORS = {
    ("nf4_gemm_ref_grouped", 3): (_lib.GemmMat, -4), ("nf4_gemm_grouped_workspace_bytes", 2): (_lib.GemmMat, -3),
    ("nf4_gemm_bnb_grouped", 3): (_lib.GemmBnbMat, -4), ("nf4_gemm_bnb_grouped_workspace_bytes", 2): (_lib.GemmBnbMat, -3),
    ("nf4_gemm_bnb_mt_swiglu", 3): (_lib.GemmBnbMat, 2),
    ("nf4_gemm_bnb_moe", 4): (_lib.MoeExperts, 1), ("nf4_gemm_bnb_moe_workspace_bytes", 1): (_lib.MoeExperts, 1),
    ("nf4_gemm_bnb_moe_rb", 4): (_lib.MoeExperts, 1), ("nf4_gemm_bnb_moe_rb_workspace_bytes", 1): (_lib.MoeExperts, 1),
    ("nf4_gemm_bnb_moe_swiglu", 4): (_lib.MoeExperts, 2),
    ("nf4_gemm_bnb_moe_swiglu_workspace_bytes", 1): (_lib.MoeExperts, 2),
    ("nf4_gemm_bnb_moe_down", 7): (_lib.MoeExperts, 1), ("nf4_gemm_bnb_moe_down_workspace_bytes", 1): (_lib.MoeExperts, 1),
    ("nf4_lora_add", 3): (_lib.LoraMat, -4), ("nf4_lora_add_routed", 5): (_lib.LoraStack, -6),
}


def _raw(v):
    return v.value if isinstance(v, ctypes._SimpleCData) else v


class Recorder:
    """The loaded library, forwarding every call and noting (entry, arguments, return value).  An
    argument is noted as ("ptr", address or None), ("int" / "float", value), ("cfg", address or None)
    or ("desc", [the fields of each structure it points to, read at the call])."""

    def __init__(self, handle):
        self._handle, self.calls = handle, []

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        types = _lib.SIGNATURES[name][1]

        def call(*args):
            noted = []
            for i, (a, ty) in enumerate(zip(args, types)):
                if (name, i) in DESCRIPTORS:
                    struct, count = DESCRIPTORS[name, i]
                    count = count if count > 0 else int(_raw(args[-count]))
                    arr = ctypes.cast(a, ctypes.POINTER(struct))
                    noted.append(("desc", [[("ptr" if fty is ctypes.c_void_p else "float" if fty is ctypes.c_float else "int",
                                             getattr(arr[j], f)) for f, fty in struct._fields_] for j in range(count)]))
                elif ty in _CFG_TYPES:
                    noted.append(("cfg", None if a is None else 1))
                elif ty is ctypes.c_void_p:
                    noted.append(("ptr", _raw(a) or None))
                else:
                    noted.append(("float" if ty is ctypes.c_float else "int", _raw(a)))
            assert len(args) == len(types), (name, len(args), len(types))
            rv = fn(*args)
            self.calls.append((name, noted, rv))
            return rv

        return call


def record(kmod, call):
    """Run ``call`` on ``kmod`` (a kernel module) behind a Recorder: (result, the calls noted)."""
    saved = {c: getattr(kmod, c) for c in call.consts}
    rec, real = Recorder(_lib.lib()), _lib.lib
    try:
        for c, v in call.consts.items():
            setattr(kmod, c, v)
        _lib.lib = lambda: rec
        with torch.no_grad():
            result = getattr(kmod, call.fn)(*call.args, **call.kwargs)
    finally:
        _lib.lib = real
        for c, v in saved.items():
            setattr(kmod, c, v)
    if isinstance(result, list):  # a grouped call: its results as one tensor
        result = torch.cat([r.reshape(-1) for r in result])
    return result, rec.calls


def launches(calls):
    return [c for c in calls if not c[0].endswith("_workspace_bytes")]


def normalise(calls, tensors, kmod, device):
    """The calls with every pointer replaced by what it is: null, the input tensor it equals ('?' for
    none of them: a temporary or an output the call allocated), a cached workspace of ``kmod``, the
    current stream -- and its value mod 16."""
    names = {t.data_ptr(): n for n, t in tensors.items()}
    for cache in ("_GEMM_WS", "_MOE_DOWN_WS"):
        for ws, _stream in getattr(kmod, cache).values():
            names[ws.data_ptr()] = cache
    stream = torch.cuda.current_stream(device).cuda_stream

    def norm(kind, v):
        if kind == "ptr":
            return "null" if not v else f"{names.get(v, '?')}%16={v % 16}"
        if kind == "cfg":
            return "cfg:null" if v is None else "cfg:set"
        if kind == "desc":
            return [[norm(k, f) for k, f in fields] for fields in v]
        return v

    out = []
    for name, args, rv in calls:
        rec = {"entry": name, "args": [norm(k, v) for k, v in args]}
        if name.endswith("_workspace_bytes"):
            rec["returns"] = rv
        elif not name.endswith("_cpu"):
            rec["args"][-1] = "stream:current" if (args[-1][1] or 0) == stream else "stream:other"
        out.append(rec)
    return out


def pointer_names(norm_calls):
    """Every tensor name that appears as a pointer, in an argument or in a descriptor."""
    found = set()

    def walk(v):
        if isinstance(v, str) and "%16=" in v:
            found.add(v.split("%16=")[0])
        elif isinstance(v, list):
            for e in v:
                walk(e)

    for rec in norm_calls:
        walk(rec["args"])
    return found


def expect_prepared(norm_clean, operand, copied_in, own_mod16):
    """What a variant's log must be, from the clean call's: in the entries of ``copied_in`` (None: all)
    the operand's pointer is a fresh 16-byte-aligned temporary, elsewhere the variant's own tensor."""
    def walk(v, copied):
        if isinstance(v, str) and v.split("%16=")[0] == operand:
            return "?%16=0" if copied else f"{operand}%16={own_mod16}"
        if isinstance(v, list):
            return [walk(e, copied) for e in v]
        return v

    return [{**rec, "args": walk(rec["args"], copied_in is None or rec["entry"] in copied_in)} for rec in norm_clean]


# ------------------------------------------------------------------------------------------ operands
def linear4(gpu, N, seed, nested=True, k=K):
    """A Linear4bit-shaped module [N, k] from the drawn weights of _gemm_bnb_cases.py (code2 rounded
    through fp16, so that an fp16 copy of it holds the same values)."""
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    if nested:
        packed, a1, code2, a2, offset = drawn_weight_bnb(N, k, seed=seed)
        st2 = SimpleNamespace(absmax=t(a2), code=t(code2).half().float(), blocksize=256)
        qs = SimpleNamespace(absmax=t(a1), state2=st2, offset=torch.tensor(offset, dtype=F32, device=gpu))
    else:
        packed, am = single_weight_bnb(N, k, seed=seed)
        qs = SimpleNamespace(absmax=t(am), state2=None, offset=None)
    qs.blocksize, qs.quant_type, qs.dtype, qs.shape = 64, "nf4", BF16, torch.Size((N, k))
    return SimpleNamespace(weight=SimpleNamespace(data=t(packed).view(-1, 1), quant_state=qs), out_features=N,
                           in_features=k, bias=None)


def _named(prefix, mod, reference=False):
    qs = mod.weight.quant_state
    d = {prefix + "packed": mod.weight.data, prefix + "absmax": qs.absmax}
    if qs.state2 is not None:
        d[prefix + "absmax2"] = qs.state2.absmax
        if not reference:
            d[prefix + "code2"] = qs.state2.code
            d[prefix + "offset"] = qs.offset
    return d


def _experts(gpu, seed, N=64):
    from nf4_triton_dequantization_amd import Experts4bit

    e = Experts4bit.from_modules([linear4(gpu, N, seed), linear4(gpu, N, seed + 1)])
    return e, {"packed": e.weight.data, "absmax": e.absmax, "code2": e.code2, "absmax2": e.absmax2, "offset": e.offset}


def _x(gpu, *shape, seed=0, variant=None):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(900 + seed)).to(BF16).to(gpu)
    if variant == "fp32_x":
        return x.float()
    if variant == "strided_x":
        big = torch.zeros(*shape[:-1], 2 * shape[-1], dtype=BF16, device=gpu)
        big[..., ::2] = x
        return big[..., ::2]
    if variant == "offset_x":
        buf = torch.zeros(x.numel() + 8, dtype=BF16, device=gpu)
        view = buf[1:1 + x.numel()].view(shape)
        view.copy_(x)
        assert view.data_ptr() % 16 == 2
        return view
    return x


def _fp16_code2(mods, variant):
    if variant == "fp16_code2":
        for m in mods:
            m.weight.quant_state.state2.code = m.weight.quant_state.state2.code.half()


def _call(fn, args, tensors, entries, kwargs=None, consts=None):
    return SimpleNamespace(fn=fn, args=args, kwargs=kwargs or {}, tensors=tensors, entries=entries, consts=consts or {})


X_ANY = ("fp32_x", "strided_x")
X_ALL = X_ANY + ("offset_x",)


def _linear(gpu, variant):
    mod = linear4(gpu, 64, 1)
    x = _x(gpu, 1, K, variant=variant)
    return _call("nf4_linear", (x, mod), {"x": x, **_named("w.", mod, reference=True)}, ["nf4_gemm_ref"])


def _linear_grouped(gpu, variant):
    mods = [linear4(gpu, 64, 2), linear4(gpu, 64, 3)]
    x = _x(gpu, 1, K, variant=variant)
    tensors = {"x": x, **_named("w0.", mods[0], reference=True), **_named("w1.", mods[1], reference=True)}
    return _call("nf4_linear_grouped", (x, mods), tensors, ["nf4_gemm_ref_grouped"])


def _linear_bnb(M, nested, entry):
    def build(gpu, variant):
        mod = linear4(gpu, 64, 4, nested=nested)
        _fp16_code2([mod], variant)
        x = _x(gpu, M, K, variant=variant)
        return _call("nf4_linear_bnb", (x, mod), {"x": x, **_named("w.", mod)}, [entry])
    return build


def _linear_bnb_grouped(gpu, variant):
    mods = [linear4(gpu, 64, 5), linear4(gpu, 128, 6)]
    _fp16_code2(mods[:1], variant)
    x = _x(gpu, 1, K, variant=variant)
    return _call("nf4_linear_bnb_grouped", (x, mods), {"x": x, **_named("w0.", mods[0]), **_named("w1.", mods[1])},
                 ["nf4_gemm_bnb_grouped"])


def _swiglu(gpu, variant):
    mods = [linear4(gpu, 64, 7), linear4(gpu, 64, 8)]
    _fp16_code2(mods[:1], variant)
    x = _x(gpu, 33, K, variant=variant)
    out = torch.empty(33, 64, dtype=BF16, device=gpu)
    tensors = {"x": x, "out": out, **_named("gate.", mods[0]), **_named("up.", mods[1])}
    return _call("nf4_swiglu_bnb", (x, *mods), tensors, ["nf4_gemm_bnb_mt_swiglu"], kwargs={"out": out})


def _ids(gpu, T, k, variant, hi=2):
    ids = torch.randint(0, hi, (T, k) if k else (T,), generator=torch.Generator().manual_seed(T)).to(torch.int32)
    return (ids.long() if variant == "int64_ids" else ids).to(gpu)


def _moe_linear(T, k, entry):
    def build(gpu, variant):
        e, named = _experts(gpu, 10)
        x, ids = _x(gpu, T, K, variant=variant), _ids(gpu, T, k, variant)
        out = torch.empty(T, k, 64, dtype=BF16, device=gpu)
        return _call("nf4_moe_linear_bnb", (x, e, ids), {"x": x, "ids": ids, "out": out, **named}, [entry],
                     kwargs={"out": out})
    return build


def _moe_swiglu(gpu, variant):
    (g, gn), (u, un) = _experts(gpu, 12), _experts(gpu, 14)
    x, ids = _x(gpu, 1, K, variant=variant), _ids(gpu, 1, 2, variant)
    out = torch.empty(1, 2, 64, dtype=BF16, device=gpu)
    tensors = {"x": x, "ids": ids, "out": out, **{"gate." + n: t for n, t in gn.items()},
               **{"up." + n: t for n, t in un.items()}}
    return _call("nf4_moe_swiglu_bnb", (x, g, u, ids), tensors, ["nf4_gemm_bnb_moe_swiglu"], kwargs={"out": out})


def _moe_down(gpu, variant):
    e, named = _experts(gpu, 16)
    h, ids = _x(gpu, 1, 2, K, variant=variant), _ids(gpu, 1, 2, variant)
    rw = torch.tensor([[0.75, 0.25]], dtype=F32, device=gpu)
    out = torch.empty(1, 64, dtype=BF16, device=gpu)
    return _call("nf4_moe_down_bnb", (h, e, ids, rw), {"x": h, "ids": ids, "rw": rw, "out": out, **named},
                 ["nf4_gemm_bnb_moe_down"], kwargs={"out": out},
                 consts={"MOE_DOWN_ROUTED_MIN_P": 1, "MOE_DOWN_ROUTED_MAX_P": 128})


def _lora(gpu, variant):
    mod = linear4(gpu, 64, 18)
    g = torch.Generator().manual_seed(18)
    A = (torch.randn(8, K, generator=g) / K ** 0.5).to(BF16).to(gpu)
    B = torch.randn(64, 8, generator=g).to(BF16).to(gpu)
    x = _x(gpu, 1, K, variant=variant)
    return _call("nf4_linear_lora_bnb", (x, mod, A, B, 0.5), {"x": x, "A": A, "B": B, **_named("w.", mod)},
                 ["nf4_gemm_bnb", "nf4_lora_add"], consts={"LORA_ROUTED_MIN_M": 1, "LORA_ROUTED_MAX_M": 128})


def _multilora(gpu, variant):
    mod = linear4(gpu, 64, 20)
    g = torch.Generator().manual_seed(20)
    A = (torch.randn(2, 8, K, generator=g) / K ** 0.5).to(BF16).to(gpu)
    B = torch.randn(2, 64, 8, generator=g).to(BF16).to(gpu)
    scaling = torch.tensor([0.5, 1.25], dtype=F32, device=gpu)
    x, ids = _x(gpu, 2, K, variant=variant), _ids(gpu, 2, 0, variant)
    tensors = {"x": x, "ids": ids, "A": A, "B": B, "scaling": scaling, **_named("w.", mod)}
    return _call("nf4_linear_multilora_bnb", (x, mod, A, B, scaling, ids), tensors, ["nf4_gemm_bnb", "nf4_lora_add_routed"])


def _embedding(gpu, variant):
    mod = linear4(gpu, 2, 22, k=64)
    _fp16_code2([mod], variant)
    ids = torch.tensor([1, 0, 1], dtype=torch.int64, device=gpu)
    out = torch.empty(3, 64, dtype=BF16, device=gpu)
    return _call("nf4_embedding_bnb", (ids, mod), {"ids": ids, "out": out, **_named("w.", mod)}, ["nf4_embedding_bnb"],
                 kwargs={"out": out})


TAILS = ("nf4_lora_add", "nf4_lora_add_routed")
# name: (builder, [(variant, the operand it replaces, the entries that get a copy of it -- None: all)])
CASES = {
    "nf4_linear": (_linear, [(v, "x", None) for v in X_ANY]),
    "nf4_linear_grouped": (_linear_grouped, [(v, "x", None) for v in X_ANY]),
    "nf4_linear_bnb-m1-nested": (_linear_bnb(1, True, "nf4_gemm_bnb"),
                                 [(v, "x", None) for v in X_ANY] + [("fp16_code2", "w.code2", None)]),
    "nf4_linear_bnb-m1-single": (_linear_bnb(1, False, "nf4_gemm_bnb_single"), [(v, "x", None) for v in X_ANY]),
    "nf4_linear_bnb-m33-row-tiled": (_linear_bnb(33, True, "nf4_gemm_bnb_mt"), [(v, "x", None) for v in X_ALL]),
    "nf4_linear_bnb_grouped": (_linear_bnb_grouped, [(v, "x", None) for v in X_ANY] + [("fp16_code2", "w0.code2", None)]),
    "nf4_swiglu_bnb": (_swiglu, [(v, "x", None) for v in X_ALL] + [("fp16_code2", "gate.code2", None)]),
    "nf4_moe_linear_bnb-p2": (_moe_linear(1, 2, "nf4_gemm_bnb_moe"),
                              [(v, "x", None) for v in X_ALL] + [("int64_ids", "ids", None)]),
    "nf4_moe_linear_bnb-p129-row-blocks": (_moe_linear(129, 1, "nf4_gemm_bnb_moe_rb"),
                                           [("offset_x", "x", None), ("int64_ids", "ids", None)]),
    "nf4_moe_swiglu_bnb": (_moe_swiglu, [(v, "x", None) for v in X_ALL] + [("int64_ids", "ids", None)]),
    "nf4_moe_down_bnb": (_moe_down, [(v, "x", None) for v in X_ALL] + [("int64_ids", "ids", None)]),
    "nf4_linear_lora_bnb": (_lora, [(v, "x", None) for v in X_ANY] + [("offset_x", "x", TAILS)]),
    "nf4_linear_multilora_bnb": (_multilora, [(v, "x", None) for v in X_ANY] + [("offset_x", "x", TAILS),
                                                                                  ("int64_ids", "ids", None)]),
    "nf4_embedding_bnb": (_embedding, [("fp16_code2", "w.code2", None)]),
}
