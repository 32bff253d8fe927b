"""Host-side time per fused-GEMM call of two builds of libnf4dq.so (``--base`` another
build, e.g. the parent commit's; ``--new`` this tree's by default), interleaved in one
process: bursts of back-to-back calls on one stream (no sync inside a burst), the host clock
around the burst; the order of the two alternates burst by burst.

Three routes.  ``abi``: the C entries by ctypes, the same arguments every call (the floor).
``dq``: the same for the dequant entries -- nf4_dequant_ref on a flat (flat1 kernel), a
dense-chunk and a piece-kernel shape, nf4_dequant_ref_batched with 24 matrices, nf4_dequant_bnb.
``py``: the package's own functions -- ``nf4_linear`` / ``nf4_linear_grouped`` and, in bitsandbytes
semantics, ``nf4_linear_bnb``, ``nf4_linear_bnb_grouped``, ``nf4_moe_linear_bnb`` and
``nf4_linear_multilora_bnb`` -- (the whole call: argument preparation, output allocation, the ctypes
call); the library behind them is switched burst by burst through ``_lib._lib``, which all read on
every call.  ``--base-kernel PATH`` switches the Python module instead of the library: PATH is another
``kernel.py`` (the parent commit's, say), loaded beside this tree's as a second submodule of the
package; both run on this tree's library and only the ``py`` cases are run.

Weights have the real bitsandbytes layout (nb = N K / 64 absmax bytes, n2 = ceil(nb / 256)
nested scales), so absmax does not wrap inside a row and the library takes its first
choice: the GEMV at M = 1 up to 4096 columns, the persistent kernel otherwise (``wraps``
on the line is the plan's predicate in Python; the kernels that ran are named by a
``rocprofv3 --kernel-trace`` run of the same case with ``--only new --bursts 1``).

``host_us``: per call until the last call returned; ``drained_us``: until the stream
drained.  host_us is the host's own cost as long as the launch queue never fills: keep the
bursts short enough (1000 calls: the widest case here returns in 4.7 us per call against
16.6 us drained, so nothing blocked; where the two are equal the GPU was waiting for the
host, as on the py route).  One JSON line per case.

    python tools/gemm_host_cost_ab.py --base /path/to/parent/libnf4dq.so --out ab.jsonl
    python tools/gemm_host_cost_ab.py --base-kernel /path/to/parent/kernel.py --out ab.jsonl
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import nf4_triton_dequantization_amd as P  # noqa: E402
from nf4_triton_dequantization_amd import _lib  # noqa: E402

CASES = {  # name: (route, M, K, Ns)
    "abi_single_m1_4096x4096": ("abi", 1, 4096, (4096,)),
    "abi_grouped_qkv_m1": ("abi", 1, 4096, (4096, 1024, 1024)),
    "abi_single_m16_4096x4096": ("abi", 16, 4096, (4096,)),
    "abi_grouped_gate_up_m8": ("abi", 8, 4096, (14336, 14336)),
    "py_nf4_linear_m1_4096x4096": ("py", 1, 4096, (4096,)),
    "py_nf4_linear_grouped_qkv_m1": ("py", 1, 4096, (4096, 1024, 1024)),
    # bitsandbytes semantics, at shapes where the route is host-bound (host_us about drained_us)
    "py_nf4_linear_bnb_m1_4096x4096": ("py_bnb", 1, 4096, (4096,)),
    "py_nf4_linear_bnb_grouped_qkv_m1": ("py_bnb", 1, 4096, (4096, 1024, 1024)),
    "py_nf4_moe_linear_bnb_p2": ("py_moe", 1, 4096, (4096,)),  # 8 experts, one token, top-2
    "py_nf4_linear_multilora_bnb_m1": ("py_multilora", 1, 4096, (4096,)),  # 4 adapters of rank 16
}
DQ_CASES = {  # name: (entry, m, n, matrices)
    "dq_ref_4096x4096_flat1": ("ref", 4096, 4096, 1),
    "dq_ref_4096x4080_dense": ("ref", 4096, 4080, 1),
    "dq_ref_4096x4090_piece": ("ref", 4096, 4090, 1),
    "dq_ref_batched_24x1024x1024": ("batched", 1024, 1024, 24),
    "dq_bnb_4096x4096": ("bnb", 4096, 4096, 1),
}

ap = argparse.ArgumentParser()
ap.add_argument("--base", default=None, help="the library to compare against")
ap.add_argument("--base-kernel", default=None, help="another kernel.py to compare against, on this tree's library "
                                                    "(py cases only)")
ap.add_argument("--new", default=os.path.join(REPO, "nf4_triton_dequantization_amd", "_lib", "libnf4dq.so"))
ap.add_argument("--out", default="launch_cost_ab.jsonl")
ap.add_argument("--case", default="all", choices=["all", "gemm", "dq", *CASES, *DQ_CASES])
ap.add_argument("--calls", type=int, default=1000, help="calls per burst")
ap.add_argument("--bursts", type=int, default=20, help="timed bursts per library (one more, untimed, first)")
ap.add_argument("--only", default=None, choices=["new"], help="run this tree's library alone (kernel traces)")
ARGS = ap.parse_args()


def load(path):
    h = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(h, name):
            f = getattr(h, name)
            f.restype = res
            f.argtypes = args
    return h


def load_kernel(path):
    """Another kernel.py as a second submodule of the package, so that its relative imports resolve."""
    spec = importlib.util.spec_from_file_location(P.__name__ + ".kernel_base", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


# build -> (the library, the Python module) a burst runs on
LIBS = {"new": (load(ARGS.new), P.kernel)}
if ARGS.base_kernel:
    LIBS = {"parent": (LIBS["new"][0], load_kernel(ARGS.base_kernel)), **LIBS}
elif not ARGS.only:
    if not ARGS.base:
        ap.error("--base or --base-kernel is required unless --only new")
    LIBS = {"parent": (load(ARGS.base), P.kernel), **LIBS}
dev = torch.device("cuda", 0)
g = torch.Generator(device="cpu")
g.manual_seed(1)


def weight(N, K):
    nb = N * K // 64
    n2 = (nb + 255) // 256
    packed = torch.randint(0, 256, (N * K // 2,), dtype=torch.uint8, generator=g).to(dev)
    a1 = torch.randint(1, 256, (nb,), dtype=torch.uint8, generator=g).to(dev)
    a2 = (torch.rand(n2, generator=g) * 0.1 + 0.01).to(dev)
    return packed, a1, a2


def wraps(N, K, nb, n2):  # nf4_gemm_plan.h no_wrap_in_row, negated
    bpr = K // 64
    groups = (bpr + 3) // 4
    return not ((nb % bpr == 0 or nb >= N * bpr) and (n2 % groups == 0 or n2 >= N * groups))


def module(w, N, K):
    qs = SimpleNamespace(absmax=w[1], state2=SimpleNamespace(absmax=w[2]), dtype=torch.bfloat16)
    return SimpleNamespace(weight=SimpleNamespace(data=w[0].view(-1, 1), quant_state=qs), out_features=N,
                           in_features=K)


def bnb_module(w, N, K):
    """``module`` in bitsandbytes semantics: the code2 table, a device offset, the block sizes."""
    mod = module(w, N, K)
    qs = mod.weight.quant_state
    qs.state2.code = torch.sort(torch.rand(256, generator=g) * 2 - 1).values.to(dev)
    qs.state2.blocksize, qs.blocksize, qs.quant_type = 256, 64, "nf4"
    qs.offset, qs.shape = torch.tensor(0.0123, device=dev), torch.Size((N, K))
    return mod


def py_bnb_call(route, M, K, Ns, ws_t, x):
    """call(kernel module) -> the outputs, for the py cases in bitsandbytes semantics."""
    mods = [bnb_module(w, N, K) for w, N in zip(ws_t, Ns)]
    if route == "py_bnb" and len(Ns) == 1:
        return lambda kmod: [kmod.nf4_linear_bnb(x, mods[0])]
    if route == "py_bnb":
        return lambda kmod: kmod.nf4_linear_bnb_grouped(x, mods)
    if route == "py_moe":
        E, N = 8, Ns[0]
        st = [weight(N, K) for _ in range(E)]
        experts = P.Experts4bit(K, N, torch.stack([w[0] for w in st]), torch.stack([w[1] for w in st]),
                                torch.stack([w[2] for w in st]), mods[0].weight.quant_state.state2.code,
                                torch.full((E,), 0.0123, device=dev), torch.bfloat16)
        ids = torch.tensor([[3, 5]], dtype=torch.int32, device=dev)
        return lambda kmod: [kmod.nf4_moe_linear_bnb(x, experts, ids)]
    S, r, N = 4, 16, Ns[0]
    A = (torch.randn(S, r, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(dev)
    B = torch.randn(S, N, r, generator=g).to(torch.bfloat16).to(dev)
    scaling = torch.full((S,), 0.5, device=dev)
    ids = torch.randint(0, S, (M,), generator=g).to(torch.int32).to(dev)
    return lambda kmod: [kmod.nf4_linear_multilora_bnb(x, mods[0], A, B, scaling, ids)]


def dq_case(name):
    """(record head, burst(L, kmod, calls) -> (t0, t1, the outputs to compare)) of a dequant case."""
    entry, m, n, count = DQ_CASES[name]
    stride, bpr = (n + 1) // 2, (n + 63) // 64
    nb, n2 = m * bpr, m * ((bpr + 3) // 4)
    ps = [torch.randint(0, 256, (m * stride,), dtype=torch.uint8, generator=g).to(dev) for _ in range(count)]
    a1 = torch.randint(1, 256, (nb,), dtype=torch.uint8, generator=g).to(dev)
    a2 = (torch.rand(n2, generator=g) * 0.1 + 0.01).to(dev)
    code2 = torch.sort(torch.rand(256, generator=g) * 2 - 1).values.to(dev)
    outs = [torch.empty(m, n, dtype=torch.bfloat16, device=dev) for _ in range(count)]
    descs = (_lib.MatrixDesc * count)(*[_lib.MatrixDesc(p.data_ptr(), p.numel(), a1.data_ptr(), nb, a2.data_ptr(), n2,
                                                        o.data_ptr(), m, n) for p, o in zip(ps, outs)])
    st = torch.cuda.current_stream().cuda_stream

    def burst(L, _kmod, calls):
        if entry == "ref":
            f, a = L.nf4_dequant_ref, (ps[0].data_ptr(), ps[0].numel(), a1.data_ptr(), nb, a2.data_ptr(), n2,
                                       outs[0].data_ptr(), _lib.BF16, m, n, st)
        elif entry == "batched":
            f, a = L.nf4_dequant_ref_batched, (descs, count, _lib.BF16, st)
        else:
            f, a = L.nf4_dequant_bnb, (ps[0].data_ptr(), a1.data_ptr(), nb, code2.data_ptr(), a2.data_ptr(), n2, 0.0,
                                       outs[0].data_ptr(), _lib.BF16, m * n, 64, 256, st)
        rcs = 0
        t0 = time.perf_counter()
        for _ in range(calls):
            rcs |= f(*a)
        t1 = time.perf_counter()
        assert rcs == 0, rcs
        return t0, t1, outs

    return {"case": name, "route": "dq", "entry": entry, "m": m, "n": n, "matrices": count}, burst


def gemm_case(name):
    route, M, K, Ns = CASES[name]
    ws_t = [weight(N, K) for N in Ns]
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    ys = [torch.empty(M, N, dtype=torch.bfloat16, device=dev) for N in Ns]
    mats = (_lib.GemmMat * len(Ns))(*[_lib.GemmMat(w[0].data_ptr(), w[0].numel(), w[1].data_ptr(), w[1].numel(),
                                                   w[2].data_ptr(), w[2].numel(), y.data_ptr(), N)
                                      for w, y, N in zip(ws_t, ys, Ns)])
    mods = [module(w, N, K) for w, N in zip(ws_t, Ns)]
    st = torch.cuda.current_stream().cuda_stream
    py_bnb = py_bnb_call(route, M, K, Ns, ws_t, x) if route.startswith("py_") else None

    def burst(L, kmod, calls):
        if py_bnb is not None:
            _lib._lib = L  # the py route reads it on every call
            with torch.no_grad():
                py_bnb(kmod)  # the first call of a burst may allocate its workspace
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    last = py_bnb(kmod)
                t1 = time.perf_counter()
            return t0, t1, last
        if len(Ns) == 1:
            wsz = L.nf4_gemm_workspace_bytes(M, Ns[0], K)
        else:
            wsz = L.nf4_gemm_grouped_workspace_bytes(M, K, mats, len(Ns), None)
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=dev)
        w0 = ws_t[0]
        _lib._lib = L  # the py route reads it on every call
        last = None
        torch.cuda.synchronize()
        rcs = 0
        t0 = time.perf_counter()
        if route == "py" and len(Ns) == 1:
            for _ in range(calls):
                last = kmod.nf4_linear(x, mods[0])
        elif route == "py":
            for _ in range(calls):
                last = kmod.nf4_linear_grouped(x, mods)
        elif len(Ns) == 1:
            f = L.nf4_gemm_ref
            a = (x.data_ptr(), M, w0[0].data_ptr(), w0[0].numel(), w0[1].data_ptr(), w0[1].numel(),
                 w0[2].data_ptr(), w0[2].numel(), ys[0].data_ptr(), _lib.BF16, Ns[0], K, ws.data_ptr(), wsz, st)
            for _ in range(calls):
                rcs |= f(*a)
        else:
            f = L.nf4_gemm_ref_grouped
            a = (x.data_ptr(), M, K, mats, len(Ns), _lib.BF16, ws.data_ptr(), wsz, None, st)
            for _ in range(calls):
                rcs |= f(*a)
        t1 = time.perf_counter()
        assert rcs == 0, rcs
        return t0, t1, ys if route == "abi" else (last if isinstance(last, list) else [last])

    return {"case": name, "route": route, "M": M, "K": K, "Ns": list(Ns),
            "wraps": any(wraps(N, K, w[1].numel(), w[2].numel()) for w, N in zip(ws_t, Ns))}, burst


def case(name, out):
    calls, reps = ARGS.calls, ARGS.bursts
    rec, burst = dq_case(name) if name in DQ_CASES else gemm_case(name)
    rec.update(calls_per_burst=calls, bursts=reps)
    times = {k: [] for k in LIBS}
    outs = {}
    for rep in range(reps + 1):
        order = list(LIBS) if rep % 2 == 0 else list(LIBS)[::-1]
        for k in order:
            torch.cuda.synchronize()
            t0, t1, res = burst(*LIBS[k], calls)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            outs.setdefault(k, [y.clone() for y in res])
            if rep:  # the first round warms up
                times[k].append({"host_us": (t1 - t0) / calls * 1e6, "drained_us": (t2 - t0) / calls * 1e6})
    if "parent" in outs:
        rec["outputs_bit_identical"] = all(torch.equal(a.view(torch.int16), b.view(torch.int16))
                                           for a, b in zip(outs["parent"], outs["new"]))
    for k in LIBS:
        h = [t["host_us"] for t in times[k]]
        d = [t["drained_us"] for t in times[k]]
        rec[k] = {"host_us_median": round(statistics.median(h), 3), "host_us_min": round(min(h), 3),
                  "host_us_max": round(max(h), 3), "drained_us_median": round(statistics.median(d), 3),
                  "host_us": [round(v, 3) for v in h]}
    if "parent" in rec:
        p = rec["parent"]
        p["host_us_spread"] = round(p["host_us_max"] - p["host_us_min"], 3)  # of its own burst medians: the margin
        rec["host_us_delta"] = round(rec["new"]["host_us_median"] - p["host_us_median"], 3)
        rec["new_median_within_parent_spread"] = p["host_us_min"] <= rec["new"]["host_us_median"] <= p["host_us_max"]
        rec["new_median_within_or_below_parent_spread"] = rec["new"]["host_us_median"] <= p["host_us_max"]
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")
    out.flush()


with open(ARGS.out, "w") as out:
    groups = {"all": [*CASES, *DQ_CASES], "gemm": list(CASES), "dq": list(DQ_CASES)}
    for name in groups.get(ARGS.case, [ARGS.case]):
        if ARGS.base_kernel and not CASES.get(name, ("",))[0].startswith("py"):
            continue  # the C entries and the dequant cases never touch kernel.py
        case(name, out)
