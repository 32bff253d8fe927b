"""The routed adapter launch (nf4_lora_add_routed) against the composite it replaces, one MI355X.

    python tools/bench_multilora.py [--what tail,single,linear] [--ms 1,8,32,64,128] [--ranks 16,64]
                                    [--shapes "4096,4096;14336,4096;4096,14336"] [--routings own,four,one]
                                    [--rounds 5] [--budget-mb 512] [--sweep]

One NF4 ``Linear4bit`` serves a batch whose rows belong to different LoRA adapters:
``y[m] = W x[m] + scaling[a] * B[a] (A[a] x[m])`` with ``a = adapter_ids[m]`` (bf16 throughout).
Routings: ``own`` every row its own adapter (S = min(M, 64)), ``four`` 4 adapters drawn uniformly,
``one`` a stack of 64 of which every row takes the same one.  Each measurement is a pair of routes
captured once as a graph and replayed in turn for ``--rounds`` rounds, timed with device events;
one JSON line each with every round's microseconds per call, the medians, each route's spread
(max - min over its rounds) and the ratios:

  tail    the adapters alone on a resident base result: one nf4_lora_add_routed (the library's
          cfg, in place on a copy of the base) against ``kernel._multilora_composite`` -- the
          gather of A[ids] and B[ids], two bmm, the scale and the select.  Adapter stacks rotate
          (8 per cell while they fit 256 MB, 2 at least), 48 calls per graph.
  single  the ``one`` routing against nf4_lora_add on the same adapter at the same M: what the
          slots, the routing and the idle workgroups cost.
  linear  base plus tail through ``nf4_linear_multilora_bnb``: with the routed range opened (the
          base launch, then nf4_lora_add_routed in place) against the range closed (the base launch
          and the composite).  The base weights rotate over ``--budget-mb`` of packed bytes per
          shape, more than the Infinity Cache holds, so they stream from HBM as in
          tools/bench_gemm.py; the weights share one adapter stack.

``--sweep`` times the tail under every cfg instead (tile_n x waves), for the plan's default rule.
Run it twice (run a, run b): the project's rule routes a row count only where, at every shape,
rank and routing, the slower run of the launch beats the faster run of the composite by more than
the spread.  The routes' results are compared before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nf4_triton_dequantization_amd import Linear4bit, _lib, kernel, nf4_linear_multilora_bnb  # noqa: E402

DT = torch.bfloat16
STACK_BUDGET = 256 << 20  # bytes of rotating adapter stacks per tail cell


def med(v):
    return sorted(v)[len(v) // 2]


def timed_rounds(fns, calls, rounds):
    """Each of fns (`calls` calls each) captured once, replayed in turn; microseconds per call of
    every round, in round order."""
    graphs = []
    side = torch.cuda.Stream()  # warm-up and capture on ONE stream: the per-stream workspaces exist before the capture
    for fn in fns:
        with torch.cuda.stream(side):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for g, ts in zip(graphs, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            g.replay()
            e1.record(st)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return out


def routed(on: bool):
    kernel.MULTILORA_ROUTED_MIN_M, kernel.MULTILORA_ROUTED_MAX_M = (1, 128) if on else (1, 0)


def report(what, tf, tc, other="composite", **fields):
    print(json.dumps({"what": what, **fields, "fused_us": [round(v, 3) for v in tf], f"{other}_us": [round(v, 3) for v in tc],
                      "fused_med": round(med(tf), 3), f"{other}_med": round(med(tc), 3),
                      "fused_spread": round(max(tf) - min(tf), 3), f"{other}_spread": round(max(tc) - min(tc), 3),
                      f"{other}_over_fused_per_round": [round(b / a, 4) for a, b in zip(tf, tc)],
                      f"{other}_over_fused_med": round(med(tc) / med(tf), 4)}), flush=True)


def close(a, b, what):
    d = float((a.float() - b.float()).abs().max())
    s = float(b.float().abs().max())
    assert d <= 2.0 ** -6 * s + 1e-3, f"{what}: the routes differ by {d} at a scale of {s}"


def make_routing(name, M, dev, gen):
    """(S, ids int32 [M])."""
    if name == "own":
        S = min(M, 64)
        return S, (torch.randperm(M, device=dev, generator=gen) % S).to(torch.int32)
    if name == "four":
        return 4, torch.randint(0, 4, (M,), device=dev, generator=gen).to(torch.int32)
    assert name == "one"
    return 64, torch.full((M,), 37, dtype=torch.int32, device=dev)


def stack(S, n, k, r, dev, gen):
    A = (torch.randn((S, r, k), device=dev, generator=gen) / k ** 0.5).to(DT)
    B = (torch.randn((S, n, r), device=dev, generator=gen) / r ** 0.5).to(DT)
    scaling = 0.5 + torch.rand((S,), device=dev, generator=gen)
    return A, B, scaling


def routed_add(L, x, ids, M, K, S, st, y, cfg=None):
    A, B, scaling = st
    r, n = A.shape[1], B.shape[1]
    d = (_lib.LoraStack * 1)(_lib.LoraStack(A.data_ptr(), B.data_ptr(), scaling.data_ptr(), y.data_ptr(), y.data_ptr(), n,
                                            r * K, n * r, r))
    c = _lib.LoraCfg(*cfg) if cfg is not None else None
    rc = L.nf4_lora_add_routed(x.data_ptr(), ids.data_ptr(), M, K, S, ctypes.cast(d, ctypes.c_void_p), 1, _lib.BF16,
                               ctypes.cast(ctypes.pointer(c), ctypes.c_void_p) if c is not None else None,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def lora_add(L, x, M, K, A, B, scale, y):
    d = (_lib.LoraMat * 1)(_lib.LoraMat(A.data_ptr(), B.data_ptr(), y.data_ptr(), y.data_ptr(), B.shape[0], A.shape[0], scale))
    rc = L.nf4_lora_add(x.data_ptr(), M, K, ctypes.cast(d, ctypes.c_void_p), 1, _lib.BF16, None,
                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def bench_tail(args, L, dev, gen, n, k, r, M, rname, what):
    calls = 48
    S, ids = make_routing(rname, M, dev, gen)
    copies = max(2, min(8, STACK_BUDGET // (S * r * (n + k) * 2)))
    stacks = [stack(S, n, k, r, dev, gen) for _ in range(copies)]
    x = torch.randn((M, k), device=dev, generator=gen).to(DT)
    base = torch.randn((M, n), device=dev, generator=gen).to(DT)
    y = base.clone()  # in place, as the API calls it: the values drift over the calls, the time does not

    def fused_with(cfg):
        def fused():
            for c in range(calls):
                routed_add(L, x, ids, M, k, S, stacks[c % copies], y, cfg)
        return fused

    def composite():
        for c in range(calls):
            kernel._multilora_composite(base, x, *stacks[c % copies], ids)

    def single():
        for c in range(calls):
            A, B, _ = stacks[c % copies]
            lora_add(L, x, M, k, A[37], B[37], 1.25, y)

    y.copy_(base)
    routed_add(L, x, ids, M, k, S, stacks[0], y)
    close(y, kernel._multilora_composite(base, x, *stacks[0], ids), f"tail {n}x{k} r={r} M={M} {rname}")
    y.copy_(base)
    fields = dict(N=n, K=k, r=r, M=M, routing=rname, S=S, calls=calls, stacks=copies)
    if args.sweep:
        cfgs = [(t, w) for t in (32, 64, 128, 256) for w in (1, 2, 4)]
        ts = timed_rounds([fused_with(None)] + [fused_with(c) for c in cfgs], calls, args.rounds)
        print(json.dumps({"what": "tail sweep", **fields, "default_med": round(med(ts[0]), 3),
                          "cfg_med": {f"{t}x{w}": round(med(v), 3) for (t, w), v in zip(cfgs, ts[1:])}}), flush=True)
        return
    if what == "single":
        tf, tc = timed_rounds((fused_with(None), single), calls, args.rounds)
        report("single", tf, tc, other="lora_add", **fields)
        return
    tf, tc = timed_rounds((fused_with(None), composite), calls, args.rounds)
    report("tail", tf, tc, **fields)


def quantized(n, k, dev, gen):
    w = torch.randn((n, k), device=dev, generator=gen, dtype=DT) * 0.02
    return Linear4bit.from_float(w, compute_dtype=DT)


def bench_linear(args, dev, gen, mods, st, n, k, r, M, rname, ids):
    x = torch.randn((M, k), device=dev, generator=gen).to(DT)

    def run():
        for m in mods:
            nf4_linear_multilora_bnb(x, m, *st, ids)

    def fused():
        routed(True)
        run()

    def composite():
        routed(False)
        run()

    routed(True)
    a = nf4_linear_multilora_bnb(x, mods[0], *st, ids)
    routed(False)
    close(a, nf4_linear_multilora_bnb(x, mods[0], *st, ids), f"linear {n}x{k} r={r} M={M} {rname}")
    tf, tc = timed_rounds((fused, composite), len(mods), args.rounds)
    report("linear", tf, tc, N=n, K=k, r=r, M=M, routing=rname, S=int(st[0].shape[0]), calls=len(mods))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="tail,single,linear")
    ap.add_argument("--ms", default="1,8,32,64,128")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--shapes", default="4096,4096;14336,4096;4096,14336", help="N,K;N,K;...")
    ap.add_argument("--routings", default="own,four,one")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays")
    ap.add_argument("--budget-mb", type=int, default=512, help="linear: packed bytes of a shape's rotation")
    ap.add_argument("--sweep", action="store_true", help="tail under every cfg instead of the comparison")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    what = args.what.split(",")
    ms = [int(v) for v in args.ms.split(",")]
    ranks = [int(v) for v in args.ranks.split(",")]
    routings = args.routings.split(",")
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";") if s]
    saved = kernel.MULTILORA_ROUTED_MIN_M, kernel.MULTILORA_ROUTED_MAX_M
    with torch.no_grad():
        if "tail" in what:
            for n, k in shapes:
                for r in ranks:
                    for M in ms:
                        for rname in routings:
                            bench_tail(args, L, dev, gen, n, k, r, M, rname, "tail")
                            torch.cuda.empty_cache()
        if "single" in what and not args.sweep:
            for n, k in shapes:
                for r in ranks:
                    for M in ms:
                        bench_tail(args, L, dev, gen, n, k, r, M, "one", "single")
                        torch.cuda.empty_cache()
        if "linear" in what and not args.sweep:
            for n, k in shapes:
                copies = max(8, args.budget_mb * (1 << 20) // (n * k // 2))
                mods = [quantized(n, k, dev, gen) for _ in range(copies)]
                for r in ranks:
                    for rname in routings:
                        for M in ms:
                            S, ids = make_routing(rname, M, dev, gen)
                            st = stack(S, n, k, r, dev, gen)
                            bench_linear(args, dev, gen, mods, st, n, k, r, M, rname, ids)
                            del st
                            torch.cuda.empty_cache()
                del mods
    kernel.MULTILORA_ROUTED_MIN_M, kernel.MULTILORA_ROUTED_MAX_M = saved


if __name__ == "__main__":
    main()
