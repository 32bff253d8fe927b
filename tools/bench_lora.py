"""The fused adapter launch (nf4_lora_add) against the four torch launches it replaces, one MI355X.

    python tools/bench_lora.py [--what tail,linear,pass] [--ms 1,8,32,64,128] [--ranks 16,64]
                               [--shapes "4096,4096;1024,4096;14336,4096;4096,14336"] [--rounds 5]
                               [--budget-mb 512] [--layers 32] [--sweep]

A ``Linear4bit`` with a LoRA adapter computes ``y = W x + scaling * B (A x)`` (bf16 throughout).
Three measurements, each a pair of routes captured once as a graph and replayed in turn for
``--rounds`` rounds, timed with device events; one JSON line each with every round's microseconds
per call, the medians, each route's spread (max - min over its rounds) and the ratios:

  tail    the adapter alone on a resident base result: one nf4_lora_add (the library's cfg)
          against ``base + F.linear(F.linear(x, A), B) * scaling`` -- four launches.  Eight
          adapters per shape in rotation, 48 calls per graph.
  linear  base plus adapter through ``nf4_linear_lora_bnb``: with the routed range opened (the
          base launch, then nf4_lora_add in place) against the range closed (the base launch and
          the four torch launches).  The base weights rotate over ``--budget-mb`` of packed bytes
          per shape, more than the Infinity Cache holds, so they stream from HBM as in
          tools/bench_gemm.py; every weight has its own adapter.
  pass    Llama-3-8B's 224 linears with an adapter on every one, q/k/v and gate/up through
          ``nf4_linear_lora_bnb_grouped`` (one nf4_lora_add per group), against the same pass
          with the range closed; up to 32 rows (the grouped base launch's range).

``--sweep`` times the tail under every cfg instead (tile_n x waves), for the plan's default rule.
Run it twice (run a, run b): the project's rule routes a row count only where, at every shape and
rank, the slower run of the fused route beats the faster run of the composite by more than the
spread.  The routes' results are compared before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nf4_triton_dequantization_amd import (Linear4bit, _lib, kernel, nf4_linear_lora_bnb,  # noqa: E402
                                           nf4_linear_lora_bnb_grouped)

LLAMA = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336)]  # q k v o gate up down
SCALING = 2.0
DT = torch.bfloat16


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
    kernel.LORA_ROUTED_MIN_M, kernel.LORA_ROUTED_MAX_M = (1, 128) if on else (1, 0)


def report(what, tf, tc, **fields):
    print(json.dumps({"what": what, **fields, "fused_us": [round(v, 3) for v in tf], "composite_us": [round(v, 3) for v in tc],
                      "fused_med": round(med(tf), 3), "composite_med": round(med(tc), 3),
                      "fused_spread": round(max(tf) - min(tf), 3), "composite_spread": round(max(tc) - min(tc), 3),
                      "composite_over_fused_per_round": [round(b / a, 4) for a, b in zip(tf, tc)],
                      "composite_over_fused_med": round(med(tc) / med(tf), 4)}), flush=True)


def close(a, b, what):
    d = float((a.float() - b.float()).abs().max())
    s = float(b.float().abs().max())
    assert d <= 2.0 ** -6 * s + 1e-3, f"{what}: the routes differ by {d} at a scale of {s}"


def adapter(n, k, r, dev, gen):
    A = (torch.randn((r, k), device=dev, generator=gen) / k ** 0.5).to(DT)
    B = (torch.randn((n, r), device=dev, generator=gen) / r ** 0.5).to(DT)
    return A, B


def lora_add(L, x, M, K, A, B, base, y, cfg=None):
    d = (_lib.LoraMat * 1)(_lib.LoraMat(A.data_ptr(), B.data_ptr(), base.data_ptr(), y.data_ptr(), B.shape[0], A.shape[0],
                                        SCALING))
    c = _lib.LoraCfg(*cfg) if cfg is not None else None
    rc = L.nf4_lora_add(x.data_ptr(), M, K, ctypes.cast(d, ctypes.c_void_p), 1, _lib.BF16,
                        ctypes.cast(ctypes.pointer(c), ctypes.c_void_p) if c is not None else None,
                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def bench_tail(args, L, dev, gen, n, k, r, M):
    copies, calls = 8, 48
    ads = [adapter(n, k, r, dev, gen) for _ in range(copies)]
    x = torch.randn((M, k), device=dev, generator=gen).to(DT)
    base = torch.randn((M, n), device=dev, generator=gen).to(DT)
    y = torch.empty_like(base)

    def fused_with(cfg):
        def fused():
            for c in range(calls):
                lora_add(L, x, M, k, *ads[c % copies], base, y, cfg)
        return fused

    def composite_call(c):
        A, B = ads[c % copies]
        return base + F.linear(F.linear(x, A), B) * SCALING

    def composite():
        for c in range(calls):
            composite_call(c)

    lora_add(L, x, M, k, *ads[0], base, y)
    close(y, composite_call(0), f"tail {n}x{k} r={r} M={M}")
    if args.sweep:
        cfgs = [(t, w) for t in (32, 64, 128, 256) for w in (1, 2, 4)]
        ts = timed_rounds([fused_with(None)] + [fused_with(c) for c in cfgs], calls, args.rounds)
        print(json.dumps({"what": "tail sweep", "N": n, "K": k, "r": r, "M": M, "default_med": round(med(ts[0]), 3),
                          "cfg_med": {f"{t}x{w}": round(med(v), 3) for (t, w), v in zip(cfgs, ts[1:])}}), flush=True)
        return
    tf, tc = timed_rounds((fused_with(None), composite), calls, args.rounds)
    report("tail", tf, tc, N=n, K=k, r=r, M=M, calls=calls)


def quantized(n, k, dev, gen):
    w = torch.randn((n, k), device=dev, generator=gen, dtype=DT) * 0.02
    return Linear4bit.from_float(w, compute_dtype=DT)


def bench_linear(args, dev, gen, mods, ads, n, k, r, M):
    x = torch.randn((M, k), device=dev, generator=gen).to(DT)

    def run():
        for m, (A, B) in zip(mods, ads):
            nf4_linear_lora_bnb(x, m, A, B, SCALING)

    def fused():
        routed(True)
        run()

    def composite():
        routed(False)
        run()

    routed(True)
    a = nf4_linear_lora_bnb(x, mods[0], *ads[0], SCALING)
    routed(False)
    close(a, nf4_linear_lora_bnb(x, mods[0], *ads[0], SCALING), f"linear {n}x{k} r={r} M={M}")
    tf, tc = timed_rounds((fused, composite), len(mods), args.rounds)
    report("linear", tf, tc, N=n, K=k, r=r, M=M, calls=len(mods))


def bench_pass(args, dev, gen, layers, r, M):
    x = {k: torch.randn((M, k), device=dev, generator=gen).to(DT) for k in (4096, 14336)}

    def run():
        for mods, ads in layers:
            q, kk, v, o, gate, up, down = mods
            aq, ak, av, ao, ag, au, ad = ads
            nf4_linear_lora_bnb_grouped(x[4096], [q, kk, v], [(*aq, SCALING), (*ak, SCALING), (*av, SCALING)])
            nf4_linear_lora_bnb(x[4096], o, *ao, SCALING)
            nf4_linear_lora_bnb_grouped(x[4096], [gate, up], [(*ag, SCALING), (*au, SCALING)])
            nf4_linear_lora_bnb(x[14336], down, *ad, SCALING)

    def fused():
        routed(True)
        run()

    def composite():
        routed(False)
        run()

    tf, tc = timed_rounds((fused, composite), 1, args.rounds)
    report("pass", tf, tc, linears=7 * len(layers), r=r, M=M, unit="us per pass")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="tail,linear,pass")
    ap.add_argument("--ms", default="1,8,32,64,128")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--shapes", default="4096,4096;1024,4096;14336,4096;4096,14336", help="N,K;N,K;...")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays")
    ap.add_argument("--budget-mb", type=int, default=512, help="linear: packed bytes of a shape's rotation")
    ap.add_argument("--layers", type=int, default=32, help="pass: layers of 7 linears")
    ap.add_argument("--sweep", action="store_true", help="tail under every cfg instead of the comparison")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    what = args.what.split(",")
    ms = [int(v) for v in args.ms.split(",")]
    ranks = [int(v) for v in args.ranks.split(",")]
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";") if s]
    saved = kernel.LORA_ROUTED_MIN_M, kernel.LORA_ROUTED_MAX_M
    with torch.no_grad():
        if "tail" in what:
            for n, k in shapes:
                for r in ranks:
                    for M in ms:
                        bench_tail(args, L, dev, gen, n, k, r, M)
        if "linear" in what and not args.sweep:
            for n, k in shapes:
                copies = max(8, args.budget_mb * (1 << 20) // (n * k // 2))
                mods = [quantized(n, k, dev, gen) for _ in range(copies)]
                for r in ranks:
                    ads = [adapter(n, k, r, dev, gen) for _ in mods]
                    for M in ms:
                        bench_linear(args, dev, gen, mods, ads, n, k, r, M)
                del mods
        if "pass" in what and not args.sweep and args.layers > 0:
            mods = [[quantized(n, k, dev, gen) for n, k in LLAMA] for _ in range(args.layers)]
            for r in ranks:
                layers = [(m, [adapter(n, k, r, dev, gen) for n, k in LLAMA]) for m in mods]
                for M in [m for m in ms if m <= _lib.GEMM_MAX_M]:
                    bench_pass(args, dev, gen, layers, r, M)
    kernel.LORA_ROUTED_MIN_M, kernel.LORA_ROUTED_MAX_M = saved


if __name__ == "__main__":
    main()
