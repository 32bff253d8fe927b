#!/usr/bin/env python3
"""Input-gradient GEMM measurement (profiles/gemm_dx/): the fused launch nf4_linear_bnb_dx
(dx = g . W, one launch, no 16-bit weight) against g @ dequantize(W) in its best case (the offset
read ahead of capture, which a real call does not arrange).

Default mode: graph replay, bf16, weights streaming from HBM -- every graph walks `copies` distinct
modules whose packed bytes together exceed the last-level cache several times.  Two runs per route,
each the median of `--rounds` replays; reported: the SLOWER run of the launch against the FASTER run
of the composite, and the spread of the rounds.
`--step` times one forward + backward per module, eager (autograd does not run under capture
here; the composite's forward reads the offset on the host, as a real call does): through
nf4_linear_bnb_autograd against nf4_linear_bnb's composite, the same two-run rule.
`--memory` gives torch.cuda.max_memory_allocated above the resident tensors for one forward +
backward of a 14336 x 4096 layer at 512 rows, and for a stack of eight such layers (each fed the
first 4096 columns of the one before), through both routes.
One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nf4_triton_dequantization_amd import Linear4bit, kernel

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]  # (N, K)
ROWS = [129, 512, 2048, 4096]
CACHE_BYTES = 1 << 30  # packed bytes a graph walks: four times the 256 MiB last-level cache


def modules(N, K, copies, dev):
    w = torch.randn((N, K), device=dev, dtype=torch.bfloat16) * 0.05
    mods = [Linear4bit.from_float(w.roll(i, 0), compute_dtype=torch.bfloat16) for i in range(copies)]
    for m in mods:  # the composite's best case: the offset as a Python number, read before any capture
        m.offset_read_ahead = float(m.weight.quant_state.offset)
    return mods


def composite_dx(g, m):
    """g @ dequantize(W) with the offset already on the host (no read inside the call)."""
    qs = m.weight.quant_state
    on_device, qs.offset = qs.offset, m.offset_read_ahead
    try:
        return g @ kernel.dequantize_nf4_bnb(m)
    finally:
        qs.offset = on_device


def replayed(fn, mods, rounds):
    """(median, spread) in us per call of fn(mod) over one graph that walks mods."""
    fn(mods[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for m in mods:
            fn(m)
    for _ in range(3):
        g.replay()
    return rounds_of(g.replay, len(mods), rounds)


def rounds_of(run, calls, rounds):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def step_routes(x, g):
    def run(linear, mods):
        for m in mods:
            xi = x.detach().requires_grad_()
            linear(xi, m).backward(g)
    return {"autograd": lambda mods: run(kernel.nf4_linear_bnb_autograd, mods),
            "composite": lambda mods: run(kernel.nf4_linear_bnb, mods)}


def peak(linear, mods, x):
    """Peak allocation of a forward + backward through mods above what was resident before it."""
    kernel.release_gemm_workspaces()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    h = x.detach().requires_grad_()
    y = h
    for m in mods:
        y = linear(y[..., :m.in_features], m)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="*", default=ROWS)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--memory", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.memory:
        N, K, M = 14336, 4096, 512
        mods = modules(N, K, 8, dev)
        x = torch.randn((M, K), device=dev, dtype=torch.bfloat16)
        for layers in (1, 8):
            out = {"memory": True, "N": N, "K": K, "M": M, "layers": layers, "weight_bf16_bytes": N * K * 2}
            for name, f in (("autograd", kernel.nf4_linear_bnb_autograd), ("composite", kernel.nf4_linear_bnb)):
                f(x.detach().requires_grad_(), mods[0]).sum().backward()  # warm: libraries, workspaces' first use
                out[name + "_peak_bytes"] = peak(f, mods[:layers], x)
            print(json.dumps(out), flush=True)
        return
    for N, K in (SHAPES[i] for i in a.shapes):
        copies = max(2, CACHE_BYTES // (N * K // 2))
        mods = modules(N, K, copies, dev)
        for M in a.rows:
            g = torch.randn((M, N), device=dev, dtype=torch.bfloat16)
            out = {"N": N, "K": K, "M": M, "copies": copies}
            if a.step:
                x = torch.randn((M, K), device=dev, dtype=torch.bfloat16)
                routes = step_routes(x, g)
                for f in routes.values():
                    f(mods[:1])
                runs = {k: [rounds_of(lambda: f(mods), len(mods), a.rounds) for _ in range(2)] for k, f in routes.items()}
                new, old = max(runs["autograd"]), min(runs["composite"])
                out.update(step=True, autograd_us=round(new[0], 1), autograd_spread=round(new[1], 4),
                           composite_us=round(old[0], 1), composite_spread=round(old[1], 4),
                           autograd_over_composite=round(new[0] / old[0], 3))
            else:
                with torch.no_grad():
                    routes = {"dx": lambda m: kernel.nf4_linear_bnb_dx(g, m), "composite": lambda m: composite_dx(g, m)}
                    runs = {k: [replayed(f, mods, a.rounds) for _ in range(2)] for k, f in routes.items()}
                new, old = max(runs["dx"]), min(runs["composite"])
                out.update(dx_us=round(new[0], 1), dx_spread=round(new[1], 4), dx_tflops=round(2 * M * N * K / new[0] / 1e6, 1),
                           composite_us=round(old[0], 1), composite_spread=round(old[1], 4),
                           dx_over_composite=round(new[0] / old[0], 3))
            print(json.dumps(out), flush=True)
        del mods
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
