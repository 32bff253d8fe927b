#!/usr/bin/env python3
"""Prefill GEMM measurement (profiles/gemm_pf/): the fused launch nf4_linear_bnb_prefill against
(b) dequantize + matmul in its best case (the offset read ahead of capture, which a real call
does not arrange) and (c) nf4_linear_bnb on ceil(M / 128) row slices, the best fused route without
the new entry: nf4_gemm_bnb_mt per full slice, and the <= 32-row family (nf4_gemm_bnb) for a
shorter tail such as the one row of M = 129.

Graph replay, bf16, weights streaming from HBM: every graph walks `copies` distinct modules whose
packed bytes together exceed the last-level cache several times.  Two runs per route, each the
median of `--rounds` replays; reported: the slower run of (a) against the faster run of each other
route, the spread of the rounds, and the memory of one FIRST call of (a) against (b): the peak
allocation above the resident tensors with the cached split-K workspaces released beforehand, so
(a)'s figure is y plus the workspace the call leaves cached (given separately as
pf_workspace_bytes, from nf4_gemm_bnb_pf_workspace_bytes; the cache's floor is 64 KiB), and
(b)'s is y plus the 16-bit weight.  `--sweep` times every
(waves, ksplit) of the prefill entry through the C ABI instead (the default rule's evidence).
One JSON line per measurement on stdout.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nf4_triton_dequantization_amd import Linear4bit, _lib, kernel

SHAPES = [(4096, 4096), (14336, 4096), (4096, 14336)]  # (N, K)
ROWS = [129, 256, 512, 1024, 2048, 4096]
CACHE_BYTES = 1 << 30  # packed bytes a graph walks: four times the 256 MiB last-level cache


def modules(N, K, copies, dev):
    w = torch.randn((N, K), device=dev, dtype=torch.bfloat16) * 0.05
    mods = [Linear4bit.from_float(w.roll(i, 0), compute_dtype=torch.bfloat16) for i in range(copies)]
    for m in mods:  # route (b)'s best case: the offset as a Python number, read before any capture
        m.offset_read_ahead = float(m.weight.quant_state.offset)
    return mods


def composite(x, m):
    """dequantize + matmul with the offset already on the host (no read inside the call)."""
    qs = m.weight.quant_state
    on_device, qs.offset = qs.offset, m.offset_read_ahead
    try:
        return x @ kernel.dequantize_nf4_bnb(m).t()
    finally:
        qs.offset = on_device


def timed(fn, mods, rounds):
    """(median, spread) in us per call of fn(mod) over one graph that walks mods."""
    fn(mods[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for m in mods:
            fn(m)
    for _ in range(3):
        g.replay()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / len(mods))
    del g
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def peak(fn, mod):
    """Peak allocation of one first call: no split-K workspace cached, nothing of an earlier call alive."""
    kernel.release_gemm_workspaces()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(mod)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def pf_cfg_call(x, mod, y, ws, cfg):
    """nf4_gemm_bnb_pf under a named cfg (the sweep)."""
    L, qs, keep = _lib.lib(), mod.weight.quant_state, []
    M, (N, K) = x.shape[0], (mod.out_features, mod.in_features)
    args = (x.data_ptr(), M, *kernel._operand(mod.weight.data, None, keep),
            *kernel._bnb_stats("bench", qs, x.device, keep), y.data_ptr(), _lib.BF16, N, K)
    need = L.nf4_gemm_bnb_pf_workspace_bytes(M, N, K, ctypes.byref(cfg))
    assert need <= ws.numel()
    _lib.check(L.nf4_gemm_bnb_pf(*args, ws.data_ptr() if need else None, need, ctypes.byref(cfg),
                                 torch.cuda.current_stream().cuda_stream), "sweep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="*", default=ROWS)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    for N, K in (SHAPES[i] for i in a.shapes):
        copies = max(2, CACHE_BYTES // (N * K // 2))
        mods = modules(N, K, copies, dev)
        for M in a.rows:
            x = torch.randn((M, K), device=dev, dtype=torch.bfloat16)
            with torch.no_grad():
                if a.sweep:
                    y = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
                    ws = torch.zeros((1 << 17) + 16 * M * N * 4, dtype=torch.uint8, device=dev)
                    for waves in (4, 8):
                        for ks in (1, 2, 4, 8, 16):
                            cfg = _lib.GemmCfg(_lib.GEMM_PF, waves, 1, ks, 0)
                            if ks > 1 and (-(-M // (32 * waves))) * (N // 128) * ks > 4 * 256:
                                continue  # a grid far beyond the CUs: slabs for nothing
                            us, spread = timed(lambda m: pf_cfg_call(x, m, y, ws, cfg), mods, a.rounds)
                            print(json.dumps({"sweep": True, "N": N, "K": K, "M": M, "waves": waves, "ksplit": ks,
                                              "us": round(us, 1), "spread": round(spread, 4)}), flush=True)
                    continue
                routes = {
                    "pf": lambda m: kernel.nf4_linear_bnb_prefill(x, m),
                    "composite": lambda m: composite(x, m),
                    "mt_slices": lambda m: [kernel.nf4_linear_bnb(x[r:r + 128], m) for r in range(0, M, 128)],
                }
                runs = {k: [timed(f, mods, a.rounds) for _ in range(2)] for k, f in routes.items()}
                pf = max(runs["pf"])
                out = {"N": N, "K": K, "M": M, "copies": copies, "pf_us": round(pf[0], 1), "pf_spread": round(pf[1], 4),
                       "pf_tflops": round(2 * M * N * K / pf[0] / 1e6, 1)}
                for k in ("composite", "mt_slices"):
                    best = min(runs[k])
                    out[k + "_us"], out[k + "_spread"] = round(best[0], 1), round(best[1], 4)
                    out["pf_over_" + k] = round(pf[0] / best[0], 3)
                out["pf_peak_bytes"] = peak(routes["pf"], mods[0])
                out["pf_workspace_bytes"] = _lib.lib().nf4_gemm_bnb_pf_workspace_bytes(M, N, K, None)
                out["composite_peak_bytes"] = peak(routes["composite"], mods[0])
                print(json.dumps(out), flush=True)
        del mods
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
