"""The fused gate/up SwiGLU launch against what a caller did before it, one MI355X.

    python tools/bench_swiglu.py [--ms 1,8,32,33,48,64,96,128] [--pairs 10] [--rounds 7]
    python tools/bench_swiglu.py --sweep [--ms 64,128]     # named cfgs: 2 / 4 waves, 1..16 K slices

Workload: ``silu(gate(x)) * up(x)`` of a Llama-family MLP in bf16 with nested statistics, I x K =
14336 x 4096 (Llama-3-8B) and 11008 x 4096 (Llama-2-7B), for M rows of x.

Per shape ``--pairs`` distinct (gate, up) pairs (29 MB of packed bytes per 14336 x 4096 weight;
random bytes and statistics: the kernels' time does not depend on the values); call i of a graph
uses pair i % pairs, so with the default 10 pairs a graph reads 587 MB (450 MB at 11008) of
distinct packed bytes before one repeats: the weights stream from HBM, not from the 256 MB
Infinity Cache.

Three routes on the same packed bytes, each captured once as a graph of ``--pairs`` calls and
replayed in turn for ``--rounds`` rounds, timed with device events:

  fused   nf4_swiglu_bnb with its routed range opened to 1..128 rows: ONE launch
          (nf4_gemm_bnb_mt_swiglu), whatever the committed range says
  today   g, u = nf4_linear_bnb_grouped(x, [gate, up]); F.silu(g) * u -- one grouped launch up to 32
          rows, two row-tiled launches above, and two elementwise launches either way
  dequant nf4_dequant_bnb of both weights, two matmuls, the same elementwise launches: what
          dequantize_nf4_bnb + matmul runs, without its host read of the offset (read ahead of
          the timed region here, or the route could not be captured)

One JSON line per (shape, M): microseconds per call of every round, medians, each route's spread
(max - min over its rounds), today / fused per round, and ``fused_wins``: the fused median is
below today's by more than the larger of the two spreads -- the routing rule of
``SWIGLU_ROUTED_MIN_M`` / ``SWIGLU_ROUTED_MAX_M``.  ``--sweep``: per (shape, M) the C entry under
named cfgs (2 and 4 waves, every admissible count of K slices in 1..16) and the library's choice,
three timings each.
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
from nf4_triton_dequantization_amd import Experts4bit, _lib, kernel, nf4_linear_bnb_grouped, nf4_swiglu_bnb  # noqa: E402
from nf4_triton_dequantization_amd.bnb_layout import dynamic_map  # noqa: E402

SHAPES = [("llama3-8b", 14336, 4096), ("llama2-7b", 11008, 4096)]  # name, I, K


def random_pairs(pairs, n, k, dev, gen):
    """[(gate, up)] * pairs: bias-free Linear4bit views of one stack of random packed bytes and
    statistics of the size real ones have."""
    e, nblk = 2 * pairs, n * k // 64
    packed = torch.randint(0, 256, (e, n * k // 2), dtype=torch.uint8, device=dev, generator=gen)
    absmax = torch.randint(0, 256, (e, nblk), dtype=torch.uint8, device=dev, generator=gen)
    absmax2 = torch.rand((e, -(-nblk // 256)), device=dev, generator=gen) * 0.01 + 1e-3
    offset = torch.rand(e, device=dev, generator=gen) * 0.01 + 0.01
    ex = Experts4bit(k, n, packed, absmax, absmax2, dynamic_map(signed=True).to(dev), offset, torch.bfloat16)
    return ex, [(ex.expert(2 * i), ex.expert(2 * i + 1)) for i in range(pairs)]


def timed_rounds(fns, calls, rounds):
    """Each of fns (`calls` calls each) captured once, replayed in turn; microseconds per call of
    every round, in round order."""
    graphs = []
    side = torch.cuda.Stream()  # warm-up and capture on ONE stream: the per-stream workspace exists before the capture
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


def med(v):
    return sorted(v)[len(v) // 2]


def mat_of(mod, n):
    qs = mod.weight.quant_state
    q = mod.weight.data
    return _lib.GemmBnbMat(q.data_ptr(), q.numel(), qs.absmax.data_ptr(), qs.absmax.numel(), qs.state2.code.data_ptr(),
                           qs.state2.absmax.data_ptr(), qs.state2.absmax.numel(), qs.offset.data_ptr(), 64,
                           int(qs.state2.blocksize), None, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default=None, help="rows of x (default 1,8,32,33,48,64,96,128; --sweep: 64,128)")
    ap.add_argument("--shapes", default="llama3-8b,llama2-7b")
    ap.add_argument("--pairs", type=int, default=10, help="distinct (gate, up) pairs per shape = calls per graph")
    ap.add_argument("--rounds", type=int, default=7, help="interleaved replays")
    ap.add_argument("--sweep", action="store_true", help="named cfgs (waves, K slices) instead of the comparison")
    args = ap.parse_args()
    ms = [int(v) for v in (args.ms or ("64,128" if args.sweep else "1,8,32,33,48,64,96,128")).split(",")]
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    kernel.SWIGLU_ROUTED_MIN_M, kernel.SWIGLU_ROUTED_MAX_M = 1, 128  # the fused route at every M measured here
    for name, n, k in SHAPES:
        if name not in args.shapes.split(","):
            continue
        stack, mods = random_pairs(args.pairs, n, k, dev, gen)
        for M in ms:
            x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
            if args.sweep:
                h = torch.empty((M, n), dtype=torch.bfloat16, device=dev)
                descs = [(_lib.GemmBnbMat * 2)(mat_of(g, n), mat_of(u, n)) for g, u in mods]
                cfgs = [_lib.GemmCfg(_lib.GEMM_MT_SWIGLU, w, 1, ks, 2) for w in (4, 2) for ks in range(1, 17)
                        if ks <= k // 128] + [None]
                for cfg in cfgs:
                    cp = ctypes.byref(cfg) if cfg is not None else None
                    wsz = L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(M, n, k, cp)
                    work = torch.zeros(max(wsz, 1 << 16), dtype=torch.uint8, device=dev)

                    def fused():
                        sp = torch.cuda.current_stream().cuda_stream
                        for d in descs:
                            rc = L.nf4_gemm_bnb_mt_swiglu(x.data_ptr(), M, k, ctypes.cast(d, ctypes.c_void_p), 0, _lib.ACT_SILU,
                                                          h.data_ptr(), _lib.BF16, work.data_ptr() if wsz else None, wsz, cp, sp)
                            assert rc == 0, rc

                    (ts,) = timed_rounds((fused,), len(descs), 3)
                    assert int(work.count_nonzero()) == 0
                    print(json.dumps({"shape": name, "I": n, "K": k, "M": M,
                                      "waves": cfg.waves if cfg is not None else "library",
                                      "ksplit": cfg.ksplit if cfg is not None else "library",
                                      "us": [round(v, 3) for v in ts], "med": round(med(ts), 3)}), flush=True)
                continue

            def fused():
                for g, u in mods:
                    nf4_swiglu_bnb(x, g, u)

            def today():
                for g, u in mods:
                    a, b = nf4_linear_bnb_grouped(x, [g, u])
                    F.silu(a) * b

            offs = [[float(m.weight.quant_state.offset) for m in pair] for pair in mods]
            wtmp = torch.empty((2, n, k), dtype=torch.bfloat16, device=dev)

            def dequant():
                sp = torch.cuda.current_stream().cuda_stream
                for pair, off in zip(mods, offs):
                    for i, m in enumerate(pair):
                        qs = m.weight.quant_state
                        rc = L.nf4_dequant_bnb(m.weight.data.data_ptr(), qs.absmax.data_ptr(), qs.absmax.numel(),
                                               qs.state2.code.data_ptr(), qs.state2.absmax.data_ptr(), qs.state2.absmax.numel(),
                                               ctypes.c_float(off[i]), wtmp[i].data_ptr(), _lib.BF16, n * k, 64,
                                               int(qs.state2.blocksize), sp)
                        assert rc == 0, rc
                    F.silu(x @ wtmp[0].t()) * (x @ wtmp[1].t())

            with torch.no_grad():
                ta, tb, tc = timed_rounds((fused, today, dequant), len(mods), args.rounds)
            kernel.check_gemm_workspaces()
            spread = {r: max(t) - min(t) for r, t in (("fused", ta), ("today", tb), ("dequant", tc))}
            nblk = n * k // 64
            algo = 2 * (n * k // 2 + nblk + -(-nblk // 256) * 4) + M * k * 2 + M * n * 2
            print(json.dumps({"shape": name, "I": n, "K": k, "M": M, "calls": len(mods), "rounds": args.rounds,
                              "distinct_packed_mb": round(2 * len(mods) * n * k / 2 / 1e6, 1),
                              "fused_us": [round(v, 3) for v in ta], "today_us": [round(v, 3) for v in tb],
                              "dequant_us": [round(v, 3) for v in tc],
                              "fused_med": round(med(ta), 3), "today_med": round(med(tb), 3), "dequant_med": round(med(tc), 3),
                              "spread_us": {r: round(v, 3) for r, v in spread.items()},
                              "today_over_fused_per_round": [round(b / a, 4) for a, b in zip(ta, tb)],
                              "today_over_fused_med": round(med(tb) / med(ta), 4),
                              "dequant_over_fused_med": round(med(tc) / med(ta), 4),
                              "fused_wins": bool(med(tb) - med(ta) > max(spread["fused"], spread["today"])),
                              "algorithmic_bytes": int(algo), "fused_tb_per_s": round(algo / med(ta) / 1e6, 3)}), flush=True)
        del stack, mods


if __name__ == "__main__":
    main()
