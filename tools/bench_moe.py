"""Fused NF4 expert GEMM of a mixture-of-experts block against the per-expert loop, one MI355X.

    python tools/bench_moe.py [--ts 1,4,16,64] [--stacks 3] [--rounds 5] [--calls 24]
    python tools/bench_moe.py --sweep            # named cfgs: 1..16 K slices

Workload: the expert projections of Mixtral-8x7B (8 experts, top-2, bf16, nested statistics):
w1 / w3 = 14336 x 4096 applied to the token's hidden state (x [T, K], x_div = 2) and w2 = 4096 x
14336 applied to per-pair activations (x [T, 2, K], x_div = 1), for T = 1, 4, 16, 64 tokens.

Per shape ``--stacks`` distinct stacks of 8 experts (235 MB of packed bytes each; random bytes
and statistics: the kernels' time does not depend on the values) and per call a fresh routing:
at T = 1 call i goes to stack i % stacks, experts (2 i, 2 i + 1) % 8, so 12 calls touch all 24
experts (705 MB) before one repeats; from T = 4 on every token draws two distinct experts at
random and a call reads (nearly) a whole stack.  Either way the weights stream from HBM, not
from the 256 MB Infinity Cache.

Two contenders on the same packed bytes, each captured once as a graph of ``--calls`` calls and
replayed in turn for ``--rounds`` rounds, timed with device events:

  fused   nf4_gemm_bnb_moe: one launch per call, the ids read on the device
  loop    the per-expert loop: one nf4_linear_bnb call per ACTIVE expert on its row slice.  Its
          best case: the index lists are made on the host outside the timed region, x is already
          sorted by expert (no gather) and y stays in that order (no scatter), so the graph holds
          nothing but the per-expert fused launches (nf4_gemm_bnb below 33 rows, nf4_gemm_bnb_mt
          above).  The real loop also reads the routing back once per layer and cannot be
          captured at all.

One JSON line per (shape, T): microseconds per call of every round, medians, the ratio per round,
the achieved bytes/s of the fused launch from its algorithmic bytes (the active experts' packed
bytes and statistics, x and y).  ``--sweep``: per (shape, T) the fused launch under named cfgs
(4 waves, every admissible count of K slices in 1..16), three timings each.
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
from nf4_triton_dequantization_amd import Experts4bit, _lib, nf4_linear_bnb  # noqa: E402
from nf4_triton_dequantization_amd.bnb_layout import dynamic_map  # noqa: E402

E, TOP_K = 8, 2
SHAPES = [("w1/w3", 14336, 4096, TOP_K), ("w2", 4096, 14336, 1)]  # name, N, K, x_div
PEAK = 8e12


def random_stack(n, k, dev, gen):
    """An Experts4bit over random packed bytes and statistics of the size real ones have."""
    nblk = n * k // 64
    packed = torch.randint(0, 256, (E, n * k // 2), dtype=torch.uint8, device=dev, generator=gen)
    absmax = torch.randint(0, 256, (E, nblk), dtype=torch.uint8, device=dev, generator=gen)
    absmax2 = torch.rand((E, -(-nblk // 256)), device=dev, generator=gen) * 0.01 + 1e-3
    offset = torch.rand(E, device=dev, generator=gen) * 0.01 + 0.01
    return Experts4bit(k, n, packed, absmax, absmax2, dynamic_map(signed=True).to(dev), offset, torch.bfloat16)


def routing(T, call, rng):
    """ids [T, 2] of one call: two distinct experts per token."""
    if T == 1:
        return torch.tensor([[(2 * call) % E, (2 * call + 1) % E]], dtype=torch.int32)
    first = torch.randint(0, E, (T,), generator=rng)
    second = (first + torch.randint(1, E, (T,), generator=rng)) % E
    return torch.stack([first, second], dim=1).to(torch.int32)


def desc_of(ex):
    d = _lib.MoeExperts(ex.weight.data.data_ptr(), ex.weight.data.stride(0), ex.absmax.data_ptr(), ex.absmax.stride(0),
                        ex.code2.data_ptr(), 0, ex.absmax2.data_ptr(), ex.absmax2.stride(0), ex.offset.data_ptr(),
                        ex.out_features, ex.in_features, ex.num_experts, 0, 64, 256)
    return d, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)


def timed_rounds(fns, calls, rounds):
    """Each of fns (`calls` calls each) captured once, replayed in turn; microseconds per call of
    every round, in round order."""
    graphs = []
    side = torch.cuda.Stream()  # warm-up and capture on ONE stream: nf4_linear_bnb's per-stream workspace exists before the capture
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="1,4,16,64", help="tokens per call")
    ap.add_argument("--stacks", type=int, default=3, help="distinct stacks of 8 experts per shape (the rotation)")
    ap.add_argument("--calls", type=int, default=24, help="calls per graph")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays")
    ap.add_argument("--sweep", action="store_true", help="named cfgs (K slices) instead of the comparison")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rng = torch.Generator()
    rng.manual_seed(1)
    for name, n, k, x_div in SHAPES:
        stacks = [random_stack(n, k, dev, gen) for _ in range(args.stacks)]
        descs = [desc_of(ex) for ex in stacks]
        for T in [int(v) for v in args.ts.split(",")]:
            P = T * TOP_K
            rows = P // x_div
            x = torch.randn((rows, k), device=dev, generator=gen).to(torch.bfloat16)
            y = torch.empty((P, n), dtype=torch.bfloat16, device=dev)
            ids_host = [routing(T, c, rng) for c in range(args.calls)]
            ids_dev = [i.reshape(-1).to(dev) for i in ids_host]
            active = sum(len(set(i.reshape(-1).tolist())) for i in ids_host) / args.calls

            def fused_with(cfg):
                cp = ctypes.byref(cfg) if cfg is not None else None
                wsz = max(L.nf4_gemm_bnb_moe_workspace_bytes(P, dp, cp) for _, dp in descs)
                work = torch.zeros(max(wsz, 1 << 16), dtype=torch.uint8, device=dev)

                def fused():
                    sp = torch.cuda.current_stream().cuda_stream
                    for c in range(args.calls):
                        _, dp = descs[c % len(descs)]
                        rc = L.nf4_gemm_bnb_moe(x.data_ptr(), ids_dev[c].data_ptr(), P, x_div, dp, y.data_ptr(), _lib.BF16,
                                                work.data_ptr() if wsz else None, wsz, cp, sp)
                        assert rc == 0, rc
                return fused, work, wsz

            if args.sweep:
                for ks in range(1, 17):
                    cfg = _lib.GemmCfg(_lib.GEMM_MOE, 4, 1, ks, 2)
                    if ks > k // 128:
                        continue
                    fused, work, wsz = fused_with(cfg)
                    (ts,) = timed_rounds((fused,), args.calls, 3)
                    assert int(work.count_nonzero()) == 0
                    print(json.dumps({"what": name, "N": n, "K": k, "T": T, "pairs": P, "waves": 4, "ksplit": ks,
                                      "us": [round(v, 3) for v in ts], "med": round(med(ts), 3)}), flush=True)
                fused, work, wsz = fused_with(None)
                (ts,) = timed_rounds((fused,), args.calls, 3)
                print(json.dumps({"what": name, "N": n, "K": k, "T": T, "pairs": P, "ksplit": "library",
                                  "us": [round(v, 3) for v in ts], "med": round(med(ts), 3)}), flush=True)
                continue

            # the loop's best case: per call the pairs sorted by expert on the host, x gathered in
            # that order ahead of time, y left in that order
            slices, xs_sorted = [], []
            for c, ih in enumerate(ids_host):
                flat = ih.reshape(-1)
                order = torch.argsort(flat, stable=True)
                xs_sorted.append(x[(order // x_div).to(dev)].contiguous())
                counts = torch.bincount(flat.to(torch.int64), minlength=E).tolist()
                at, sl = 0, []
                for e, cnt in enumerate(counts):
                    if cnt:
                        sl.append((e, at, at + cnt))
                    at += cnt
                slices.append(sl)
            lins = [[ex.expert(e) for e in range(E)] for ex in stacks]

            def loop():
                for c in range(args.calls):
                    for e, a, b in slices[c]:
                        nf4_linear_bnb(xs_sorted[c][a:b], lins[c % len(stacks)][e])

            fused, work, wsz = fused_with(None)
            with torch.no_grad():
                tf, tl = timed_rounds((fused, loop), args.calls, args.rounds)
            if wsz:
                assert L.nf4_gemm_check_workspace(work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0
            assert int(work.count_nonzero()) == 0
            nblk = n * k // 64
            algo = active * (n * k // 2 + nblk + -(-nblk // 256) * 4) + rows * k * 2 + P * n * 2
            print(json.dumps({"what": name, "N": n, "K": k, "T": T, "pairs": P, "x_div": x_div, "calls": args.calls,
                              "stacks": args.stacks, "active_experts_per_call": round(active, 2),
                              "loop_launches_per_call": round(sum(len(s) for s in slices) / args.calls, 2),
                              "fused_us": [round(v, 3) for v in tf], "loop_us": [round(v, 3) for v in tl],
                              "fused_med": round(med(tf), 3), "loop_med": round(med(tl), 3),
                              "loop_over_fused_per_round": [round(b / a, 4) for a, b in zip(tf, tl)],
                              "loop_over_fused_med": round(med(tl) / med(tf), 4),
                              "algorithmic_bytes": int(algo), "fused_tb_per_s": round(algo / med(tf) / 1e6, 3),
                              "share_of_8tb_per_s": round(algo / med(tf) / 1e6 / (PEAK / 1e12), 4)}), flush=True)
        del stacks, descs


if __name__ == "__main__":
    main()
