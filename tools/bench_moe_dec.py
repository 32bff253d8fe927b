"""The slot launch nf4_gemm_bnb_moe_dec against nf4_gemm_bnb_moe and the per-expert loop, one MI355X.

    python tools/bench_moe_dec.py [--ts 1,4,16,64] [--stacks 3] [--rounds 5] [--calls 24] [--many]

Workload, rotation of the stacks, routings, capture and timing are tools/bench_moe.py's (whose
docstring describes them): Mixtral-8x7B's expert projections (8 experts, top-2, bf16, nested
statistics), w1 / w3 = 14336 x 4096 on the token's hidden state and w2 = 4096 x 14336 on per-pair
activations, T = 1, 4, 16, 64 tokens, weights streaming from HBM.  ``--many`` adds one many-expert
cell: 128 experts of 2048 x 4096 at top-8 and 4 tokens (32 pairs; two stacks of 537 MB).

Three contenders on the same packed bytes, each captured once as a graph of ``--calls`` calls and
replayed in turn for ``--rounds`` rounds, timed with device events:

  dec     nf4_gemm_bnb_moe_dec, the library's cfg: one launch per call, the ids read on the device
  moe     nf4_gemm_bnb_moe, the library's cfg: the same
  loop    the per-expert loop in its best case (bench_moe.py: index lists made on the host outside
          the timed region, x already sorted by expert, y left in that order)

The two fused launches' outputs of the last call are compared (the largest difference in units of
2^-8 of its row's largest output: bf16's last place there, or half of it).  One JSON line per (shape, T):
microseconds per call of every round and the medians, the achieved bytes/s of the slot launch from
its algorithmic bytes.
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
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench_moe as B  # noqa: E402
from nf4_triton_dequantization_amd import _lib, nf4_linear_bnb  # noqa: E402


def routing(T, top_k, E, call, rng):
    """ids [T, top_k] of one call: distinct experts per token (bench_moe.py's at Mixtral's sizes)."""
    if (E, top_k) == (B.E, B.TOP_K):
        return B.routing(T, call, rng)
    return torch.stack([torch.randperm(E, generator=rng)[:top_k] for _ in range(T)]).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="1,4,16,64", help="tokens per call")
    ap.add_argument("--stacks", type=int, default=3, help="distinct stacks of experts per shape (the rotation)")
    ap.add_argument("--calls", type=int, default=24, help="calls per graph")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays")
    ap.add_argument("--many", action="store_true", help="the many-expert cell alone: 128 experts, top-8, 4 tokens")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rng = torch.Generator()
    rng.manual_seed(1)
    cells = ([("128 experts", 2048, 4096, 8, 128, 8, [4])] if args.many else
             [(name, n, k, x_div, B.E, B.TOP_K, [int(v) for v in args.ts.split(",")]) for name, n, k, x_div in B.SHAPES])
    for name, n, k, x_div, E, top_k, ts in cells:
        B.E = E  # (random_stack's expert count)
        stacks = [B.random_stack(n, k, dev, gen) for _ in range(2 if args.many else args.stacks)]
        descs = [B.desc_of(ex) for ex in stacks]
        for T in ts:
            P = T * top_k
            rows = P // x_div
            x = torch.randn((rows, k), device=dev, generator=gen).to(torch.bfloat16)
            ids_host = [routing(T, top_k, E, c, rng) for c in range(args.calls)]
            ids_dev = [i.reshape(-1).to(dev) for i in ids_host]
            active = sum(len(set(i.reshape(-1).tolist())) for i in ids_host) / args.calls

            def fused_of(entry, size):
                wsz = max(size(P, dp, None) for _, dp in descs)
                work = torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev)
                y = torch.empty((P, n), dtype=torch.bfloat16, device=dev)

                def fused():
                    sp = torch.cuda.current_stream().cuda_stream
                    for c in range(args.calls):
                        _, dp = descs[c % len(descs)]
                        rc = entry(x.data_ptr(), ids_dev[c].data_ptr(), P, x_div, dp, y.data_ptr(), _lib.BF16,
                                   work.data_ptr() if wsz else None, wsz, None, sp)
                        assert rc == 0, rc
                return fused, work, y

            dec, dwork, ydec = fused_of(L.nf4_gemm_bnb_moe_dec, L.nf4_gemm_bnb_moe_dec_workspace_bytes)
            moe, mwork, ymoe = fused_of(L.nf4_gemm_bnb_moe, L.nf4_gemm_bnb_moe_workspace_bytes)

            slices, xs_sorted = [], []
            for ih in ids_host:
                flat = ih.reshape(-1)
                order = torch.argsort(flat, stable=True)
                xs_sorted.append(x[(order // x_div).to(dev)].contiguous())
                at, sl = 0, []
                for e, cnt in enumerate(torch.bincount(flat.to(torch.int64), minlength=E).tolist()):
                    if cnt:
                        sl.append((e, at, at + cnt))
                    at += cnt
                slices.append(sl)
            lins = [[ex.expert(e) for e in range(E)] for ex in stacks]

            def loop():
                for c in range(args.calls):
                    for e, a, b in slices[c]:
                        nf4_linear_bnb(xs_sorted[c][a:b], lins[c % len(stacks)][e])

            with torch.no_grad():
                td, tm, tl = B.timed_rounds((dec, moe, loop), args.calls, args.rounds)
            # (both y hold the last call's products: same inputs, two summation orders)
            a, b = ydec.float(), ymoe.float()
            unit = b.abs().amax(dim=1, keepdim=True).clamp_min(1e-30) * 2.0 ** -8
            worst = float(((a - b).abs() / unit).max())
            sp = torch.cuda.current_stream().cuda_stream
            for w in (dwork, mwork):
                assert L.nf4_gemm_check_workspace(w.data_ptr(), w.numel(), sp) == 0 and int(w.count_nonzero()) == 0
            nblk = n * k // 64
            algo = active * (n * k // 2 + nblk + -(-nblk // 256) * 4) + rows * k * 2 + P * n * 2
            med = B.med
            print(json.dumps({"what": name, "N": n, "K": k, "experts": E, "top_k": top_k, "T": T, "pairs": P, "x_div": x_div,
                              "calls": args.calls, "active_experts_per_call": round(active, 2),
                              "dec_us": [round(v, 3) for v in td], "moe_us": [round(v, 3) for v in tm],
                              "loop_us": [round(v, 3) for v in tl],
                              "dec_med": round(med(td), 3), "moe_med": round(med(tm), 3), "loop_med": round(med(tl), 3),
                              "dec_vs_moe_worst_in_row_last_places": round(worst, 3),
                              "algorithmic_bytes": int(algo), "dec_tb_per_s": round(algo / med(td) / 1e6, 3),
                              "dec_share_of_8tb_per_s": round(algo / med(td) / 1e6 / (B.PEAK / 1e12), 4)}), flush=True)
        del stacks, descs, lins


if __name__ == "__main__":
    main()
