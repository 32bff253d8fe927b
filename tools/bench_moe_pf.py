"""The expert GEMM for prompts (nf4_gemm_bnb_moe_pf, 1 .. 16384 pairs in one call, routed on the
device) against what a caller could do without it, one MI355X.

    python tools/bench_moe_pf.py [--ts 512,1024,2048,4096,8192] [--stacks 3] [--rounds 5] [--calls 6]

Workload: the expert projections of Mixtral-8x7B (8 experts, top-2, bf16, nested statistics), as
tools/bench_moe.py builds them: w1 / w3 = 14336 x 4096 on the token's hidden state (x_div 2) and w2 =
4096 x 14336 on per-pair activations (x_div 1).  Per shape ``--stacks`` distinct stacks of 8 experts
(235 MB of packed bytes each), call i on stack i % stacks with a fresh drawn routing, so the weights
stream from HBM, not from the 256 MB Infinity Cache.

Contenders on the same packed bytes, each captured once as a graph of some calls and replayed in turn
for ``--rounds`` rounds, timed with device events; the whole series runs twice:

  pf      nf4_gemm_bnb_moe_pf under the library's cfg: routing kernel, GEMM and clear kernel per call
  loop    the per-expert loop in its BEST case: the index lists made on the host outside the timed
          region, x already sorted by expert, y left in that order, the offset read ahead of the
          capture; per active expert one dequantize to 16 bits and one torch matmul on its rows.
          The real loop (kernel._moe_fallback) reads the routing back once per expert, gathers and
          scatters, and cannot be captured at all.
  rb      nf4_gemm_bnb_moe_rb, at 1024 pairs only: the one cell both entries serve.

One JSON line per (shape, T): microseconds per call of every round of both runs, the median of each
run, the ratio FASTER run of an alternative over SLOWER run of the launch (above 1: the launch wins
even so), and the peak device memory a first call through the public functions adds
(nf4_moe_linear_bnb_prefill against nf4_moe_linear_bnb's loop), workspaces released before each.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_gemm_pf import composite  # noqa: E402
from bench_moe import E, SHAPES, TOP_K, desc_of, med, random_stack, routing, timed_rounds  # noqa: E402
from nf4_triton_dequantization_amd import _lib, kernel, nf4_moe_linear_bnb, nf4_moe_linear_bnb_prefill  # noqa: E402


def first_call_peak(fn):
    """Bytes of device memory one call of fn adds at its peak, the cached workspaces released first."""
    kernel.release_gemm_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="512,1024,2048,4096,8192", help="tokens per call")
    ap.add_argument("--stacks", type=int, default=3, help="distinct stacks of 8 experts per shape (the rotation)")
    ap.add_argument("--calls", type=int, default=6, help="calls per graph (a quarter of it above 2048 tokens)")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays per run")
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
        lins = [[ex.expert(e) for e in range(E)] for ex in stacks]
        for row in lins:
            for m in row:
                m.offset_read_ahead = float(m.weight.quant_state.offset)
        for T in [int(v) for v in args.ts.split(",")]:
            P = T * TOP_K
            assert 1 <= P <= _lib.MOE_PF_MAX_PAIRS
            calls = args.calls if T <= 2048 else max(2, args.calls // 4)
            x = torch.randn((P // x_div, k), device=dev, generator=gen).to(torch.bfloat16)
            y = torch.empty((P, n), dtype=torch.bfloat16, device=dev)
            ids_host = [routing(T, c, rng) for c in range(calls)]
            ids_dev = [i.reshape(-1).to(dev) for i in ids_host]
            with_rb = P <= _lib.MOE_RB_MAX_PAIRS
            wsz = max(L.nf4_gemm_bnb_moe_pf_workspace_bytes(P, dp, None) for _, dp in descs)
            wsz_rb = max(L.nf4_gemm_bnb_moe_rb_workspace_bytes(P, dp, None) for _, dp in descs) if with_rb else 0
            work = torch.zeros(max(wsz, wsz_rb), dtype=torch.uint8, device=dev)

            def pf():
                sp = torch.cuda.current_stream().cuda_stream
                for c in range(calls):
                    _, dp = descs[c % len(descs)]
                    rc = L.nf4_gemm_bnb_moe_pf(x.data_ptr(), ids_dev[c].data_ptr(), P, x_div, dp, y.data_ptr(), _lib.BF16,
                                               work.data_ptr(), wsz, None, sp)
                    assert rc == 0, rc

            def rb():
                sp = torch.cuda.current_stream().cuda_stream
                for c in range(calls):
                    _, dp = descs[c % len(descs)]
                    rc = L.nf4_gemm_bnb_moe_rb(x.data_ptr(), ids_dev[c].data_ptr(), P, x_div, dp, y.data_ptr(), _lib.BF16,
                                               work.data_ptr() if wsz_rb else None, wsz_rb, None, sp)
                    assert rc == 0, rc

            # the loop's best case: per call the pairs sorted by expert on the host, x gathered in that
            # order ahead of time, y left in that order
            per_expert, xs_sorted, rows_per_expert = [], [], []
            for ih in ids_host:
                flat = ih.reshape(-1)
                order = torch.argsort(flat, stable=True)
                xs_sorted.append(x[(order // x_div).to(dev)].contiguous())
                counts = torch.bincount(flat.to(torch.int64), minlength=E).tolist()
                rows_per_expert += [c for c in counts if c]
                at, sl = 0, []
                for e, cnt in enumerate(counts):
                    if cnt:
                        sl.append((e, at, at + cnt))
                    at += cnt
                per_expert.append(sl)

            def loop():
                for c in range(calls):
                    for e, a, b in per_expert[c]:
                        composite(xs_sorted[c][a:b], lins[c % len(stacks)][e])

            fns = (pf, loop, rb) if with_rb else (pf, loop)
            runs = []
            with torch.no_grad():
                for _ in range(2):
                    runs.append(timed_rounds(fns, calls, args.rounds))
                assert L.nf4_gemm_check_workspace(work.data_ptr(), work.numel(), torch.cuda.current_stream().cuda_stream) == 0
                assert int(work.count_nonzero()) == 0
                ids2 = ids_host[0].to(dev)
                x_api = x if x_div == TOP_K else x.view(T, TOP_K, k)
                peak_pf = first_call_peak(lambda: nf4_moe_linear_bnb_prefill(x_api, stacks[0], ids2))
                peak_loop = first_call_peak(lambda: nf4_moe_linear_bnb(x_api, stacks[0], ids2))
            meds = {who: [med(run[i]) for run in runs] for i, who in enumerate(("pf", "loop", "rb")[:len(fns)])}
            line = {"what": name, "N": n, "K": k, "T": T, "pairs": P, "x_div": x_div, "calls": calls, "stacks": args.stacks,
                    "rounds": args.rounds, "rows_per_expert_min_max": [min(rows_per_expert), max(rows_per_expert)],
                    "pf_workspace_bytes": wsz, "first_call_peak_bytes": {"prefill": peak_pf, "loop": peak_loop}}
            for i, who in enumerate(meds):
                line[f"{who}_us"] = [[round(v, 3) for v in run[i]] for run in runs]
                line[f"{who}_med"] = [round(v, 3) for v in meds[who]]
            line["pf_tflops"] = round(2.0 * P * n * k / (max(meds["pf"]) * 1e-6) / 1e12, 1)  # the slower run, routing and clear included
            line["faster_loop_over_slower_pf"] = round(min(meds["loop"]) / max(meds["pf"]), 4)
            if with_rb:
                line["faster_rb_over_slower_pf"] = round(min(meds["rb"]) / max(meds["pf"]), 4)
            print(json.dumps(line), flush=True)
            del xs_sorted, x, y
        del stacks, descs, lins


if __name__ == "__main__":
    main()
