"""The expert GEMM in row blocks (nf4_gemm_bnb_moe_rb, 129 .. 1024 pairs in one launch) against
what a caller could do without it, one MI355X.

    python tools/bench_moe_rb.py [--ts 128,256,512] [--stacks 3] [--rounds 5] [--calls 12]

Workload: the expert projections of Mixtral-8x7B (8 experts, top-2, bf16, nested statistics), as
tools/bench_moe.py builds them: w1 / w3 = 14336 x 4096 applied to the token's hidden state (x [T, K],
x_div = 2) and w2 = 4096 x 14336 applied to per-pair activations (x [T, 2, K], x_div = 1), for
T = 128, 256, 512 tokens (256, 512, 1024 pairs).  Per shape ``--stacks`` distinct stacks of 8
experts (235 MB of packed bytes each), call i on stack i % stacks with a fresh drawn routing (two
distinct experts per token), so the weights stream from HBM, not from the 256 MB Infinity Cache.

Three contenders on the same packed bytes, each captured once as a graph of ``--calls`` calls and
replayed in turn for ``--rounds`` rounds, timed with device events; the whole series runs twice:

  rb      nf4_gemm_bnb_moe_rb: one launch per call, the ids read on the device
  loop    the per-expert loop in its best case (tools/bench_moe.py): one nf4_linear_bnb call per
          active expert on its row slice, the index lists made on the host outside the timed
          region, x already sorted by expert and y left in that order; an expert with more than
          128 rows is called in slices of 128 (beyond them nf4_linear_bnb leaves its fused
          route).  The real loop reads the routing back once per expert and cannot be captured
          at all.
  slices  ceil(P / 128) launches of nf4_gemm_bnb_moe, each on 128 consecutive pairs: capturable
          and routed on the device, every launch reads every active expert's weight again.

One JSON line per (shape, T): microseconds per call of every round of both runs, the median of each
run, and the two ratios the project quotes: the FASTER run of an alternative over the SLOWER run
of the launch (above 1: the launch wins even so).
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
from bench_moe import E, SHAPES, TOP_K, desc_of, med, random_stack, routing, timed_rounds  # noqa: E402
from nf4_triton_dequantization_amd import _lib, nf4_linear_bnb  # noqa: E402
from nf4_triton_dequantization_amd.kernel import GEMM_MT_ROUTED_M as LOOP_ROWS  # noqa: E402  (rows of one fused nf4_linear_bnb call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="128,256,512", help="tokens per call")
    ap.add_argument("--stacks", type=int, default=3, help="distinct stacks of 8 experts per shape (the rotation)")
    ap.add_argument("--calls", type=int, default=12, help="calls per graph")
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
        for T in [int(v) for v in args.ts.split(",")]:
            P = T * TOP_K
            assert _lib.MOE_MAX_PAIRS < P <= _lib.MOE_RB_MAX_PAIRS, "this tool is about 129 .. 1024 pairs"
            rows = P // x_div
            x = torch.randn((rows, k), device=dev, generator=gen).to(torch.bfloat16)
            y = torch.empty((P, n), dtype=torch.bfloat16, device=dev)
            ids_host = [routing(T, c, rng) for c in range(args.calls)]
            ids_dev = [i.reshape(-1).to(dev) for i in ids_host]
            wsz = max(L.nf4_gemm_bnb_moe_rb_workspace_bytes(P, dp, None) for _, dp in descs)
            wsz_sl = max(L.nf4_gemm_bnb_moe_workspace_bytes(min(128, P), dp, None) for _, dp in descs)
            work = torch.zeros(max(wsz, wsz_sl, 1 << 16), dtype=torch.uint8, device=dev)

            def rb():
                sp = torch.cuda.current_stream().cuda_stream
                for c in range(args.calls):
                    _, dp = descs[c % len(descs)]
                    rc = L.nf4_gemm_bnb_moe_rb(x.data_ptr(), ids_dev[c].data_ptr(), P, x_div, dp, y.data_ptr(), _lib.BF16,
                                               work.data_ptr() if wsz else None, wsz, None, sp)
                    assert rc == 0, rc

            def slices128():
                sp = torch.cuda.current_stream().cuda_stream
                for c in range(args.calls):
                    _, dp = descs[c % len(descs)]
                    for s in range(0, P, 128):
                        q = min(128, P - s)
                        need = L.nf4_gemm_bnb_moe_workspace_bytes(q, dp, None)
                        rc = L.nf4_gemm_bnb_moe(x.data_ptr() + s // x_div * k * 2, ids_dev[c].data_ptr() + 4 * s, q, x_div, dp,
                                                y.data_ptr() + s * n * 2, _lib.BF16, work.data_ptr() if need else None, need,
                                                None, sp)
                        assert rc == 0, rc

            # the loop's best case: per call the pairs sorted by expert on the host, x gathered in
            # that order ahead of time, y left in that order
            per_expert, xs_sorted, rows_per_expert = [], [], []
            for ih in ids_host:
                flat = ih.reshape(-1)
                order = torch.argsort(flat, stable=True)
                xs_sorted.append(x[(order // x_div).to(dev)].contiguous())
                counts = torch.bincount(flat.to(torch.int64), minlength=E).tolist()
                rows_per_expert += [c for c in counts if c]
                at, sl = 0, []
                for e, cnt in enumerate(counts):
                    # (at most LOOP_ROWS rows a call: beyond them nf4_linear_bnb dequantizes and
                    # multiplies with torch, and reads the offset on the host -- not capturable)
                    for a in range(at, at + cnt, LOOP_ROWS):
                        sl.append((e, a, min(a + LOOP_ROWS, at + cnt)))
                    at += cnt
                per_expert.append(sl)

            def loop():
                for c in range(args.calls):
                    for e, a, b in per_expert[c]:
                        nf4_linear_bnb(xs_sorted[c][a:b], lins[c % len(stacks)][e])

            runs = []
            with torch.no_grad():
                for _ in range(2):
                    runs.append(timed_rounds((rb, loop, slices128), args.calls, args.rounds))
            if max(wsz, wsz_sl):
                assert L.nf4_gemm_check_workspace(work.data_ptr(), max(wsz, wsz_sl), torch.cuda.current_stream().cuda_stream) == 0
            assert int(work.count_nonzero()) == 0
            meds = {who: [med(run[i]) for run in runs] for i, who in enumerate(("rb", "loop", "slices"))}
            print(json.dumps({"what": name, "N": n, "K": k, "T": T, "pairs": P, "x_div": x_div, "calls": args.calls,
                              "stacks": args.stacks, "rounds": args.rounds,
                              "rows_per_expert_min_max": [min(rows_per_expert), max(rows_per_expert)],
                              "loop_launches_per_call": round(sum(len(sl) for sl in per_expert) / args.calls, 2),
                              "rb_ksplit_workspace_bytes": wsz,
                              "rb_us": [[round(v, 3) for v in run[0]] for run in runs],
                              "loop_us": [[round(v, 3) for v in run[1]] for run in runs],
                              "slices_us": [[round(v, 3) for v in run[2]] for run in runs],
                              "rb_med": [round(v, 3) for v in meds["rb"]], "loop_med": [round(v, 3) for v in meds["loop"]],
                              "slices_med": [round(v, 3) for v in meds["slices"]],
                              "faster_loop_over_slower_rb": round(min(meds["loop"]) / max(meds["rb"]), 4),
                              "faster_slices_over_slower_rb": round(min(meds["slices"]) / max(meds["rb"]), 4)}), flush=True)
        del stacks, descs, lins


if __name__ == "__main__":
    main()
