"""Fused NF4 expert down projection with the routed weighted sum against the composite it replaces,
one MI355X.

    python tools/bench_moe_down.py [--ts 1,4,16,64] [--stacks 3] [--rounds 5] [--calls 24]

Workload: the second half of Mixtral-8x7B's expert MLP (8 experts, top-2, bf16, nested statistics):
y[t] = sum_j rw[t, j] * w2_e(h[t, j]) with w2 = 4096 x 14336 applied to per-pair activations
(h [T, 2, K], x_div = 1), for T = 1, 4, 16, 64 tokens (2 / 8 / 32 / 128 pairs); fp32 routing weights.

``--stacks`` distinct stacks of 8 experts (235 MB of packed bytes each; random bytes and statistics:
the kernels' time does not depend on the values) and per call a fresh routing, as in
tools/bench_moe.py, so the weights stream from HBM, not from the 256 MB Infinity Cache.

Two contenders on the same packed bytes, each captured once as a graph of ``--calls`` calls and
replayed in turn for ``--rounds`` rounds, timed with device events:

  fused      nf4_gemm_bnb_moe_down: one launch per call, the library's cfg
  composite  what nf4_moe_mlp_bnb did before: nf4_moe_linear_bnb (one nf4_gemm_bnb_moe launch, the
             library's cfg -- the same waves and K slices), then ``.to``, ``*`` and ``.sum(dim=1)``
             in torch -- four launches, d [T, 2, N] through memory

One JSON line per T: microseconds per call of every round, medians, each route's spread (max - min
over its rounds) and the ratio per round.  Run it twice (run a, run b); the project's rule compares
the slower run of the fused launch with the faster run of the composite.  The fused results are
checked against the composite's, bit for bit, before anything is timed.
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
from bench_moe import TOP_K, desc_of, med, random_stack, routing, timed_rounds  # noqa: E402
from nf4_triton_dequantization_amd import _lib, nf4_moe_linear_bnb  # noqa: E402

N, K = 4096, 14336


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="1,4,16,64", help="tokens per call")
    ap.add_argument("--stacks", type=int, default=3, help="distinct stacks of 8 experts (the rotation)")
    ap.add_argument("--calls", type=int, default=24, help="calls per graph")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rng = torch.Generator()
    rng.manual_seed(1)
    stacks = [random_stack(N, K, dev, gen) for _ in range(args.stacks)]
    descs = [desc_of(ex) for ex in stacks]
    for T in [int(v) for v in args.ts.split(",")]:
        P = T * TOP_K
        h = torch.randn((T, TOP_K, K), device=dev, generator=gen).to(torch.bfloat16)
        rw = torch.rand((T, TOP_K), device=dev, generator=gen)
        y = torch.empty((T, N), dtype=torch.bfloat16, device=dev)
        d = torch.empty((T, TOP_K, N), dtype=torch.bfloat16, device=dev)
        ids_dev = [routing(T, c, rng).to(dev) for c in range(args.calls)]
        wsz = max(L.nf4_gemm_bnb_moe_down_workspace_bytes(P, dp, None) for _, dp in descs)
        work = torch.zeros(wsz, dtype=torch.uint8, device=dev)

        def fused_call(c):
            _, dp = descs[c % len(descs)]
            rc = L.nf4_gemm_bnb_moe_down(h.data_ptr(), ids_dev[c].data_ptr(), P, 1, TOP_K, rw.data_ptr(), _lib.F32, dp,
                                         y.data_ptr(), _lib.BF16, work.data_ptr(), wsz, None,
                                         torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc

        def composite_call(c):
            nf4_moe_linear_bnb(h, stacks[c % len(stacks)], ids_dev[c], out=d)
            return (d * rw.to(d.dtype).unsqueeze(-1)).sum(dim=1)

        def fused():
            for c in range(args.calls):
                fused_call(c)

        def composite():
            for c in range(args.calls):
                composite_call(c)

        with torch.no_grad():
            for c in range(min(args.calls, 2 * len(stacks))):  # the same bits before any timing
                fused_call(c)
                assert torch.equal(y, composite_call(c)), f"T={T} call {c}: the routes differ"
            tf, tc = timed_rounds((fused, composite), args.calls, args.rounds)
        scratch_at = wsz - P * N * 2
        assert L.nf4_gemm_check_workspace(work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0
        assert int(work[:scratch_at].count_nonzero()) == 0
        print(json.dumps({"what": "w2 down + routed sum", "N": N, "K": K, "T": T, "pairs": P, "calls": args.calls,
                          "stacks": args.stacks, "workspace_bytes": wsz,
                          "fused_us": [round(v, 3) for v in tf], "composite_us": [round(v, 3) for v in tc],
                          "fused_med": round(med(tf), 3), "composite_med": round(med(tc), 3),
                          "fused_spread": round(max(tf) - min(tf), 3), "composite_spread": round(max(tc) - min(tc), 3),
                          "composite_over_fused_per_round": [round(b / a, 4) for a, b in zip(tf, tc)],
                          "composite_over_fused_med": round(med(tc) / med(tf), 4)}), flush=True)


if __name__ == "__main__":
    main()
