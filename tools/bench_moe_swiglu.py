"""Fused NF4 expert SwiGLU launch of a mixture-of-experts block against the composite it replaces,
one MI355X.

    python tools/bench_moe_swiglu.py [--ts 1,4,16,64] [--stacks 2] [--rounds 5] [--calls 16]
    python tools/bench_moe_swiglu.py --sweep      # named cfgs: waves 2 / 4 x 1..16 K slices

Workload: the first half of Mixtral-8x7B's expert MLP (8 experts, top-2, bf16, nested statistics):
h = silu(w1(x)) * w3(x) per (token, choice) pair with w1 / w3 = 14336 x 4096 applied to the token's
hidden state (x [T, K], x_div = 2), for T = 1, 4, 16, 64 tokens (2 / 8 / 32 / 128 pairs).

``--stacks`` distinct (w1, w3) pairs of stacks of 8 experts (2 x 235 MB of packed bytes each; random
bytes and statistics: the kernels' time does not depend on the values) and per call a fresh
routing, as in tools/bench_moe.py: at T = 1 call i goes to pair i % stacks, experts
(2 i, 2 i + 1) % 8, so 8 calls touch all experts of two pairs (940 MB) before one repeats; from
T = 4 on every token draws two distinct experts at random and a call reads (nearly) a whole pair of
stacks.  Either way the weights stream from HBM, not from the 256 MB Infinity Cache.

Two contenders on the same packed bytes, each captured once as a graph of ``--calls`` calls and
replayed in turn for ``--rounds`` rounds, timed with device events:

  fused      nf4_gemm_bnb_moe_swiglu: one launch per call, the library's cfg
  composite  what a caller wrote before: nf4_moe_linear_bnb on w1, nf4_moe_linear_bnb on w3 (one
             nf4_gemm_bnb_moe launch each, the library's cfg), then F.silu(g) * u (two elementwise
             launches) -- four launches, g and u through memory

One JSON line per T: microseconds per call of every round, medians, the ratio per round, the
achieved bytes/s of the fused launch from its algorithmic bytes (the active experts' packed bytes
and statistics of both stacks, x and h).  The per-expert loop of tools/bench_moe.py's comparison
is a different contender (it needs the routing on the host) and is not run here.
``--sweep``: per T the fused launch under named cfgs (2 and 4 waves, every admissible count of K
slices in 1..16; a slice costs two planes), three timings each, and the library's choice.
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
from bench_moe import E, PEAK, TOP_K, desc_of, med, random_stack, routing, timed_rounds  # noqa: E402
from nf4_triton_dequantization_amd import _lib, nf4_moe_linear_bnb  # noqa: E402

I, K = 14336, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="1,4,16,64", help="tokens per call")
    ap.add_argument("--stacks", type=int, default=2, help="distinct (w1, w3) pairs of stacks (the rotation)")
    ap.add_argument("--calls", type=int, default=16, help="calls per graph")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved replays")
    ap.add_argument("--sweep", action="store_true", help="named cfgs (waves x K slices) instead of the comparison")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rng = torch.Generator()
    rng.manual_seed(1)
    pairs = [(random_stack(I, K, dev, gen), random_stack(I, K, dev, gen)) for _ in range(args.stacks)]
    descs = []
    for w1, w3 in pairs:
        arr = (_lib.MoeExperts * 2)(desc_of(w1)[0], desc_of(w3)[0])
        descs.append((arr, ctypes.cast(arr, ctypes.c_void_p)))
    for T in [int(v) for v in args.ts.split(",")]:
        P = T * TOP_K
        x = torch.randn((T, K), device=dev, generator=gen).to(torch.bfloat16)
        h = torch.empty((P, I), dtype=torch.bfloat16, device=dev)
        ids_host = [routing(T, c, rng) for c in range(args.calls)]
        ids_dev = [i.to(dev) for i in ids_host]
        active = sum(len(set(i.reshape(-1).tolist())) for i in ids_host) / args.calls

        def fused_with(cfg):
            cp = ctypes.byref(cfg) if cfg is not None else None
            wsz = max(L.nf4_gemm_bnb_moe_swiglu_workspace_bytes(P, dp, cp) for _, dp in descs)
            work = torch.zeros(max(wsz, 1 << 16), dtype=torch.uint8, device=dev)

            def fused():
                sp = torch.cuda.current_stream().cuda_stream
                for c in range(args.calls):
                    _, dp = descs[c % len(descs)]
                    rc = L.nf4_gemm_bnb_moe_swiglu(x.data_ptr(), ids_dev[c].data_ptr(), P, TOP_K, dp, _lib.ACT_SILU,
                                                   h.data_ptr(), _lib.BF16, work.data_ptr() if wsz else None, wsz, cp, sp)
                    assert rc == 0, rc
            return fused, work, wsz

        if args.sweep:
            for waves in (2, 4):
                for ks in range(1, 17):
                    cfg = _lib.GemmCfg(_lib.GEMM_MOE_SWIGLU, waves, 1, ks, 2)
                    fused, work, wsz = fused_with(cfg)
                    (ts,) = timed_rounds((fused,), args.calls, 3)
                    assert int(work.count_nonzero()) == 0
                    print(json.dumps({"I": I, "K": K, "T": T, "pairs": P, "waves": waves, "ksplit": ks,
                                      "us": [round(v, 3) for v in ts], "med": round(med(ts), 3)}), flush=True)
            fused, work, wsz = fused_with(None)
            (ts,) = timed_rounds((fused,), args.calls, 3)
            print(json.dumps({"I": I, "K": K, "T": T, "pairs": P, "ksplit": "library", "workspace_bytes": wsz,
                              "us": [round(v, 3) for v in ts], "med": round(med(ts), 3)}), flush=True)
            continue

        g = torch.empty((T, TOP_K, I), dtype=torch.bfloat16, device=dev)
        u = torch.empty((T, TOP_K, I), dtype=torch.bfloat16, device=dev)

        def composite():
            for c in range(args.calls):
                w1, w3 = pairs[c % len(pairs)]
                nf4_moe_linear_bnb(x, w1, ids_dev[c], out=g)
                nf4_moe_linear_bnb(x, w3, ids_dev[c], out=u)
                torch.nn.functional.silu(g) * u

        fused, work, wsz = fused_with(None)
        with torch.no_grad():
            tf, tc = timed_rounds((fused, composite), args.calls, args.rounds)
        if wsz:
            assert L.nf4_gemm_check_workspace(work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0
        assert int(work.count_nonzero()) == 0
        nblk = I * K // 64
        algo = active * 2 * (I * K // 2 + nblk + -(-nblk // 256) * 4) + T * K * 2 + P * I * 2
        print(json.dumps({"what": "w1/w3 swiglu", "I": I, "K": K, "T": T, "pairs": P, "calls": args.calls,
                          "stacks": args.stacks, "active_experts_per_call": round(active, 2),
                          "fused_us": [round(v, 3) for v in tf], "composite_us": [round(v, 3) for v in tc],
                          "fused_med": round(med(tf), 3), "composite_med": round(med(tc), 3),
                          "composite_over_fused_per_round": [round(b / a, 4) for a, b in zip(tf, tc)],
                          "composite_over_fused_med": round(med(tc) / med(tf), 4),
                          "algorithmic_bytes": int(algo), "fused_tb_per_s": round(algo / med(tf) / 1e6, 3),
                          "share_of_8tb_per_s": round(algo / med(tf) / 1e6 / (PEAK / 1e12), 4)}), flush=True)


if __name__ == "__main__":
    main()
