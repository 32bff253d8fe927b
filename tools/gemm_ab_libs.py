"""Two builds of the library against each other in ONE process: the existing fused-GEMM
entries (nf4_gemm_ref, nf4_gemm_ref_grouped, nf4_gemm_bnb), graph replay, interleaved rounds.

    python tools/gemm_ab_libs.py --a parent --b prod [--again parent2] [--ms 1,8,32] [--rounds 7]

``--a`` / ``--b`` / ``--again``: ``prod`` (the product library) or the name of a
tools/_build/libnf4dq_<name>.so.  ``--again`` is a second copy of build A under another file
name (the loader maps one file once): its rounds against A's give the spread of a build
against itself, measured in the same run.  Per shape of ``--shapes`` a rotation of distinct
weights larger than the Infinity Cache; per (entry, shape, M) the captured launches of every
build are replayed in turn, ``rounds`` times.  ``grouped``: nf4_gemm_ref_grouped over the
Llama q/k/v (4096, 1024, 1024) and gate/up (14336, 14336) groups at K = 4096.  One JSON line
per point: per-launch medians, B over A, and the largest per-round deviation of A against its
second copy.
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
from nf4_triton_dequantization_amd import _lib  # noqa: E402
from tools.bench_gemm import _interleaved_rounds  # noqa: E402

ENTRIES = ("nf4_gemm_ref", "nf4_gemm_ref_grouped", "nf4_gemm_bnb", "nf4_gemm_workspace_bytes",
           "nf4_gemm_grouped_workspace_bytes", "nf4_gemm_bnb_workspace_bytes", "nf4_gemm_check_workspace")


def load(name):
    path = _lib.LIB_PATH if name == "prod" else os.path.join(REPO, "tools", "_build", f"libnf4dq_{name}.so")
    h = ctypes.CDLL(path)
    for e in ENTRIES:
        getattr(h, e).restype, getattr(h, e).argtypes = _lib.SIGNATURES[e]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", default="parent")
    ap.add_argument("--b", default="prod")
    ap.add_argument("--again", default="")
    ap.add_argument("--ms", default="1,8,32")
    ap.add_argument("--shapes", default="4096,4096;14336,4096;4096,14336")
    ap.add_argument("--budget-mb", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    names = [args.a, args.b] + ([args.again] if args.again else [])
    libs = [load(n) for n in names]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def weight(n, k):
        nb = n * k // 64
        return (torch.randint(0, 256, (n * k // 2,), dtype=torch.uint8, device=dev, generator=gen),
                torch.randint(0, 256, (nb,), dtype=torch.uint8, device=dev, generator=gen),
                torch.rand((nb + 255) // 256, device=dev, generator=gen) * 0.01 + 1e-3)

    code2 = torch.linspace(-1.0, 1.0, 256, device=dev)
    off = torch.full((1,), 0.01, device=dev)

    def report(entry, what, M, n, ts):
        med = [sorted(t)[len(t) // 2] for t in ts]
        res = {"entry": entry, "what": what, "M": M, "launches": n, "a": names[0], "b": names[1],
               "a_us": round(med[0], 3), "b_us": round(med[1], 3), "b_over_a": round(med[1] / med[0], 4),
               "b_over_a_by_round": [round(b / a, 4) for a, b in zip(ts[0], ts[1])]}
        if len(ts) > 2:
            res["a_again_over_a_by_round"] = [round(c / a, 4) for a, c in zip(ts[0], ts[2])]
            res["self_spread_max"] = round(max(abs(c / a - 1.0) for a, c in zip(ts[0], ts[2])), 4)
        print(json.dumps(res), flush=True)

    def check(work, wsz):
        for L in libs if wsz else ():  # a buffer no split-K ever ran on has nothing to report
            assert L.nf4_gemm_check_workspace(work.data_ptr(), work.numel(), torch.cuda.current_stream().cuda_stream) == 0

    ms = [int(v) for v in args.ms.split(",")]
    for sh in [s for s in args.shapes.split(";") if s]:
        n, k = (int(v) for v in sh.split(","))
        copies = max(8, args.budget_mb * (1 << 20) // (n * k // 2))
        ws = [weight(n, k) for _ in range(copies)]
        for M in ms:
            x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
            y = torch.empty((M, n), dtype=torch.bfloat16, device=dev)
            wsz = max(max(L.nf4_gemm_workspace_bytes(M, n, k), L.nf4_gemm_bnb_workspace_bytes(M, n, k, None)) for L in libs)
            work = torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev)

            def ref(L):
                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for (q, a1, a2) in ws:
                        rc = L.nf4_gemm_ref(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                            a2.data_ptr(), a2.numel(), y.data_ptr(), _lib.BF16, n, k, work.data_ptr(),
                                            work.numel(), sp)
                        assert rc == 0, rc
                return run

            def bnb(L):
                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for (q, a1, a2) in ws:
                        rc = L.nf4_gemm_bnb(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                            code2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256,
                                            y.data_ptr(), _lib.BF16, n, k, work.data_ptr(), work.numel(), None, sp)
                        assert rc == 0, rc
                return run

            report("nf4_gemm_ref", f"{n}x{k}", M, copies, _interleaved_rounds([ref(L) for L in libs], copies, args.rounds))
            report("nf4_gemm_bnb", f"{n}x{k}", M, copies, _interleaved_rounds([bnb(L) for L in libs], copies, args.rounds))
            check(work, wsz)
        del ws
    k = 4096
    for label, ns in (("qkv", (4096, 1024, 1024)), ("gate_up", (14336, 14336))):
        copies = max(8, args.budget_mb * (1 << 20) // (sum(ns) * k // 2))
        groups, keep = [], []
        ys = None
        for M in ms:
            x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
            ys = [torch.empty((M, n), dtype=torch.bfloat16, device=dev) for n in ns]
            if not keep:
                keep = [[weight(n, k) for n in ns] for _ in range(copies)]
            groups = []
            for g in keep:
                mats = (_lib.GemmMat * len(ns))()
                for j, ((q, a1, a2), n) in enumerate(zip(g, ns)):
                    mats[j] = _lib.GemmMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(), a2.numel(),
                                           ys[j].data_ptr(), n)
                groups.append(mats)
            wsz = max(L.nf4_gemm_grouped_workspace_bytes(M, k, groups[0], len(ns), None) for L in libs)
            work = torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev)

            def grouped(L):
                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for mats in groups:
                        rc = L.nf4_gemm_ref_grouped(x.data_ptr(), M, k, mats, len(ns), _lib.BF16, work.data_ptr(),
                                                    work.numel(), None, sp)
                        assert rc == 0, rc
                return run

            report("nf4_gemm_ref_grouped", label, M, copies,
                   _interleaved_rounds([grouped(L) for L in libs], copies, args.rounds))
            check(work, wsz)


if __name__ == "__main__":
    main()
