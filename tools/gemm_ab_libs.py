"""Two builds of the library against each other in ONE process: the fused-GEMM entries of
``--entries``, outputs compared bit for bit, then graph replay in interleaved rounds.

    python tools/gemm_ab_libs.py --a parent --b prod [--again parent2] [--ms 1,8,32] [--rounds 7]
        [--entries nf4_gemm_bnb_mt,nf4_gemm_bnb_mt_swiglu,nf4_gemm_bnb_moe]

``--a`` / ``--b`` / ``--again``: ``prod`` (the product library) or the name of a
tools/_build/libnf4dq_<name>.so.  ``--again`` is a second copy of build A under another file
name (the loader maps one file once): its rounds against A's give the spread of a build
against itself, measured in the same run.  Per shape of ``--shapes`` a rotation of distinct
weights larger than the Infinity Cache; per (entry, shape, M) the captured launches of every
build are replayed in turn, ``rounds`` times.  ``grouped``: nf4_gemm_ref_grouped over the
Llama q/k/v (4096, 1024, 1024) and gate/up (14336, 14336) groups at K = 4096.  One JSON line
per point: per-launch medians, B over A, and the largest per-round deviation of A against its
second copy.  ``nf4_gemm_bnb_mt`` and ``nf4_gemm_bnb_mt_swiglu`` (``--shapes`` are N,K and I,K)
run over ``--ms``; the expert entries ``nf4_gemm_bnb_moe``, ``nf4_gemm_bnb_moe_swiglu`` (N = I, a
gate and an up stack) and ``nf4_gemm_bnb_moe_down`` (top-2, fp32 routing weights) over ``--moe``
("experts,N,K,x_div;...") and ``--tokens`` (two choices per token, drawn once).  All with the
library's own cfg and the workspace each build asks for.  Before a point is timed every build
runs it once on the same inputs into its own output.  For the row-tiled family's entries (those
five) any bit that differs from build A's ends the run:
their sums run in MFMA order over the chunks and in slice order in the reducer in every build,
so anything but equality is a behaviour change.  For the older entries, whose builds may
legitimately order a sum differently, the line only reports ``bit_equal``.

The adapter launches ``nf4_lora_add`` and ``nf4_lora_add_routed`` are exact entries too (chunk
order in a wave, wave order in the sum).  Their points: ``--lora-shapes`` (N,K) x ``--ranks`` x
``--lora-ms``, bf16, in place on a resident base, the library's cfg, 8 rotating adapters or stacks;
the routed entry under the routings ``own`` (S = min(M, 64), every row its own adapter while they
last) and ``one`` (one adapter of a stack of 64), as tools/bench_multilora.py builds them.  Every
build starts from the same base and its 8 launches accumulate in place before the comparison.
The timed replays then go on accumulating into the same outputs: those values mean nothing and
may overflow, which is harmless here because these kernels' time does not depend on the data.
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
from tools.bench_multilora import make_routing  # noqa: E402

ENTRIES = ("nf4_gemm_ref", "nf4_gemm_ref_grouped", "nf4_gemm_bnb", "nf4_gemm_workspace_bytes",
           "nf4_gemm_grouped_workspace_bytes", "nf4_gemm_bnb_workspace_bytes", "nf4_gemm_check_workspace",
           "nf4_gemm_bnb_mt", "nf4_gemm_bnb_mt_workspace_bytes", "nf4_gemm_bnb_mt_swiglu",
           "nf4_gemm_bnb_mt_swiglu_workspace_bytes", "nf4_gemm_bnb_moe", "nf4_gemm_bnb_moe_workspace_bytes",
           "nf4_gemm_bnb_moe_swiglu", "nf4_gemm_bnb_moe_swiglu_workspace_bytes", "nf4_gemm_bnb_moe_down",
           "nf4_gemm_bnb_moe_down_workspace_bytes", "nf4_lora_add", "nf4_lora_add_routed")


def load(name):
    path = _lib.LIB_PATH if name == "prod" else os.path.join(REPO, "tools", "_build", f"libnf4dq_{name}.so")
    h = ctypes.CDLL(path)
    for e in ENTRIES:
        if not hasattr(h, e):  # a build from before the entry: fine while --entries does not ask for it
            continue
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
    ap.add_argument("--entries", default="nf4_gemm_ref,nf4_gemm_bnb,nf4_gemm_ref_grouped")
    ap.add_argument("--moe", default="8,14336,4096,2;8,4096,14336,1")
    ap.add_argument("--tokens", default="1,16,64")
    ap.add_argument("--lora-shapes", default="4096,4096;14336,4096")
    ap.add_argument("--ranks", default="16,64,128", help="128 is the only way to the 8-r-tile kernels")
    ap.add_argument("--lora-ms", default="1,16,32,128", help="both row-block heights")
    args = ap.parse_args()
    entries = [e for e in args.entries.split(",") if e]
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

    EXACT = ("nf4_gemm_bnb_mt", "nf4_gemm_bnb_mt_swiglu", "nf4_gemm_bnb_moe", "nf4_gemm_bnb_moe_swiglu", "nf4_gemm_bnb_moe_down",
             "nf4_lora_add", "nf4_lora_add_routed")

    def report(entry, what, M, n, ts, bit_equal):
        med = [sorted(t)[len(t) // 2] for t in ts]
        res = {"entry": entry, "what": what, "M": M, "launches": n, "a": names[0], "b": names[1],
               "a_us": round(med[0], 3), "b_us": round(med[1], 3), "b_over_a": round(med[1] / med[0], 4), "bit_equal": bit_equal,
               "b_over_a_by_round": [round(b / a, 4) for a, b in zip(ts[0], ts[1])]}
        if len(ts) > 2:
            res["a_again_over_a_by_round"] = [round(c / a, 4) for a, c in zip(ts[0], ts[2])]
            res["self_spread_max"] = round(max(abs(c / a - 1.0) for a, c in zip(ts[0], ts[2])), 4)
        print(json.dumps(res), flush=True)

    def check(work, wsz):
        for L in libs if wsz else ():  # a buffer no split-K ever ran on has nothing to report
            assert L.nf4_gemm_check_workspace(work.data_ptr(), work.numel(), torch.cuda.current_stream().cuda_stream) == 0

    def point(entry, what, M, n, work, wsz, runs, outs, start=None):
        """runs[i]: build i's n launches (the first into outs[i]).  Bit-equal outputs, then the rounds.
        start: what an in-place entry's outputs begin as."""
        same = True
        for i, (run, out) in enumerate(zip(runs, outs)):
            if start is None:
                out.view(torch.int16).fill_(0x7FFF)  # NaN bits: a row nobody stores is seen
            else:
                out.copy_(start)
            run()
            torch.cuda.synchronize()
            eq = torch.equal(out.view(torch.int16), outs[0].view(torch.int16))
            assert eq or entry not in EXACT, \
                f"{entry} {what} M={M}: build {names[i]} differs from {names[0]} in " \
                f"{int((out.view(torch.int16) != outs[0].view(torch.int16)).sum())} elements"
            same = same and eq
        report(entry, what, M, n, _interleaved_rounds(runs, n, args.rounds), same)
        check(work, wsz)

    def bf16_out(M, n):
        return [torch.empty((M, n), dtype=torch.bfloat16, device=dev) for _ in libs]

    ms = [int(v) for v in args.ms.split(",")]
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";") if s]
    if "nf4_gemm_bnb_mt" in entries:
        for n, k in shapes:
            copies = max(8, args.budget_mb * (1 << 20) // (n * k // 2))
            ws = [weight(n, k) for _ in range(copies)]
            for M in ms:
                x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
                ys = bf16_out(M, n)
                wsz = max(L.nf4_gemm_bnb_mt_workspace_bytes(M, n, k, None) for L in libs)
                work = torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev)

                def mt(L, y):
                    def run():
                        sp = torch.cuda.current_stream().cuda_stream
                        for (q, a1, a2) in ws:
                            rc = L.nf4_gemm_bnb_mt(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                                   code2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256,
                                                   y.data_ptr(), _lib.BF16, n, k, work.data_ptr(), work.numel(), None, sp)
                            assert rc == 0, rc
                    return run

                point("nf4_gemm_bnb_mt", f"{n}x{k}", M, copies, work, wsz, [mt(L, y) for L, y in zip(libs, ys)], ys)
            del ws
    if "nf4_gemm_bnb_mt_swiglu" in entries:
        code2u = torch.linspace(0.75, -0.75, 256, device=dev)
        offu = torch.full((1,), -0.02, device=dev)
        for n, k in shapes:
            copies = max(8, args.budget_mb * (1 << 20) // (n * k))
            ws = [(weight(n, k), weight(n, k)) for _ in range(copies)]
            pairs = []
            for g, u in ws:
                mats = (_lib.GemmBnbMat * 2)()
                for j, ((q, a1, a2), c2, o) in enumerate(((g, code2, off), (u, code2u, offu))):
                    mats[j] = _lib.GemmBnbMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(), a2.data_ptr(),
                                              a2.numel(), o.data_ptr(), 64, 256, None, n)
                pairs.append(mats)
            for M in ms:
                x = (torch.randn((M, k), device=dev, generator=gen) * 0.05).to(torch.bfloat16)
                hs = bf16_out(M, n)
                wsz = max(L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(M, n, k, None) for L in libs)
                work = torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev)

                def sg(L, h):
                    def run():
                        sp = torch.cuda.current_stream().cuda_stream
                        for mats in pairs:
                            rc = L.nf4_gemm_bnb_mt_swiglu(x.data_ptr(), M, k, ctypes.cast(mats, ctypes.c_void_p), 0, _lib.ACT_SILU,
                                                          h.data_ptr(), _lib.BF16, work.data_ptr(), work.numel(), None, sp)
                            assert rc == 0, rc
                    return run

                point("nf4_gemm_bnb_mt_swiglu", f"{n}x{k}", M, copies, work, wsz, [sg(L, h) for L, h in zip(libs, hs)], hs)
            del ws, pairs
    lora_entries = [e for e in ("nf4_lora_add", "nf4_lora_add_routed") if e in entries]
    lora_shapes = [tuple(int(v) for v in t.split(",")) for t in args.lora_shapes.split(";") if t]
    for n, k, r in [(n, k, int(r)) for n, k in lora_shapes for r in args.ranks.split(",")] if lora_entries else ():
        # 8 stacks of 64 adapters; a routing over S < 64 takes a stack's first S, the dense entry its adapter 37
        stacks = [((torch.randn((64, r, k), device=dev, generator=gen) / k ** 0.5).to(torch.bfloat16),
                   (torch.randn((64, n, r), device=dev, generator=gen) / r ** 0.5).to(torch.bfloat16),
                   0.5 + torch.rand((64,), device=dev, generator=gen)) for _ in range(8)]
        for M in [int(v) for v in args.lora_ms.split(",")]:
            x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
            base = torch.randn((M, n), device=dev, generator=gen).to(torch.bfloat16)
            ys = bf16_out(M, n)
            what = f"{n}x{k} r={r}"

            def dense(L, y):
                mats = [(_lib.LoraMat * 1)(_lib.LoraMat(A[37].data_ptr(), B[37].data_ptr(), y.data_ptr(), y.data_ptr(), n, r, 1.25))
                        for A, B, _ in stacks]

                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for d in mats:
                        rc = L.nf4_lora_add(x.data_ptr(), M, k, ctypes.cast(d, ctypes.c_void_p), 1, _lib.BF16, None, sp)
                        assert rc == 0, rc
                return run

            def routed(L, y, S, ids):
                descs = [(_lib.LoraStack * 1)(_lib.LoraStack(A.data_ptr(), B.data_ptr(), sc.data_ptr(), y.data_ptr(), y.data_ptr(), n,
                                                             r * k, n * r, r)) for A, B, sc in stacks]

                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for d in descs:
                        rc = L.nf4_lora_add_routed(x.data_ptr(), ids.data_ptr(), M, k, S, ctypes.cast(d, ctypes.c_void_p), 1, _lib.BF16,
                                                   None, sp)
                        assert rc == 0, rc
                return run

            if "nf4_lora_add" in entries:
                point("nf4_lora_add", what, M, 8, None, 0, [dense(L, y) for L, y in zip(libs, ys)], ys, start=base)
            for routing in ("own", "one") if "nf4_lora_add_routed" in entries else ():
                S, ids = make_routing(routing, M, dev, gen)
                point("nf4_lora_add_routed", f"{what} {routing} S={S}", M, 8, None, 0,
                      [routed(L, y, S, ids) for L, y in zip(libs, ys)], ys, start=base)
        del stacks
    moe_entries = [e for e in ("nf4_gemm_bnb_moe", "nf4_gemm_bnb_moe_swiglu", "nf4_gemm_bnb_moe_down") if e in entries]
    for E, n, k, x_div in [tuple(int(v) for v in s.split(",")) for s in args.moe.split(";") if s] if moe_entries else ():
        copies = max(8, args.budget_mb * (1 << 20) // (E * n * k // 2))
        nb, n2 = n * k // 64, (n * k // 64 + 255) // 256

        def stack(c2, lo):
            q = torch.randint(0, 256, (E, n * k // 2), dtype=torch.uint8, device=dev, generator=gen)
            a1 = torch.randint(0, 256, (E, nb), dtype=torch.uint8, device=dev, generator=gen)
            a2 = torch.rand((E, n2), device=dev, generator=gen) * 0.01 + 1e-3
            offs = torch.linspace(lo, 2 * lo, E, device=dev)
            d = _lib.MoeExperts(q.data_ptr(), n * k // 2, a1.data_ptr(), nb, c2.data_ptr(), 0, a2.data_ptr(), n2,
                                offs.data_ptr(), n, k, E, 0, 64, 256)
            return d, (q, a1, a2, offs)

        stacks = [stack(code2, 0.01) for _ in range(copies)]
        what = f"{E}x{n}x{k} x_div={x_div}"
        gate_up = []
        if "nf4_gemm_bnb_moe_swiglu" in entries:  # the stacks above are the gates; an up stack each
            code2u = torch.linspace(0.75, -0.75, 256, device=dev)
            ups = [stack(code2u, -0.02) for _ in range(copies)]
            gate_up = [(_lib.MoeExperts * 2)(g[0], u[0]) for g, u in zip(stacks, ups)]
        for tokens in [int(v) for v in args.tokens.split(",")]:
            P = 2 * tokens  # two choices per token: w1 (x_div 2) reads the token's row twice, w2 a row per pair
            ids = torch.randint(0, E, (P,), dtype=torch.int32, device=dev, generator=gen)
            x = (torch.randn((-(-P // x_div), k), device=dev, generator=gen) * 0.05).to(torch.bfloat16)
            first = ctypes.cast(ctypes.pointer(stacks[0][0]), ctypes.c_void_p)

            def workspace(bytes_entry, desc):
                wsz = max(getattr(L, bytes_entry)(P, desc, None) for L in libs)
                return torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev), wsz

            if "nf4_gemm_bnb_moe" in entries:
                ys = bf16_out(P, n)
                work, wsz = workspace("nf4_gemm_bnb_moe_workspace_bytes", first)

                def moe(L, y):
                    def run():
                        sp = torch.cuda.current_stream().cuda_stream
                        for d, _ in stacks:
                            rc = L.nf4_gemm_bnb_moe(x.data_ptr(), ids.data_ptr(), P, x_div, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p),
                                                    y.data_ptr(), _lib.BF16, work.data_ptr(), work.numel(), None, sp)
                            assert rc == 0, rc
                    return run

                point("nf4_gemm_bnb_moe", what, P, copies, work, wsz, [moe(L, y) for L, y in zip(libs, ys)], ys)
            if "nf4_gemm_bnb_moe_swiglu" in entries:
                hs = bf16_out(P, n)
                work, wsz = workspace("nf4_gemm_bnb_moe_swiglu_workspace_bytes", ctypes.cast(gate_up[0], ctypes.c_void_p))

                def msg(L, h):
                    def run():
                        sp = torch.cuda.current_stream().cuda_stream
                        for gu in gate_up:
                            rc = L.nf4_gemm_bnb_moe_swiglu(x.data_ptr(), ids.data_ptr(), P, x_div, ctypes.cast(gu, ctypes.c_void_p),
                                                           _lib.ACT_SILU, h.data_ptr(), _lib.BF16, work.data_ptr(), work.numel(), None, sp)
                            assert rc == 0, rc
                    return run

                point("nf4_gemm_bnb_moe_swiglu", what, P, copies, work, wsz, [msg(L, h) for L, h in zip(libs, hs)], hs)
            if "nf4_gemm_bnb_moe_down" in entries:
                rw = torch.rand(P, device=dev, generator=gen) * 0.96 + 0.02
                ys = bf16_out(tokens, n)
                work, wsz = workspace("nf4_gemm_bnb_moe_down_workspace_bytes", first)

                def down(L, y):
                    def run():
                        sp = torch.cuda.current_stream().cuda_stream
                        for d, _ in stacks:
                            rc = L.nf4_gemm_bnb_moe_down(x.data_ptr(), ids.data_ptr(), P, x_div, 2, rw.data_ptr(), _lib.F32,
                                                         ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), y.data_ptr(), _lib.BF16,
                                                         work.data_ptr(), work.numel(), None, sp)
                            assert rc == 0, rc
                    return run

                point("nf4_gemm_bnb_moe_down", what, P, copies, work, wsz, [down(L, y) for L, y in zip(libs, ys)], ys)
        del stacks, gate_up
    for n, k in shapes if ("nf4_gemm_ref" in entries or "nf4_gemm_bnb" in entries) else ():
        copies = max(8, args.budget_mb * (1 << 20) // (n * k // 2))
        ws = [weight(n, k) for _ in range(copies)]
        for M in ms:
            x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
            ys = bf16_out(M, n)
            wsz = max(max(L.nf4_gemm_workspace_bytes(M, n, k), L.nf4_gemm_bnb_workspace_bytes(M, n, k, None)) for L in libs)
            work = torch.zeros(max(wsz, 1 << 17), dtype=torch.uint8, device=dev)

            def ref(L, y):
                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for (q, a1, a2) in ws:
                        rc = L.nf4_gemm_ref(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                            a2.data_ptr(), a2.numel(), y.data_ptr(), _lib.BF16, n, k, work.data_ptr(),
                                            work.numel(), sp)
                        assert rc == 0, rc
                return run

            def bnb(L, y):
                def run():
                    sp = torch.cuda.current_stream().cuda_stream
                    for (q, a1, a2) in ws:
                        rc = L.nf4_gemm_bnb(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                            code2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256,
                                            y.data_ptr(), _lib.BF16, n, k, work.data_ptr(), work.numel(), None, sp)
                        assert rc == 0, rc
                return run

            if "nf4_gemm_ref" in entries:
                point("nf4_gemm_ref", f"{n}x{k}", M, copies, work, wsz, [ref(L, y) for L, y in zip(libs, ys)], ys)
            if "nf4_gemm_bnb" in entries:
                point("nf4_gemm_bnb", f"{n}x{k}", M, copies, work, wsz, [bnb(L, y) for L, y in zip(libs, ys)], ys)
        del ws
    k = 4096
    for label, ns in (("qkv", (4096, 1024, 1024)), ("gate_up", (14336, 14336))) if "nf4_gemm_ref_grouped" in entries else ():
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
                   _interleaved_rounds([grouped(L) for L in libs], copies, args.rounds), None)  # shared outputs: not compared
            check(work, wsz)


if __name__ == "__main__":
    main()
