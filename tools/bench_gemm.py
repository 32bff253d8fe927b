"""Fused NF4 dequant-GEMM (decode shapes) vs the unfused alternatives, one MI355X.

    python tools/bench_gemm.py [--layers 32] [--ms 1,4,8,16,32]

Workload: every linear of Llama-3-8B (32 layers x {q,o 4096x4096; k,v
1024x4096; gate,up 14336x4096; down 4096x14336}), y = x @ W^T for a decode
batch of M rows.  All 224 weights are distinct buffers (3.5 GB packed), so
each pass streams them from HBM.  Per M, hipGraph replay of one full pass:

  fused      nf4_gemm_ref per weight (4-bit weight read once, dequant in registers)
  grouped    nf4_gemm_ref_grouped: q/k/v in one launch, gate/up in one (they share x), o and down alone
  composite  nf4_dequant_ref + torch.matmul per weight (the reference harness's pattern)
  bf16       torch.matmul on pre-dequantized bf16 weights (no quantization; 4x the weight bytes)

Roofline of the fused kernel: HBM bytes = N*K/2 packed + N*K/64 absmax + nested
absmax + x + y per weight, vs 8 TB/s.

``--semantics bnb``: the bitsandbytes-semantics path.  The weights come from
``nf4_quantize`` (nested statistics, blocksize 64).  Per shape of ``--shapes`` and per M, a
rotation of distinct weights larger than the Infinity Cache, and then the whole pass:

  bnb        nf4_gemm_bnb per weight, hipGraph replay
  ref        nf4_gemm_ref on the same packed bytes and statistics arrays (same traffic,
             the reference scale), replayed in turn with bnb: ``rounds`` interleaved pairs
  forward    Linear4bit.forward (nf4_linear_bnb: one fused launch), eager, wall clock
  unfused    what forward did before: dequantize_nf4_bnb (host read of the offset) + matmul,
             eager, wall clock
  (``--ms 48,64,96,128``: rows above NF4DQ_GEMM_MAX_M.  Per shape and M three graphs of >= 100
   calls each over the rotation, replayed in turn for ``rounds`` rounds and timed with device
   events: mt = nf4_gemm_bnb_mt; composite = nf4_dequant_bnb into a 16-bit temporary +
   torch.matmul, the path it replaces in nf4_linear_bnb, here without that path's host read of
   the offset; sliced = ceil(M / 32) calls of nf4_gemm_bnb on row slices.  Also the composite
   eager with the host read, wall clock, and the achieved bytes/s from the algorithmic bytes.)
  grouped    (the pass only) nf4_gemm_bnb_grouped: q/k/v in one launch, gate/up in one, o and
             down through nf4_gemm_bnb -- 128 launches -- replayed in turn with the per-weight
             bnb pass (224 launches, from ``--parent-lib`` when given: another build of the
             library loaded beside this one), with a second capture of that per-weight pass
             (the spread of a pass against itself) and with the reference-mode grouped pass
             (nf4_gemm_ref_grouped on the same bytes: a yardstick)

One JSON line per (shape, M) with medians, min - max of the rounds and the ratios.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nf4_triton_dequantization_amd import _lib  # noqa: E402

SHAPES = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096), (14336, 4096), (14336, 4096), (4096, 14336)]
PEAK = 8e12


def graph_ms(fn, reps=5):
    fn()  # eager first: library handles/workspaces (hipBLASLt) cannot be created under capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        g.replay()
        e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def _wall_us(fn, n, reps=3):
    """Median wall-clock microseconds per call of fn(i), i < n, host work and waits included."""
    import time

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6 / n)
    ts.sort()
    return ts[len(ts) // 2]


def _interleaved_rounds(fns, n, rounds=5):
    """Each of fns (n launches each) captured once, replayed in turn; per-launch microseconds
    of every round, in round order (entry r of every list belongs to the same round)."""
    graphs = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
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
            ts.append(e0.elapsed_time(e1) * 1e3 / n)
    return out


def _interleaved_us(fa, fb, n, rounds=5):
    """fa and fb (n launches each) captured once, replayed in turn; per-launch microseconds
    of every round."""
    return [sorted(t) for t in _interleaved_rounds((fa, fb), n, rounds)]


def _stats(ts):
    return {"med": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}


def main_bnb(args):
    from nf4_triton_dequantization_amd import Linear4bit, dequantize_nf4_bnb

    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def quantized(n, k):
        w = torch.randn((n, k), device=dev, generator=gen, dtype=torch.bfloat16) * 0.02
        return Linear4bit.from_float(w, compute_dtype=torch.bfloat16)

    def measure(label, mods, M):
        """mods: the weights one pass goes through, in order."""
        ks = {m.in_features for m in mods}
        xs = {k: torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16) for k in ks}
        ys = [torch.empty((M, m.out_features), dtype=torch.bfloat16, device=dev) for m in mods]
        wsz = max(max(L.nf4_gemm_bnb_workspace_bytes(M, m.out_features, m.in_features, None),
                      L.nf4_gemm_workspace_bytes(M, m.out_features, m.in_features)) for m in mods)
        work = torch.zeros(max(wsz, 1 << 16), dtype=torch.uint8, device=dev)
        t = []
        for m in mods:
            qs = m.weight.quant_state
            t.append((m.weight.data, qs.absmax, qs.state2.code, qs.state2.absmax, qs.offset))

        def bnb():
            sp = torch.cuda.current_stream().cuda_stream
            for m, y, (q, a1, c2, a2, off) in zip(mods, ys, t):
                rc = L.nf4_gemm_bnb(xs[m.in_features].data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                    c2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256, y.data_ptr(),
                                    _lib.BF16, m.out_features, m.in_features, work.data_ptr(), wsz, None, sp)
                assert rc == 0, rc

        def ref():
            sp = torch.cuda.current_stream().cuda_stream
            for m, y, (q, a1, _c2, a2, _off) in zip(mods, ys, t):
                rc = L.nf4_gemm_ref(xs[m.in_features].data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                    a2.data_ptr(), a2.numel(), y.data_ptr(), _lib.BF16, m.out_features, m.in_features,
                                    work.data_ptr(), wsz, sp)
                assert rc == 0, rc

        tb, tr = _interleaved_us(bnb, ref, len(mods), args.rounds)
        if wsz:
            assert L.nf4_gemm_check_workspace(work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0

        def forward(i):
            mods[i](xs[mods[i].in_features])

        def unfused(i):  # Linear4bit.forward before the fused path
            w = dequantize_nf4_bnb(mods[i])
            xs[mods[i].in_features].to(w.dtype) @ w.t()

        with torch.no_grad():
            forward(0), unfused(0)
            fw, un = _wall_us(forward, len(mods)), _wall_us(unfused, len(mods))
        res = {"semantics": "bnb", "what": label, "M": M, "launches": len(mods), "bnb_us": _stats(tb),
               "ref_us": _stats(tr), "bnb_over_ref": round(tb[len(tb) // 2] / tr[len(tr) // 2], 4),
               "forward_eager_us": round(fw, 3), "unfused_eager_us": round(un, 3),
               "unfused_over_forward": round(un / fw, 3), "unfused_over_bnb_graph": round(un / tb[len(tb) // 2], 3)}
        if label == "pass":
            res["bnb_pass_ms"] = round(tb[len(tb) // 2] * len(mods) / 1e3, 4)
            res["ref_pass_ms"] = round(tr[len(tr) // 2] * len(mods) / 1e3, 4)
        print(json.dumps(res), flush=True)

    def measure_grouped(mods, M):
        """The pass with q/k/v and gate/up grouped (128 launches) against the per-weight pass."""
        Lp = L
        if args.parent_lib:
            import ctypes

            Lp = ctypes.CDLL(os.path.join(REPO, "tools", "_build", f"libnf4dq_{args.parent_lib}.so"))
            for name in ("nf4_gemm_bnb", "nf4_gemm_bnb_workspace_bytes"):
                getattr(Lp, name).restype, getattr(Lp, name).argtypes = _lib.SIGNATURES[name]
        K = 4096
        x = {k: torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16) for k in {m.in_features for m in mods}}
        ys = [torch.empty((M, m.out_features), dtype=torch.bfloat16, device=dev) for m in mods]
        t = []
        for m in mods:
            qs = m.weight.quant_state
            t.append((m.weight.data, qs.absmax, qs.state2.code, qs.state2.absmax, qs.offset))
        import ctypes

        plan, keep = [], []  # (in_features, bnb mats or None, ref mats or None, count, module index)
        for b in range(0, len(mods), len(SHAPES)):
            for idx in ((0, 1, 2), (3,), (4, 5), (6,)):
                if len(idx) == 1:
                    plan.append((mods[b + idx[0]].in_features, None, None, 1, b + idx[0]))
                    continue
                bm, rm = (_lib.GemmBnbMat * len(idx))(), (_lib.GemmMat * len(idx))()
                for j, i in enumerate(idx):
                    q, a1, c2, a2, off = t[b + i]
                    n = mods[b + i].out_features
                    bm[j] = _lib.GemmBnbMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                                            a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256, ys[b + i].data_ptr(), n)
                    rm[j] = _lib.GemmMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(), a2.numel(),
                                         ys[b + i].data_ptr(), n)
                keep.append((bm, rm))
                plan.append((K, ctypes.cast(bm, ctypes.c_void_p), rm, len(idx), b + idx[0]))
        wsz = max(max(L.nf4_gemm_bnb_workspace_bytes(M, m.out_features, m.in_features, None),
                      Lp.nf4_gemm_bnb_workspace_bytes(M, m.out_features, m.in_features, None),
                      L.nf4_gemm_workspace_bytes(M, m.out_features, m.in_features)) for m in mods)
        for (k, bm, rm, c, _i) in plan:
            if c > 1:
                wsz = max(wsz, L.nf4_gemm_bnb_grouped_workspace_bytes(M, k, bm, c, 0, None),
                          L.nf4_gemm_grouped_workspace_bytes(M, k, rm, c, None))
        work = torch.zeros(max(wsz, 1 << 16), dtype=torch.uint8, device=dev)

        def one(lib, i, sp):
            m, (q, a1, c2, a2, off) = mods[i], t[i]
            rc = lib.nf4_gemm_bnb(x[m.in_features].data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                  c2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256, ys[i].data_ptr(),
                                  _lib.BF16, m.out_features, m.in_features, work.data_ptr(), wsz, None, sp)
            assert rc == 0, rc

        def per_weight():
            sp = torch.cuda.current_stream().cuda_stream
            for i in range(len(mods)):
                one(Lp, i, sp)

        def grouped():
            sp = torch.cuda.current_stream().cuda_stream
            for (k, bm, _rm, c, i) in plan:
                if c == 1:
                    one(L, i, sp)
                else:
                    rc = L.nf4_gemm_bnb_grouped(x[k].data_ptr(), M, k, bm, c, 0, _lib.BF16, work.data_ptr(), wsz, None, sp)
                    assert rc == 0, rc

        def ref_grouped():
            sp = torch.cuda.current_stream().cuda_stream
            for (k, _bm, rm, c, i) in plan:
                if c == 1:
                    m, (q, a1, _c2, a2, _off) = mods[i], t[i]
                    rc = L.nf4_gemm_ref(x[m.in_features].data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(),
                                        a1.numel(), a2.data_ptr(), a2.numel(), ys[i].data_ptr(), _lib.BF16,
                                        m.out_features, m.in_features, work.data_ptr(), wsz, sp)
                else:
                    rc = L.nf4_gemm_ref_grouped(x[k].data_ptr(), M, k, rm, c, _lib.BF16, work.data_ptr(), wsz, None, sp)
                assert rc == 0, rc

        pa, gr, pb, rg = _interleaved_rounds((per_weight, grouped, per_weight, ref_grouped), 1, args.rounds)
        assert L.nf4_gemm_check_workspace(work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        self_spread = max(abs(a / b - 1.0) for a, b in zip(pa, pb))
        gain = [a / g - 1.0 for a, g in zip(pa, gr)]
        print(json.dumps({"semantics": "bnb", "what": "grouped", "M": M, "launches": len(plan),
                          "per_weight_launches": len(mods), "per_weight_lib": args.parent_lib or "this",
                          "per_weight_pass_us": _stats(sorted(pa)), "per_weight_again_pass_us": _stats(sorted(pb)),
                          "grouped_pass_us": _stats(sorted(gr)), "ref_grouped_pass_us": _stats(sorted(rg)),
                          "per_weight_over_grouped": round(med(pa) / med(gr), 4),
                          "gain_per_round_min": round(min(gain), 4), "self_pair_spread_max": round(self_spread, 4),
                          "faster_by_more_than_the_spread": bool(min(gain) > self_spread),
                          "grouped_over_ref_grouped": round(med(gr) / med(rg), 4)}), flush=True)

    def measure_mt(label, mods, M):
        """33..128 rows: the row-tiled entry (nf4_gemm_bnb_mt) against the composite it replaces
        in nf4_linear_bnb and against ceil(M / 32) calls of nf4_gemm_bnb on row slices."""
        n, k = mods[0].out_features, mods[0].in_features
        calls = -(-max(100, len(mods)) // len(mods)) * len(mods)  # >= 100, whole turns of the rotation
        x = torch.randn((M, k), device=dev, generator=gen).to(torch.bfloat16)
        y = torch.empty((M, n), dtype=torch.bfloat16, device=dev)
        wtmp = torch.empty((n, k), dtype=torch.bfloat16, device=dev)  # the composite's 16-bit temporary
        slices = [(r, min(32, M - r)) for r in range(0, M, 32)]
        wsz = max(L.nf4_gemm_bnb_mt_workspace_bytes(M, n, k, None), L.nf4_gemm_bnb_workspace_bytes(32, n, k, None),
                  L.nf4_gemm_bnb_workspace_bytes(slices[-1][1], n, k, None))
        work = torch.zeros(max(wsz, 1 << 16), dtype=torch.uint8, device=dev)
        t = []
        for m in mods:
            qs = m.weight.quant_state
            t.append((m.weight.data, qs.absmax, qs.state2.code, qs.state2.absmax, qs.offset, float(qs.offset)))

        def mt():
            sp = torch.cuda.current_stream().cuda_stream
            for i in range(calls):
                q, a1, c2, a2, off, _ = t[i % len(t)]
                rc = L.nf4_gemm_bnb_mt(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                                       a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256, y.data_ptr(), _lib.BF16, n, k,
                                       work.data_ptr(), wsz, None, sp)
                assert rc == 0, rc

        def composite():  # nf4_linear_bnb's other path, without its host read of the offset
            import ctypes

            sp = torch.cuda.current_stream().cuda_stream
            for i in range(calls):
                q, a1, c2, a2, _, off = t[i % len(t)]
                rc = L.nf4_dequant_bnb(q.data_ptr(), a1.data_ptr(), a1.numel(), c2.data_ptr(), a2.data_ptr(), a2.numel(),
                                       ctypes.c_float(off), wtmp.data_ptr(), _lib.BF16, n * k, 64, 256, sp)
                assert rc == 0, rc
                torch.matmul(x, wtmp.t(), out=y)

        def sliced():
            sp = torch.cuda.current_stream().cuda_stream
            for i in range(calls):
                q, a1, c2, a2, off, _ = t[i % len(t)]
                for r, rows in slices:
                    rc = L.nf4_gemm_bnb(x.data_ptr() + r * k * 2, rows, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                        c2.data_ptr(), a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256,
                                        y.data_ptr() + r * n * 2, _lib.BF16, n, k, work.data_ptr(), wsz, None, sp)
                    assert rc == 0, rc

        def eager(i):  # exactly what nf4_linear_bnb ran for these M before: host read of the offset included
            w = dequantize_nf4_bnb(mods[i % len(mods)])
            x @ w.t()

        with torch.no_grad():
            tm, tc, ts = _interleaved_rounds((mt, composite, sliced), calls, args.rounds)
            eager(0)
            te = _wall_us(eager, calls)
        assert L.nf4_gemm_check_workspace(work.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream) == 0
        assert int(work.count_nonzero()) == 0
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        nblk = n * k // 64
        algo = n * k // 2 + nblk + -(-nblk // 256) * 4 + M * k * 2 + M * n * 2
        print(json.dumps({"semantics": "bnb", "what": label, "M": M, "calls": calls, "distinct_weights": len(mods),
                          "packed_mib_per_round": round(calls * n * k / 2 / 2 ** 20, 1),
                          "mt_us": [round(v, 3) for v in tm], "composite_us": [round(v, 3) for v in tc],
                          "sliced_us": [round(v, 3) for v in ts], "mt_med": round(med(tm), 3),
                          "composite_med": round(med(tc), 3), "sliced_med": round(med(ts), 3),
                          "composite_eager_wall_us": round(te, 3),
                          "composite_over_mt_min": round(min(c / m for c, m in zip(tc, tm)), 4),
                          "sliced_over_mt_min": round(min(c / m for c, m in zip(ts, tm)), 4),
                          "algorithmic_bytes": algo, "mt_tb_per_s": round(algo / med(tm) / 1e6, 3),
                          "share_of_8tb_per_s": round(algo / med(tm) / 1e6 / (PEAK / 1e12), 4)}), flush=True)

    ms = [int(v) for v in args.ms.split(",")]
    for sh in [s for s in args.shapes.split(";") if s]:
        n, k = (int(v) for v in sh.split(","))
        copies = max(8, args.budget_mb * (1 << 20) // (n * k // 2))
        mods = [quantized(n, k) for _ in range(copies)]
        for M in ms:
            if M > _lib.GEMM_MAX_M:  # 33..128 rows: the row-tiled entry and its alternatives
                measure_mt(f"{n}x{k}", mods, M)
            else:
                measure(f"{n}x{k}", mods, M)
        del mods
    ms = [M for M in ms if M <= _lib.GEMM_MAX_M]  # the whole pass: decode sizes only
    if args.layers > 0 and ms:
        mods = [quantized(n, k) for _ in range(args.layers) for (n, k) in SHAPES]
        for M in ms:
            if not args.grouped_only:
                measure("pass", mods, M)
            measure_grouped(mods, M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--semantics", choices=["ref", "bnb"], default="ref")
    ap.add_argument("--shapes", default="4096,4096;14336,4096;4096,14336", help="--semantics bnb: N,K;N,K;...")
    ap.add_argument("--budget-mb", type=int, default=768, help="--semantics bnb: packed bytes of a shape's rotation")
    ap.add_argument("--rounds", type=int, default=5, help="--semantics bnb: interleaved replay pairs")
    ap.add_argument("--parent-lib", default="", help="--semantics bnb: tools/_build/libnf4dq_<name>.so whose "
                    "nf4_gemm_bnb runs the per-weight side of the grouped row")
    ap.add_argument("--grouped-only", action="store_true", help="--semantics bnb: of the pass, only the grouped row")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ms", default="1,4,8,16,32")
    ap.add_argument("--no-bf16", action="store_true")
    ap.add_argument("--no-composite", action="store_true")
    ap.add_argument("--lib", default="prod", help="prod, or a tools/_build/libnf4dq_<name>.so variant (A/B runs)")
    args = ap.parse_args()
    if args.lib != "prod":
        _lib.LIB_PATH = os.path.join(REPO, "tools", "_build", f"libnf4dq_{args.lib}.so")
    if args.semantics == "bnb":
        return main_bnb(args)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    ws = []
    for _ in range(args.layers):
        for (n, k) in SHAPES:
            nb = n * k // 64
            ws.append((n, k, torch.randint(0, 256, (n * k // 2,), dtype=torch.uint8, device=dev, generator=gen),
                       torch.randint(0, 256, (nb,), dtype=torch.uint8, device=dev, generator=gen),
                       torch.rand((nb + 255) // 256, device=dev, generator=gen) * 0.01 + 1e-3))
    wbf = None
    if not args.no_bf16:
        wbf = []
        for (n, k, q, a1, a2) in ws:
            w = torch.empty((n, k), dtype=torch.bfloat16, device=dev)
            assert L.nf4_dequant_ref(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(), a2.numel(),
                                     w.data_ptr(), _lib.BF16, n, k, torch.cuda.current_stream().cuda_stream) == 0
            wbf.append(w)
    tmp = {(n, k): torch.empty((n, k), dtype=torch.bfloat16, device=dev) for (n, k) in set(SHAPES)}
    packed_bytes = sum(q.numel() + a1.numel() + 4 * a2.numel() for (_, _, q, a1, a2) in ws)
    for M in [int(v) for v in args.ms.split(",")]:
        xs = {k: torch.randn((M, k), device=dev).to(torch.bfloat16) for k in {k for _, k in SHAPES}}
        ys = [torch.empty((M, n), dtype=torch.bfloat16, device=dev) for (n, _, _, _, _) in ws]
        wsz = max(L.nf4_gemm_workspace_bytes(M, n, k) for (n, k) in SHAPES)
        work = torch.zeros(max(wsz, 1), dtype=torch.uint8, device=dev)  # zero before first use (counters)

        def fused():
            sp = torch.cuda.current_stream().cuda_stream
            for i, (n, k, q, a1, a2) in enumerate(ws):
                x = xs[k]
                rc = L.nf4_gemm_ref(x.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(),
                                    a2.data_ptr(), a2.numel(), ys[i].data_ptr(), _lib.BF16, n, k, work.data_ptr(),
                                    wsz, sp)
                assert rc == 0, rc

        # q,k,v (0,1,2) and gate,up (4,5) share their input: one launch each
        groups = []
        for layer in range(args.layers):
            b = layer * len(SHAPES)
            for idx in ((0, 1, 2), (3,), (4, 5), (6,)):
                mats = (_lib.GemmMat * len(idx))()
                for j, i in enumerate(idx):
                    n, k, q, a1, a2 = ws[b + i]
                    mats[j] = _lib.GemmMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(),
                                           a2.numel(), ys[b + i].data_ptr(), n)
                groups.append((ws[b + idx[0]][1], mats, len(idx)))
        gwsz = max(L.nf4_gemm_grouped_workspace_bytes(M, k, mats, c, None) for (k, mats, c) in groups)
        gwork = torch.zeros(max(gwsz, 1), dtype=torch.uint8, device=dev)

        def grouped():
            sp = torch.cuda.current_stream().cuda_stream
            for (k, mats, c) in groups:
                rc = L.nf4_gemm_ref_grouped(xs[k].data_ptr(), M, k, mats, c, _lib.BF16, gwork.data_ptr(), gwsz,
                                            None, sp)
                assert rc == 0, rc

        def composite():
            sp = torch.cuda.current_stream().cuda_stream
            for i, (n, k, q, a1, a2) in enumerate(ws):
                w = tmp[(n, k)]
                assert L.nf4_dequant_ref(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(),
                                         a2.numel(), w.data_ptr(), _lib.BF16, n, k, sp) == 0
                torch.matmul(xs[k], w.t(), out=ys[i])

        def bf16():
            for i, (n, k, *_r) in enumerate(ws):
                torch.matmul(xs[k], wbf[i].t(), out=ys[i])

        io_bytes = sum(M * k * 2 + M * n * 2 for (n, k, *_r) in ws)
        res = {"M": M, "weights": len(ws)}
        t = graph_ms(fused)
        res.update({"fused_ms": t, "fused_TBps": (packed_bytes + io_bytes) / (t * 1e-3) / 1e12,
                    "fused_frac": (packed_bytes + io_bytes) / (t * 1e-3) / PEAK})
        tg = graph_ms(grouped)
        res.update({"grouped_ms": tg, "grouped_TBps": (packed_bytes + io_bytes) / (tg * 1e-3) / 1e12,
                    "grouped_launches": len(groups)})
        res["lib"] = args.lib
        if not args.no_composite:
            res["composite_ms"] = graph_ms(composite)
            res["speedup_vs_composite"] = res["composite_ms"] / t
        if wbf is not None:
            res["bf16_weights_ms"] = graph_ms(bf16)
        if wbf is not None:
            res["speedup_vs_bf16_weights"] = res["bf16_weights_ms"] / t
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
