"""Times the NF4 embedding gather (csrc/nf4_embed.hip) on one MI355X.

    python tools/bench_embed.py [--rounds 7] [--out profiles/embedding/bench_embed.jsonl]

Weight: rows = 128256, dim = 4096 (a Llama-3-8B table), bf16, nested statistics, built by
``Embedding4bit.from_float`` from a seeded weight.  Ids: seeded uniform, a different set for
every launch of a graph.  Counts 1, 8, 32, 512 and 8192.

Method: graph replay.  Each contender is captured once as a graph of ``inner`` calls (distinct
ids and outputs per call) and the graphs are replayed in turn in one process for ``rounds``
rounds; a round's figure is the time between two device events around ``replays`` replays,
per call; the medians over the rounds are reported.

  a   ``Embedding4bit(ids)``: the new call (0.5 B in + 2 B out per element)
  b   ``torch.nn.functional.embedding`` on a bf16 copy of the same table -- the layer it
      replaces (2 B in + 2 B out) -- the copy being ``dequantize_nf4_bnb`` of the NF4 table, so
      that (a) and (b) must return the same bits: a mismatch fails the run
  c   ``dequantize_nf4_bnb(module)[ids]`` at count 32 only (its cost does not depend on the
      count); it reads the offset on the host, which a capture refuses, so it is timed eagerly
  b2  (b) a second time: |b - b2| is the spread the comparisons are judged against

and (a) on one dim % 64 != 0 table (the general form): reported, not judged.

Acceptance (line "accept"): at count 8192, a <= b + spread; at counts <= 32 (launch-bound for
both), a - b <= spread, else the difference is reported (the kernel's prologue -- the
staging of the nested code and the workgroup barrier ahead of the first gather -- is the
place to look).
``frac_of_copy_rate``: algorithmic bytes over time, as a share of the 6.29 TB/s float4-copy
rate measured on this part (not of the 8 TB/s specification).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nf4_triton_dequantization_amd import Embedding4bit, dequantize_nf4_bnb  # noqa: E402

ROWS, DIM = 128256, 4096
COUNTS = (1, 8, 32, 512, 8192)
GENERAL = (32000, 4100, 512)  # rows, dim (dim % 64 == 4), count
COPY_RATE = 6.29e12


def seeded_weight(rows, dim, dev, seed):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    w = torch.empty(rows, dim, dtype=torch.bfloat16, device=dev)
    step = 8192
    for r in range(0, rows, step):  # in pieces: no fp32 temporary of the whole table
        n = min(step, rows - r)
        w[r:r + n] = (torch.randn(n, dim, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
    return w


def event_time(fn, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / replays


def capture(call, inner):
    """A graph of `inner` calls of call(i); returns (graph, outputs)."""
    outs = []
    call(0)  # warm: code objects loaded, allocations made outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(inner):
            outs.append(call(i))
    g.replay()
    torch.cuda.synchronize()
    return g, outs


def alg_bytes(count, dim, ids_bytes=8):
    el = count * dim
    return el // 2 + el // 64 + 4 * (el // 64 // 256 + 1) + 2 * el + count * ids_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_embed.py needs a ROCm device"
    dev = torch.device("cuda", 0)
    fh = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fh = open(args.out, "a")

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    torch.set_grad_enabled(False)
    emb = Embedding4bit.from_float(seeded_weight(ROWS, DIM, dev, 1))
    table = dequantize_nf4_bnb(emb)  # the bf16 copy of the same table
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    accept = {}
    for count in COUNTS:
        inner = 4 if count >= 8192 else 16
        replays = 10 if count >= 8192 else 50
        ids = [torch.randint(0, ROWS, (count,), device=dev, generator=gen) for _ in range(inner)]
        ga, oa = capture(lambda i: emb(ids[i]), inner)
        gb, ob = capture(lambda i: torch.nn.functional.embedding(ids[i], table), inner)
        for x, y in zip(oa, ob):
            if not torch.equal(x, y):
                raise AssertionError(f"count {count}: the NF4 gather and the bf16 table's rows differ")
        series = {"a": [], "b": [], "b2": []}
        if count == 32:
            series["c"] = []
            for _ in range(2):
                dequantize_nf4_bnb(emb)[ids[0]]
            torch.cuda.synchronize()
        for _ in range(args.rounds):
            series["a"].append(event_time(ga.replay, replays) / inner)
            series["b"].append(event_time(gb.replay, replays) / inner)
            if "c" in series:
                series["c"].append(event_time(lambda: dequantize_nf4_bnb(emb)[ids[0]], 2))
            series["b2"].append(event_time(gb.replay, replays) / inner)
        med = {k: statistics.median(v) for k, v in series.items()}
        spread = max(abs(med["b"] - med["b2"]),
                     statistics.median(abs(x - y) for x, y in zip(series["b"], series["b2"])))
        byt = alg_bytes(count, DIM)
        line = {"line": "embed", "rows": ROWS, "dim": DIM, "count": count, "dtype": "bf16", "form": "aligned",
                "inner": inner, "replays": replays, "rounds": args.rounds, "a_us": med["a"] * 1e6,
                "b_us": med["b"] * 1e6, "b2_us": med["b2"] * 1e6, "spread_us": spread * 1e6,
                "a_min_us": min(series["a"]) * 1e6, "a_max_us": max(series["a"]) * 1e6,
                "algorithmic_bytes": byt, "a_TBps": byt / med["a"] / 1e12,
                "a_frac_of_copy_rate": byt / med["a"] / COPY_RATE,
                "b_frac_of_copy_rate": (4 * count * DIM + 8 * count) / med["b"] / COPY_RATE,
                "verified": True, "timing": "graph replay, events, median of rounds"}
        if "c" in med:
            line["c_us"] = med["c"] * 1e6
            line["c_timing"] = "eager (the host read of the offset cannot be captured)"
        emit(line)
        if count >= 8192:
            accept[count] = {"rule": "a <= b + spread", "holds": med["a"] <= med["b"] + spread,
                             "a_minus_b_us": (med["a"] - med["b"]) * 1e6, "spread_us": spread * 1e6}
        elif count <= 32:  # (a faster than b is no miss: only the slower side is judged)
            accept[count] = {"rule": "a - b <= spread", "holds": med["a"] - med["b"] <= spread,
                             "a_minus_b_us": (med["a"] - med["b"]) * 1e6, "spread_us": spread * 1e6}
        del ga, gb, oa, ob, ids
        torch.cuda.empty_cache()
    emit({"line": "accept", "by_count": accept,
          "note": "where a count <= 32 does not hold, the difference is a_minus_b_us; look at the prologue"})

    # the general form (dim % 64 != 0): reported, not judged
    del table, emb
    torch.cuda.empty_cache()
    rows, dim, count = GENERAL
    emb = Embedding4bit.from_float(seeded_weight(rows, dim, dev, 3))
    table = dequantize_nf4_bnb(emb)
    inner, replays = 8, 20
    ids = [torch.randint(0, rows, (count,), device=dev, generator=gen) for _ in range(inner)]
    ga, oa = capture(lambda i: emb(ids[i]), inner)
    for i, x in enumerate(oa):
        if not torch.equal(x, table[ids[i]]):
            raise AssertionError("general form: the NF4 gather and the bf16 table's rows differ")
    ts = [event_time(ga.replay, replays) / inner for _ in range(args.rounds)]
    t = statistics.median(ts)
    byt = alg_bytes(count, dim)
    emit({"line": "embed_general", "rows": rows, "dim": dim, "count": count, "dtype": "bf16", "form": "general",
          "a_us": t * 1e6, "algorithmic_bytes": byt, "a_frac_of_copy_rate": byt / t / COPY_RATE, "verified": True,
          "judged": False})


if __name__ == "__main__":
    main()
