"""Times the HIP NF4 quantizer (csrc/nf4_quant.hip) on the MI355X.

    python tools/bench_quant.py [--reps 5] [--steps 64] [--out profiles/quant/bench_quant.jsonl]

Method: tools/bench_configs.py's c4.  Every launch reads a different weight of a rotation of
>= 512 MiB of distinct inputs (HBM-streamed, not cache-resident) and writes a rotating output
set; every set is touched once first; `steps` launches are timed between HIP events behind a
device spin that covers the host's submission (``us_per_call``), and the hipGraph replay of
the same launches is reported beside it (``graph_us_per_call``).  After the timing, outputs
the timed launches wrote are compared with the Python quantizer (bnb_layout.quantize_nf4 /
quantize_blockwise_8bit on host copies of the same inputs): a mismatch fails the run.

Lines (JSON, one each):
  quant      4096x4096 and 14336x4096; bf16 / fp16 / fp32 input; single level and nested.
             algorithmic bytes = input + numel/2 + statistics; TB/s; share of 8 TB/s.
  vs_dequant the flat dequant (nf4_dequant_ref) of the same matrix, timed alternately with
             the quantizer in the same process: the same bytes in the other direction.
  vs_torch   bnb_layout.quantize_nf4 on the device (what the HIP path replaces), timed
             alternately with nf4_quantize through the same Python entry.  The run fails
             unless the HIP single-level call is >= 5x faster at 4096x4096 bf16.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nf4_triton_dequantization_amd import _lib, nf4_quantize  # noqa: E402
from nf4_triton_dequantization_amd.bnb_layout import dynamic_map, quantize_blockwise_8bit, quantize_nf4  # noqa: E402
from bench_configs import MIN_READ_FOOTPRINT, PEAK, eager_per_launch, last_writes, timed  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096)]
DTYPES = [("bf16", torch.bfloat16, _lib.BF16), ("fp16", torch.float16, _lib.F16), ("fp32", torch.float32, _lib.F32)]
MIN_SPEEDUP = 5.0


def make_inputs(m, n, dt, dev, count, gen):
    """`count` weights: normals, each 64-block scaled by 2^-8 .. 2^4."""
    ws = []
    for _ in range(count):
        e = torch.randint(-8, 5, (m * n // 64, 1), device=dev, generator=gen).float()
        w = torch.randn(m * n // 64, 64, device=dev, generator=gen) * torch.exp2(e)
        ws.append(w.to(dt).view(m, n))
    return ws


def alg_bytes(numel, esz, nested):
    nblk = numel // 64
    stats = nblk + 4 * ((nblk + 255) // 256) + 4 if nested else 4 * nblk
    return numel * esz + numel // 2 + stats


_EXPECT = {}


def expected(key, w):
    """(packed, fp32 absmax) of the Python quantizer on a host copy; one evaluation per input set."""
    if key not in _EXPECT:
        p, qs = quantize_nf4(w.cpu(), compress_statistics=False)
        _EXPECT[key] = (p.reshape(-1), qs.absmax)
    return _EXPECT[key]


def verify(key, w, out, nested):
    wp, wa = expected(key, w)
    if not torch.equal(out["packed"].cpu(), wp):
        raise AssertionError(f"{key}: packed differs from the Python quantizer")
    if not nested:
        if not torch.equal(out["absmax"].cpu().view(torch.int32), wa.view(torch.int32)):
            raise AssertionError(f"{key}: absmax differs from the Python quantizer")
        return
    o = np.float32(out["offset"].item())
    mean = np.float32(wa.double().mean().item())
    if o.tobytes() not in {mean.tobytes(), np.nextafter(mean, np.float32(np.inf)).tobytes(),
                           np.nextafter(mean, np.float32(-np.inf)).tobytes()}:
        raise AssertionError(f"{key}: offset {o} is not the fp64 mean {mean} or an fp32 neighbour")
    aq, a2 = quantize_blockwise_8bit(wa - torch.tensor(o), dynamic_map(), 256)
    if not (torch.equal(out["absmax_q"].cpu(), aq) and torch.equal(out["absmax2"].cpu().view(torch.int32),
                                                                   a2.view(torch.int32))):
        raise AssertionError(f"{key}: nested statistics differ from the Python quantizer")


def run_shape(m, n, name, dt, code, dev, reps, steps, emit):
    gen = torch.Generator(device=dev)
    gen.manual_seed(m + n)
    numel, esz = m * n, torch.empty((), dtype=dt).element_size()
    nblk = numel // 64
    pin = max(1, -(-MIN_READ_FOOTPRINT // (numel * esz)))
    pout = steps  # every timed launch keeps its own output: >= 512 MiB of distinct writes at these shapes
    ins = make_inputs(m, n, dt, dev, pin, gen)
    L = _lib.lib()
    code2 = dynamic_map().to(dev)
    wsz = L.nf4_quant_workspace_bytes(numel, 64)
    outs = [{"packed": torch.empty(numel // 2, dtype=torch.uint8, device=dev),
             "absmax": torch.empty(nblk, dtype=torch.float32, device=dev),
             "absmax_q": torch.empty(nblk, dtype=torch.uint8, device=dev),
             "absmax2": torch.empty((nblk + 255) // 256, dtype=torch.float32, device=dev),
             "offset": torch.empty((), dtype=torch.float32, device=dev),
             "ws": torch.empty(wsz, dtype=torch.uint8, device=dev)} for _ in range(pout)]

    def single(i):
        o = outs[i % pout]
        assert L.nf4_quant_bnb(ins[i % pin].data_ptr(), code, numel, 64, o["packed"].data_ptr(),
                               o["absmax"].data_ptr(), torch.cuda.current_stream().cuda_stream) == 0

    def nested(i):
        o = outs[i % pout]
        assert L.nf4_quant_bnb_nested(ins[i % pin].data_ptr(), code, numel, 64, code2.data_ptr(), 256,
                                      o["packed"].data_ptr(), o["absmax_q"].data_ptr(), o["absmax2"].data_ptr(),
                                      o["offset"].data_ptr(), o["ws"].data_ptr(), wsz,
                                      torch.cuda.current_stream().cuda_stream) == 0

    results = {}
    for form, launch in (("single", single), ("nested", nested)):
        for i in range(max(pin, pout)):  # every set touched once
            launch(i)
        torch.cuda.synchronize()
        t = eager_per_launch(launch, steps, reps)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(steps):
                launch(i)
        tg = timed(graph.replay, reps) / steps
        pairs = last_writes(pin, pout, steps, limit=2 if numel <= 4096 * 4096 else 1)
        for a, b in pairs:
            verify((m, n, name, a), ins[a], outs[b], form == "nested")
        byt = alg_bytes(numel, esz, form == "nested")
        results[form] = t
        emit({"line": "quant", "m": m, "n": n, "in_dtype": name, "form": form, "launches_per_call": 1 if form == "single" else 3,
              "in_sets": pin, "out_sets": pout, "read_footprint_bytes": pin * numel * esz,
              "us_per_call": t * 1e6, "graph_us_per_call": tg * 1e6, "algorithmic_bytes": byt,
              "TBps": byt / t / 1e12, "frac_of_8TBps": byt / t / PEAK, "graph_frac_of_8TBps": byt / tg / PEAK,
              "verified": True, "verified_outputs": len(pairs),
              "timing": "eager launches behind a spin (bench.py's method); graph replay beside it"})

    # (b) the flat dequant of the same matrix (reference semantics over the nested outputs: the
    # flat kernel), the same rotation turned round; timed alternately with the quantizer
    dq_outs = [torch.empty((m, n), dtype=dt, device=dev) for _ in range(pin)]

    def dequant(i):
        o = outs[i % pout]
        assert L.nf4_dequant_ref(o["packed"].data_ptr(), numel // 2, o["absmax_q"].data_ptr(), nblk,
                                 o["absmax2"].data_ptr(), (nblk + 255) // 256, dq_outs[i % pin].data_ptr(), code, m, n,
                                 torch.cuda.current_stream().cuda_stream) == 0

    for i in range(max(pin, pout)):
        dequant(i)
    torch.cuda.synchronize()
    tq, td = [], []
    for _ in range(reps):
        tq.append(eager_per_launch(single, steps, 1))
        td.append(eager_per_launch(dequant, steps, 1))
    tq, td = sorted(tq)[reps // 2], sorted(td)[reps // 2]
    emit({"line": "vs_dequant", "m": m, "n": n, "dtype": name, "quant_single_us": tq * 1e6, "dequant_flat_us": td * 1e6,
          "quant_over_dequant": tq / td, "dequant_frac_of_8TBps": (numel // 2 + numel * esz + nblk) / td / PEAK})
    del dq_outs

    # (a) the torch-op quantizer on the device, through the same Python entry, alternately
    def hip_api(k):
        for i in range(k):
            nf4_quantize(ins[i % pin], compress_statistics=False)

    def torch_api(k):
        for i in range(k):
            quantize_nf4(ins[i % pin], compress_statistics=False)

    hip_api(2), torch_api(1)
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(reps):
        th.append(timed(lambda: hip_api(8), 1) / 8)
        tt.append(timed(lambda: torch_api(2), 1) / 2)
    th, tt = sorted(th)[reps // 2], sorted(tt)[reps // 2]
    emit({"line": "vs_torch", "m": m, "n": n, "dtype": name, "form": "single", "hip_us": th * 1e6, "torch_us": tt * 1e6,
          "speedup": tt / th, "hip_c_abi_us": results["single"] * 1e6})
    return tt / th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--shapes", default="4096x4096,14336x4096")
    ap.add_argument("--dtypes", default="bf16,fp16,fp32")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_quant.py needs a ROCm device"
    dev = torch.device("cuda", 0)
    fh = open(args.out, "a") if args.out else None

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    bar = None
    for shp in args.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        for name, dt, code in DTYPES:
            if name not in args.dtypes.split(","):
                continue
            sp = run_shape(m, n, name, dt, code, dev, args.reps, args.steps, emit)
            if (m, n, name) == (4096, 4096, "bf16"):
                bar = sp
            torch.cuda.empty_cache()
    if bar is not None:
        emit({"line": "bar", "what": "HIP single-level vs torch-op quantizer, 4096x4096 bf16", "speedup": bar,
              "required": MIN_SPEEDUP, "holds": bar >= MIN_SPEEDUP})
        if bar < MIN_SPEEDUP:
            sys.exit(1)


if __name__ == "__main__":
    main()
