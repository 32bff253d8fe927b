"""Randomised parity sweep of the fused decode GEMM (tools only).

    python tools/fuzz_gemm.py [--cases 1500] [--seed 1] [--seconds 500] > fuzz_gemm.jsonl

Each case draws M (1-32), N (a multiple of 64 up to 3072), K (a multiple of 128 up to
6144), the dtype (bf16 / fp16), full or short absmax arrays (the reference's repeat-wrap)
and signed nested absmax. It then runs ``nf4_linear`` (the library's choice of kernel
and decomposition) and, for a share of the cases (``--cfg-rate``), an explicitly drawn
configuration of any of the six kernels through ``nf4_gemm_ref_cfg`` (invalid draws are
skipped; a split-K timeout flagged in the workspace counts as a failure). Each result is
checked against a float64 product of the C oracle's dequantized weights with the GEMM
suite's tolerance
(tests/_gemm_cases.py: 2^-p |ref| + 2^-20 sum|x w|). Half of the ``--gemv-rate`` cases are
grouped M = 1 launches (2-4 weights in multiples of 64 columns sharing x, some with absmax
wrapping at row boundaries): up to 4096 columns in all through the library's choice, or up
to 8192 with a drawn GEMV configuration; each output against its own oracle. One progress
line per 100 cases, then a summary.

``--semantics bnb``: the bitsandbytes-semantics entries instead. Each case quantizes a drawn
float weight with ``nf4_quantize`` (nested or plain fp32 statistics, blocksize 64 / 128 / 512
/ 4096), runs ``Linear4bit.forward`` (``nf4_linear_bnb``, the library's choice) and, for
``--cfg-rate`` of the cases, a drawn configuration through ``nf4_gemm_bnb`` /
``nf4_gemm_bnb_single`` (a family without the mode is rejected and skipped); the oracle is
the C oracle's ``dequant_bnb`` / ``dequant_bnb_single``, same tolerance.

``--semantics family``: the row-tiled and the expert GEMM family (nf4_gemm_bnb_mt, _mt_swiglu, _moe,
_moe_swiglu, _moe_down) on the drawn cases of tests/_family_draws.py, run and judged exactly as
tests/test_gpu_gemm_family_drawn.py does (its ``Runner``: one workspace per (entry, dtype) sequence,
every call twice, the suites' own judges).  Round r draws ``--seed`` + r for each of the ten
(entry, dtype) sequences; ``--cases`` counts calls over all rounds.  One JSON line per failing case
with its fields.

``--semantics moe_rb``: the expert GEMM in row blocks (nf4_gemm_bnb_moe_rb, 1 .. 1024 pairs) on the drawn
calls of tests/_moe_rb_draws.py, run and judged exactly as tests/test_gpu_gemm_moe_rb_drawn.py does (its
``Runner``: one workspace per dtype sequence, every call twice, test_gpu_gemm_moe.py's judge, and
nf4_gemm_bnb_moe's bits on subsets of at most 128 pairs).  Round r draws ``--seed`` + r for both dtypes;
``--cases`` counts calls over all rounds, ``launches`` every launch of either entry.

``--semantics lora``: the fused adapter launch (nf4_lora_add) on the drawn grouped calls of
tests/_lora_draws.py, run and judged exactly as tests/test_gpu_lora_drawn.py does (its ``Runner``: all
outputs of a call in one allocation with sentinel gaps, every call twice, the float64 chain's bound).
Round r draws ``--seed`` + r for both dtypes; ``--cases`` counts calls over all rounds.

``--semantics lora_routed``: the routed adapter launch (nf4_lora_add_routed) on the drawn calls of
tests/_lora_routed_draws.py, run and judged exactly as tests/test_gpu_lora_routed_drawn.py does (its
``Runner``: padded strides, NaN in everything absent, every call twice, the float64 chain's bound per
adapter group, nf4_lora_add's bits under an explicit cfg).  Rounds and ``--cases`` as for ``lora``.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import nf4_oracle as O  # noqa: E402  -- the checker
from _helpers import make_module  # noqa: E402
from nf4_triton_dequantization_amd import _lib, nf4_linear  # noqa: E402


def bits_to_f64(bits, dt):
    if dt == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def tol(ref, mag, dt):
    p, sub = (8, 2.0 ** -134) if dt == "bf16" else (10, 2.0 ** -25)
    return 2.0 ** -p * np.abs(ref) + 2.0 ** -20 * mag + sub


def random_cfg(rng, M, N, K):
    """A drawn configuration of one of the six kernels (may be invalid: skipped)."""
    k = int(rng.choice([1, 2, 3, 4, 5, 7]))  # (6, the balanced kernel, was retired in round 6)
    if k == _lib.GEMM_GEMV:  # the decode GEMV: M = 1, K % 2048 == 0 (else rejected)
        return _lib.GemmCfg(k, int(rng.choice([8, 16])), int(rng.choice([1, 2, 4])), 1, int(rng.choice([0, 1, 2])))
    waves = int(rng.choice([4, 8, 16]))
    depth = int(rng.choice([1, 2, 4, 8]))
    strips = int(rng.choice([1, 2, 4]))
    if k == _lib.GEMM_XR:
        kpw = strips
        ks = -(-(K // 128) // (waves * kpw))
    elif k == _lib.GEMM_XS:
        ks = -(-(K // 128) // depth)
        strips = 1
    else:
        ks = int(rng.choice([1, 2, 4]))
    return _lib.GemmCfg(k, waves, depth, ks, strips)


def grouped_gemv_case(rng, L, orc, dev):
    """One grouped M = 1 launch in the decode GEMV's domain; returns (mismatch records, label)."""
    K = 2048 * int(rng.integers(1, 5))
    dt = "bf16" if rng.random() < 0.6 else "f16"
    cfg = None
    if rng.random() < 0.5:
        cfg = _lib.GemmCfg(_lib.GEMM_GEMV, int(rng.choice([8, 16])), int(rng.choice([1, 2, 4])), 1,
                           int(rng.choice([0, 1, 2])))
    limit = (8192 if cfg is not None else 4096) // 64
    count = int(rng.integers(2, 5))
    cuts = np.sort(rng.choice(np.arange(1, int(rng.integers(count, limit + 1))), count - 1, replace=False))
    widths = np.diff(np.concatenate([[0], cuts, [cuts[-1] + int(rng.integers(1, limit - cuts[-1] + 1))]]))
    Ns = [64 * int(w) for w in widths]
    assert len(Ns) == count and all(n > 0 for n in Ns) and sum(Ns) <= 64 * limit
    bpr, groups = K // 64, -(-(K // 64) // 4)
    seed = int(rng.integers(1, 1 << 30))
    x = O.normal_f32(seed + 1, K, stream=9).reshape(1, K)
    xt = torch.from_numpy(x).to(torch.bfloat16 if dt == "bf16" else torch.float16)
    xb = xt.view(torch.int16).numpy().view(np.uint16)
    xf = bits_to_f64(xb, dt)
    xd = xt.to(dev)
    mats = (_lib.GemmMat * count)()
    keep, ys, refs, ovs = [], [], [], []
    for i, N in enumerate(Ns):
        ov = {"a2_kind": "normal" if rng.random() < 0.5 else "uniform"}
        if rng.random() < 0.3:  # the statistics of a few rows, repeating: a wrap at row boundaries only
            ov["nb"] = bpr * int(rng.integers(1, N + 1))
            ov["n2"] = groups * int(rng.integers(1, N + 1))
        ovs.append(ov)
        p, a1, a2, _ = O.golden_case_inputs(N, K, seed + 7 * i, ov)
        wf = bits_to_f64(orc.dequant_ref(p, a1, a2, N, K, O.BF16 if dt == "bf16" else O.F16), dt)
        ref = xf @ wf.T
        refs.append((ref, tol(ref, np.abs(xf) @ np.abs(wf).T, dt)))
        t = [torch.from_numpy(v).to(dev) for v in (p, a1, a2)]
        keep.append(t)
        y = torch.full((1, N), float("nan"), dtype=xt.dtype, device=dev)
        ys.append(y)
        mats[i] = _lib.GemmMat(t[0].data_ptr(), t[0].numel(), t[1].data_ptr(), t[1].numel(), t[2].data_ptr(),
                               t[2].numel(), y.data_ptr(), N)
    cp = ctypes.byref(cfg) if cfg is not None else None
    wsz = L.nf4_gemm_grouped_workspace_bytes(1, K, mats, count, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    rc = L.nf4_gemm_ref_grouped(xd.data_ptr(), 1, K, mats, count, _lib.BF16 if dt == "bf16" else _lib.F16,
                                ws.data_ptr() if wsz else None, wsz, cp, sp)
    label = [cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips] if cfg is not None else "default"
    info = {"grouped": Ns, "K": K, "dtype": dt, "seed": seed, "ov": ovs, "path": label}
    if rc:
        return [dict(info, rc=int(rc))], label
    out = []
    if wsz and L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp):
        out.append(dict(info, timeout=True))
    for i, (y, (ref, bound)) in enumerate(zip(ys, refs)):
        got = bits_to_f64(y.view(torch.int16).cpu().numpy().view(np.uint16), dt).reshape(1, Ns[i])
        if not (np.abs(got - ref) <= bound).all():
            fin = np.abs(got - ref)[np.isfinite(got)]
            out.append(dict(info, weight=i, worst=float(fin.max()) if fin.size else None,
                            nan=int(np.isnan(got).sum())))
    return out, label


def bnb_case(rng, L, orc, dev, cfg_rate):
    """One bitsandbytes-semantics case; returns (mismatch records, explicit cfg runs)."""
    from nf4_triton_dequantization_amd import Linear4bit

    M = int(rng.integers(1, 33))
    N = 64 * int(rng.integers(1, 49))
    K = 128 * int(rng.integers(1, 49))
    if rng.random() < 0.15:  # the decode GEMV's domain
        M, N, K = 1, 64 * int(rng.integers(1, 65)), 2048 * int(rng.integers(1, 4))
    dt = "bf16" if rng.random() < 0.6 else "f16"
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    nested = bool(rng.random() < 0.7)
    bs = int(rng.choice([64, 64, 64, 128, 512, 4096]))
    seed = int(rng.integers(1, 1 << 30))
    wf = torch.from_numpy(O.normal_f32(seed, N * K, stream=8).reshape(N, K)).to(dev) * float(rng.choice([0.02, 1.0]))
    mod = Linear4bit.from_float(wf, compute_dtype=tdt, compress_statistics=nested, blocksize=bs)
    qs = mod.weight.quant_state
    packed = mod.weight.data.view(-1).cpu().numpy()
    code = O.BF16 if dt == "bf16" else O.F16
    if nested:
        w = orc.dequant_bnb(packed, qs.absmax.cpu().numpy(), qs.state2.code.cpu().numpy(),
                            qs.state2.absmax.cpu().numpy(), float(qs.offset), N * K, code, bs, int(qs.state2.blocksize))
    else:
        w = orc.dequant_bnb_single(packed, qs.absmax.cpu().numpy(), N * K, code, bs)
    x = O.normal_f32(seed + 1, M * K, stream=9).reshape(M, K)
    xt = torch.from_numpy(x).to(tdt)
    xb = xt.view(torch.int16).numpy().view(np.uint16)
    xf, wf64 = bits_to_f64(xb, dt), bits_to_f64(w.reshape(N, K), dt)
    ref = xf @ wf64.T
    bound = tol(ref, np.abs(xf) @ np.abs(wf64).T, dt)
    xd = xt.to(dev)
    with torch.no_grad():
        outs = [("default", mod(xd))]
    info = {"semantics": "bnb", "M": M, "N": N, "K": K, "dtype": dt, "seed": seed, "nested": nested, "blocksize": bs}
    records, ran = [], 0
    if rng.random() < cfg_rate:
        cfg = random_cfg(rng, M, N, K)
        wsz = L.nf4_gemm_bnb_workspace_bytes(M, N, K, ctypes.byref(cfg))
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=dev)
        y = torch.empty((M, N), dtype=tdt, device=dev)
        q = mod.weight.data
        sp = torch.cuda.current_stream().cuda_stream
        tail = (y.data_ptr(), _lib.BF16 if dt == "bf16" else _lib.F16, N, K, ws.data_ptr() if wsz else None, wsz,
                ctypes.byref(cfg), sp)
        if nested:
            rc = L.nf4_gemm_bnb(xd.data_ptr(), M, q.data_ptr(), q.numel(), qs.absmax.data_ptr(), qs.absmax.numel(),
                                qs.state2.code.data_ptr(), qs.state2.absmax.data_ptr(), qs.state2.absmax.numel(),
                                qs.offset.data_ptr(), bs, int(qs.state2.blocksize), *tail)
        else:
            rc = L.nf4_gemm_bnb_single(xd.data_ptr(), M, q.data_ptr(), q.numel(), qs.absmax.data_ptr(),
                                       qs.absmax.numel(), bs, *tail)
        if rc == 0:
            ran = 1
            label = [cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips]
            if wsz and L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, sp):
                records.append(dict(info, timeout=True, path=label))
            outs.append((label, y))
    for label, y in outs:
        got = bits_to_f64(y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), dt).reshape(M, N)
        if not (np.abs(got - ref) <= bound).all():
            records.append(dict(info, path=label, worst=float(np.nanmax(np.abs(got - ref))),
                                nan=int(np.isnan(got).sum())))
    return records, ran


def family_sweep(args, orc, dev):
    """--semantics family: rounds of the ten drawn sequences until --cases or --seconds is reached."""
    import _family_draws as D
    import test_gpu_gemm_family_drawn as T

    t0 = time.time()
    done = bad = stale = rounds = 0
    per_entry = {e: 0 for e in D.ENTRIES}
    while done < args.cases and time.time() - t0 <= args.seconds:
        seed = args.seed + rounds
        for entry in D.ENTRIES:
            for dt in D.DTYPES:
                cases = D.draws(entry, dt, seed)
                runner = T.Runner(entry, dt, orc, dev)
                runner.prepare(cases)
                for c in cases:
                    if done >= args.cases or time.time() - t0 > args.seconds:
                        break
                    try:
                        runner.run(c)
                    except AssertionError as e:
                        bad += 1
                        print(json.dumps({"mismatch": dict(c.fields(), semantics="family", error=str(e).split("\n", 1)[-1][:400])}),
                              flush=True)
                    done += 1
                    per_entry[entry] += 1
                stale += runner.stale_slab_calls
                T._STACKS.clear()
        rounds += 1
        print(json.dumps({"progress": done, "mismatches": bad, "rounds": rounds, "seconds": round(time.time() - t0, 1)}), flush=True)
    print(json.dumps({"summary": {"semantics": "family", "cases": done, "launches": 2 * done, "per_entry": per_entry,
                                  "rounds": rounds, "mismatches": bad, "moe_down_calls_over_stale_products": stale,
                                  "seed": args.seed, "seconds": round(time.time() - t0, 1)}}), flush=True)


def moe_rb_sweep(args, orc, dev):
    """--semantics moe_rb: rounds of the two drawn sequences until --cases or --seconds is reached."""
    import _moe_rb_draws as D
    import test_gpu_gemm_family_drawn as FT
    import test_gpu_gemm_moe_rb_drawn as T

    t0 = time.time()
    done = bad = rounds = launches = 0
    per_dtype = {dt: 0 for dt in D.DTYPES}
    while done < args.cases and time.time() - t0 <= args.seconds:
        seed = args.seed + rounds
        for dt in D.DTYPES:
            cases = D.draws(dt, seed)
            runner = T.Runner(dt, orc, dev)
            runner.prepare(cases)
            for c in cases:
                if done >= args.cases or time.time() - t0 > args.seconds:
                    break
                try:
                    runner.run(c)
                except AssertionError as e:
                    bad += 1
                    print(json.dumps({"mismatch": dict(c.fields(), semantics="moe_rb", error=str(e).split("\n", 1)[-1][:400])}),
                          flush=True)
                done += 1
                per_dtype[dt] += 1
            launches += runner.launches
        FT._STACKS.clear()  # the next round's pool
        rounds += 1
        print(json.dumps({"progress": done, "mismatches": bad, "rounds": rounds, "seconds": round(time.time() - t0, 1)}), flush=True)
    print(json.dumps({"summary": {"semantics": "moe_rb", "cases": done, "launches": launches, "per_dtype": per_dtype,
                                  "rounds": rounds, "mismatches": bad, "seed": args.seed, "seconds": round(time.time() - t0, 1)}}),
          flush=True)


def lora_sweep(args, dev):
    """--semantics lora / lora_routed: rounds of the two drawn sequences until --cases or --seconds is reached."""
    routed = args.semantics == "lora_routed"
    if routed:
        import _lora_routed_draws as D
        import test_gpu_lora_routed_drawn as T
    else:
        import _lora_draws as D
        import test_gpu_lora_drawn as T

    t0 = time.time()
    done = bad = adapters = rounds = launches = 0
    per_dtype = {dt: 0 for dt in D.DTYPES}
    while done < args.cases and time.time() - t0 <= args.seconds:
        seed = args.seed + rounds
        for dt in D.DTYPES:
            runner = T.Runner(dt, dev)
            for c in D.draws(dt, seed):
                if done >= args.cases or time.time() - t0 > args.seconds:
                    break
                try:
                    runner.run(c)
                except AssertionError as e:
                    bad += 1
                    print(json.dumps({"mismatch": dict(c.fields(), semantics=args.semantics, error=str(e).split("\n", 1)[-1][:400])}), flush=True)
                done += 1
                adapters += len(c.stacks) * len(c.groups) if routed else len(c.adapters)  # routed: adapter groups judged
                per_dtype[dt] += 1
            launches += runner.launches
        rounds += 1
        print(json.dumps({"progress": done, "mismatches": bad, "rounds": rounds, "seconds": round(time.time() - t0, 1)}), flush=True)
    print(json.dumps({"summary": {"semantics": args.semantics, "cases": done, "launches": launches, "adapters": adapters, "per_dtype": per_dtype,
                                  "rounds": rounds, "mismatches": bad, "seed": args.seed, "seconds": round(time.time() - t0, 1)}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--semantics", choices=["ref", "bnb", "family", "moe_rb", "lora", "lora_routed"], default="ref",
                    help="ref: nf4_gemm_ref and its kin; bnb: nf4_gemm_bnb / nf4_gemm_bnb_single on nf4_quantize's weights; "
                         "family: the row-tiled and expert GEMMs on the drawn cases of tests/_family_draws.py; "
                         "moe_rb: nf4_gemm_bnb_moe_rb on the drawn calls of tests/_moe_rb_draws.py; "
                         "lora: nf4_lora_add on the drawn grouped calls of tests/_lora_draws.py; "
                         "lora_routed: nf4_lora_add_routed on the drawn calls of tests/_lora_routed_draws.py")
    ap.add_argument("--cases", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=500.0)
    ap.add_argument("--cfg-rate", type=float, default=0.25, help="share of cases that also run a drawn configuration")
    ap.add_argument("--gemv-rate", type=float, default=0.0,
                    help="share of cases at M = 1 with K % 2048 == 0 and N <= 4096 (the decode GEMV's domain); "
                         "half of them grouped launches of 2-4 weights")
    ap.add_argument("--boundary-rate", type=float, default=0.1,
                    help="share of cases drawn from the default-rule boundary shapes (large N, K = 14336)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    if args.semantics in ("lora", "lora_routed"):
        return lora_sweep(args, dev)
    orc = O.COracle()
    if args.semantics == "family":
        return family_sweep(args, orc, dev)
    if args.semantics == "moe_rb":
        return moe_rb_sweep(args, orc, dev)
    rng = np.random.default_rng(args.seed)
    t0 = time.time()
    done = bad = cfg_runs = grouped_runs = 0

    def progress():
        if done % 100 == 0:
            print(json.dumps({"progress": done, "mismatches": bad, "cfg_runs": cfg_runs, "grouped_runs": grouped_runs,
                              "seconds": round(time.time() - t0, 1)}), flush=True)

    for i in range(args.cases):
        if time.time() - t0 > args.seconds:
            break
        if args.semantics == "bnb":
            records, ran = bnb_case(rng, L, orc, dev, args.cfg_rate)
            for r in records:
                bad += 1
                print(json.dumps({"mismatch": r}), flush=True)
            cfg_runs += ran
            done += 1
            progress()
            continue
        M = int(rng.integers(1, 33))
        N = 64 * int(rng.integers(1, 49))
        K = 128 * int(rng.integers(1, 49))
        if rng.random() < args.boundary_rate:
            # the default-rule boundaries the uniform draw cannot reach: M on
            # either side of 8 / 16 / 24, the wide launches (16-wave whole-K XR at
            # N >= 24576, persistent strips = 4 at N >= 8192) and the down projection's K
            M = int(rng.choice([1, 8, 9, 16, 17, 24, 25, 32]))
            N, K = [(1024, 4096), (4096, 4096), (8192, 4096), (14336, 4096), (24576, 4096), (28672, 4096),
                    (4096, 14336), (1024, 14336)][int(rng.integers(0, 8))]
        if rng.random() < args.gemv_rate:
            if rng.random() < 0.5:
                records, _label = grouped_gemv_case(rng, L, orc, dev)
                for r in records:
                    bad += 1
                    print(json.dumps({"mismatch": r}), flush=True)
                grouped_runs += 1
                done += 1
                progress()
                continue
            M, N, K = 1, 64 * int(rng.integers(1, 65)), 2048 * int(rng.integers(1, 9))
        dt = "bf16" if rng.random() < 0.6 else "f16"
        nb_full = N * K // 64
        ov = {"a2_kind": "normal" if rng.random() < 0.5 else "uniform"}
        if rng.random() < 0.2:
            ov["nb"] = int(rng.integers(1, nb_full + 1))
        seed = int(rng.integers(1, 1 << 30))
        p, a1, a2, _ = O.golden_case_inputs(N, K, seed, ov)
        w = orc.dequant_ref(p, a1, a2, N, K, O.BF16 if dt == "bf16" else O.F16)
        x = O.normal_f32(seed + 1, M * K, stream=9).reshape(M, K)
        xt = torch.from_numpy(x).to(torch.bfloat16 if dt == "bf16" else torch.float16)
        xb = xt.view(torch.int16).numpy().view(np.uint16)
        xf, wf = bits_to_f64(xb, dt), bits_to_f64(w, dt)
        ref = xf @ wf.T
        bound = tol(ref, np.abs(xf) @ np.abs(wf).T, dt)
        mod = make_module(p, a1, a2, N, K, dt, dev)
        outs = [("default", nf4_linear(xt.to(dev), mod))]
        if rng.random() < args.cfg_rate:
            cfg = random_cfg(rng, M, N, K)
            wsz = L.nf4_gemm_workspace_bytes_cfg(M, N, K, ctypes.byref(cfg))
            ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=dev)
            y = torch.empty((M, N), dtype=xt.dtype, device=dev)
            q = mod.weight.data
            qs = mod.weight.quant_state
            rc = L.nf4_gemm_ref_cfg(xt.to(dev).data_ptr(), M, q.data_ptr(), q.numel(), qs.absmax.data_ptr(),
                                    qs.absmax.numel(), qs.state2.absmax.data_ptr(), qs.state2.absmax.numel(),
                                    y.data_ptr(), _lib.BF16 if dt == "bf16" else _lib.F16, N, K,
                                    ws.data_ptr() if wsz else None, wsz, ctypes.byref(cfg),
                                    torch.cuda.current_stream().cuda_stream)
            if rc == 0:
                cfg_runs += 1
                label = [cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips]
                if wsz and L.nf4_gemm_check_workspace(ws.data_ptr(), wsz, torch.cuda.current_stream().cuda_stream):
                    bad += 1
                    print(json.dumps({"timeout": {"M": M, "N": N, "K": K, "cfg": label, "seed": seed}}), flush=True)
                outs.append((label, y))
        for label, y in outs:
            got = bits_to_f64(y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), dt).reshape(M, N)
            if not (np.abs(got - ref) <= bound).all():
                bad += 1
                print(json.dumps({"mismatch": {"M": M, "N": N, "K": K, "dtype": dt, "seed": seed, "ov": ov,
                                               "path": label,
                                               "worst": float(np.abs(got - ref).max())}}), flush=True)
        done += 1
        progress()
    print(json.dumps({"summary": {"semantics": args.semantics, "cases": done, "explicit_cfg_runs": cfg_runs, "grouped_runs": grouped_runs,
                                  "mismatches": bad,
                                  "seed": args.seed, "seconds": round(time.time() - t0, 1)}}), flush=True)


if __name__ == "__main__":
    main()
