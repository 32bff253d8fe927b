"""Device assembly and resource usage of the row-tiled GEMM family (nf4_gemm_mt.hip,
nf4_gemm_mt_swiglu.hip, nf4_gemm_moe.hip, nf4_gemm_moe_rb.hip, nf4_gemm_moe_swiglu.hip, nf4_gemm_moe_down.hip) or, with
``--family lora``, of the adapter launches (nf4_lora.hip, nf4_lora_routed.hip), and one tree's
kernels against another's.

    python tools/gemm_mt_family_asm.py --out DIR [--family gemm|lora] [--csrc DIR] [--tables] [--against DIR]

Compiles the family's sources of ``--csrc`` (default: this tree's; one that tree lacks is left out)
to device assembly with the
Makefile's flags (``--cuda-device-only -S -Rpass-analysis=kernel-resource-usage``, without
-Werror) into ``--out``.  ``--tables`` rewrites profiles/gemm_{mt,mt_swiglu,moe,moe_rb,moe_swiglu,moe_down}/resource_usage.txt
from the compiler's remarks.  ``--against DIR`` (an ``--out`` of another tree, e.g. the parent
commit's sources) compares kernel by kernel: the instruction streams after dropping comments and
directives and renumbering labels, and where they differ scratch, spills, waves per SIMD,
AGPRs, the LDS bytes the compiler reports and the v_mfma count; it exits 1 when one of those
differs.  These kernels' LDS is all dynamic, so the compiler reports 0 and the tables' LDS
column is the launch's size as the plan headers compute it (`*_lds_bytes`), not a measurement:
a change of it shows in the plan snapshot tests, not here.  The adapter launches have no
resource tables: ``--family lora`` compiles and compares only, kernel by kernel over (DT, MB, RT).
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "nf4_triton_dequantization_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the Makefile's default


def makefile_flags():
    """The Makefile's HIPFLAGS for gfx950 without -Werror (it turns the driver's unused
    --hip-link into an error in this mode), plus what makes assembly and remarks."""
    text = open(os.path.join(PKG, "Makefile")).read().replace("\\\n", " ")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f != "-Werror"] + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


FLAGS = makefile_flags()
# source -> (profiles directory, the kernel template as the source instantiates it, bytes of tables behind
# the x buffers: the plan headers' k*TableBytes)
FAMILY = {"nf4_gemm_mt": ("gemm_mt", "nf4_gemm_mt_kernel<DT, MT, SM, WV>", 1104),
          "nf4_gemm_mt_swiglu": ("gemm_mt_swiglu", "nf4_gemm_mt_swiglu_kernel<DT, MT, SM, WV>", 2128),
          "nf4_gemm_moe": ("gemm_moe", "nf4_gemm_moe_kernel<DT, MT, SM, WV> (DOWN = false, W = 1)", 2128),
          "nf4_gemm_moe_rb": ("gemm_moe_rb", "nf4_gemm_moe_kernel<DT, MT, SM, WV, false, 1, true> (RB: row blocks of 128 listed rows, W = 1)", 2128),
          "nf4_gemm_moe_swiglu": ("gemm_moe_swiglu", "nf4_gemm_moe_kernel<DT, MT, SM, WV, false, 2> (W = 2: gate and up, SwiGLU)", 3152),
          "nf4_gemm_moe_down": ("gemm_moe_down", "nf4_gemm_moe_kernel<DT, MT, SM, WV, true> (DOWN: the routed sum, W = 1)", 2128)}
# the adapter launches: source -> the kernel template; 16 instantiations each, no tables
LORA = {"nf4_lora": "lora_kernel<DT, MB, RT, false> (was nf4_lora_kernel<DT, MB, RT>)",
        "nf4_lora_routed": "lora_kernel<DT, MB, RT, true> (was nf4_lora_routed_kernel<DT, MB, RT>)"}
FAMILIES = {"gemm": FAMILY, "lora": LORA}
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "waves", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
          "LDS Size [bytes/block]": "static_lds"}


def compile_all(csrc, out, family):
    os.makedirs(out, exist_ok=True)
    procs = []
    for src in family:
        if not os.path.exists(os.path.join(csrc, src + ".hip")):
            continue
        log = open(os.path.join(out, src + ".log"), "w")
        cmd = [HIPCC, *FLAGS, "-I", os.path.join(REPO, "include"), "-o", os.path.join(out, src + ".s"),
               os.path.join(csrc, src + ".hip")]
        procs.append((src, subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT)))
    for src, p in procs:
        if p.wait() != 0:
            sys.exit(f"{src}: compile failed, see {out}/{src}.log")


def kernels(out, src):
    """{mangled name: {resources, insts}} of one compiled source."""
    res, name = {}, None
    for line in open(os.path.join(out, src + ".log")):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            res[name] = {"insts": []}
        elif m.group(1) in FIELDS:
            res[name][FIELDS[m.group(1)]] = int(m.group(2))
    cur = None
    for line in open(os.path.join(out, src + ".s")):
        line = line.split(";")[0].rstrip()
        assert "s_swappc" not in line, f"{src}: a call in device code -- a pipeline stage was not inlined"
        m = re.match(r"^(\w+):$", line)
        if m and m.group(1) in res:
            cur, labels = res[m.group(1)]["insts"], {}
        elif cur is not None and line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and re.match(r"^\s+[a-z]\w*", line):
            cur.append(re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line.strip()))
    return res


def params(name):
    """The leading template parameters of a mangled kernel name: (DT, MT, SM, WV), or (DT, MB, RT)
    of an adapter kernel.  A kernel that was renamed or gained parameters behind these still maps
    to its parent by them."""
    lora = re.search(r"lora\w*kernelILi(\d+)ELi(\d+)ELi(\d+)E", name)
    if lora:
        return tuple(int(v) for v in lora.groups())
    dt, mt, sm, wv = (int(v) for v in re.search(r"kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups())
    return dt, mt, sm, wv


def write_table(out, src):
    prof, kernel, tables = FAMILY[src]
    ks = kernels(out, src)
    rows = [f"{kernel}: hipcc {' '.join(f for f in FLAGS if f not in ('-fPIC', '-Wall', '-S', '--cuda-device-only'))}",
            f"(LDS is dynamic: two x buffers of 16 MT rows x 256 bytes + {tables} bytes behind them; static LDS 0."
            "  Columns: the compiler's remarks; SGPRs = TotalSGPRs; spills: SGPR + VGPR; LDS bytes: computed as the"
            " plan header does, not measured)", "",
            "dtype row_tiles mode    waves  VGPRs  AGPRs  SGPRs  scratch  spills  waves/SIMD  LDS bytes  v_mfma"]
    for sm in (2, 1):  # kScaleBnbSingle, kScaleBnb
        for dt in (1, 0):  # NF4DQ_BF16, NF4DQ_F16
            for name, k in sorted(ks.items(), key=lambda it: (params(it[0])[1], -params(it[0])[3])):
                d, mt, s, wv = params(name)
                if (d, s) != (dt, sm):
                    continue
                assert k["static_lds"] == 0
                rows.append(f"{'bf16' if dt else 'f16':<5}{mt:>10} {'nested' if sm == 1 else 'single':<7}{wv:>6}"
                            f"{k['vgprs']:>7}{k['agprs']:>7}{k['sgprs']:>7}{k['scratch']:>9}{k['sgpr_spill'] + k['vgpr_spill']:>8}"
                            f"{k['waves']:>12}{2 * 16 * mt * 256 + tables:>11}{sum(i.startswith('v_mfma') for i in k['insts']):>8}")
    # (profiles/gemm_moe_down/resource_usage.txt is the expert GEMM's own kernels against the parent's)
    table = "resource_usage_down.txt" if src == "nf4_gemm_moe_down" else "resource_usage.txt"
    with open(os.path.join(REPO, "profiles", prof, table), "w") as f:
        f.write("\n".join(rows) + "\n")


def compare(out, base, family):
    bad = 0
    what, count = ("DT,MB,RT", 16) if family is LORA else ("DT,MT,SM,WV", 32)
    for src in family:
        if not os.path.exists(os.path.join(base, src + ".s")):
            print(f"{src}: not in the other tree")
            continue
        # by template parameters: a parameter added behind them changes the mangled names
        new, old = ({params(n): k for n, k in kernels(d, src).items()} for d in (out, base))
        assert sorted(new) == sorted(old) and len(new) == count, (src, len(new), len(old))
        same = 0
        for name in sorted(new):
            n, o = new[name], old[name]
            if n["insts"] == o["insts"]:
                same += 1
                continue
            mf = [sum(i.startswith("v_mfma") for i in k["insts"]) for k in (n, o)]
            keep = all(n[f] == o[f] for f in ("scratch", "sgpr_spill", "vgpr_spill", "waves", "agprs", "static_lds")) and mf[0] == mf[1]
            bad += not keep
            print(f"{src} {what}={name}: streams differ ({len(o['insts'])} -> {len(n['insts'])} instructions); "
                  f"VGPRs {o['vgprs']} -> {n['vgprs']}, SGPRs {o['sgprs']} -> {n['sgprs']}, AGPRs {o['agprs']} -> {n['agprs']}, "
                  f"scratch {o['scratch']} -> {n['scratch']}, spills {o['sgpr_spill'] + o['vgpr_spill']} -> "
                  f"{n['sgpr_spill'] + n['vgpr_spill']}, waves/SIMD {o['waves']} -> {n['waves']}, v_mfma {mf[1]} -> {mf[0]}"
                  f"{'' if keep else '  <-- NOT KEPT'}")
        print(f"{src}: {same} of {len(new)} instantiations have identical instruction streams")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(PKG, "csrc"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--family", default="gemm", choices=sorted(FAMILIES))
    ap.add_argument("--tables", action="store_true")
    ap.add_argument("--against", default="")
    ap.add_argument("--no-compile", action="store_true", help="--out already holds the .s and .log files")
    args = ap.parse_args()
    family = FAMILIES[args.family]
    if not args.no_compile:
        compile_all(args.csrc, args.out, family)
    if args.tables and family is LORA:
        sys.exit("--tables: the adapter launches have no resource tables")
    if args.tables:
        for src in FAMILY:
            if os.path.exists(os.path.join(args.out, src + ".s")):
                write_table(args.out, src)
    if args.against and compare(args.out, args.against, family):
        sys.exit(1)


if __name__ == "__main__":
    main()
