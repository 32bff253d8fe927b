"""The fused GEMM's host plan, pinned without a GPU.  ``csrc/nf4_gemm_plan.h`` is plain
C++: which kernel and decomposition a call runs, its fallbacks, workspace sizes and every
family's grid / block / dynamic LDS.  ``tests/plan/gemm_plan_check.cpp`` prints all of it
for a fixed list of cases; this builds it for the host under AddressSanitizer + UBSan,
runs it and compares line by line with ``tests/plan/gemm_plan_snapshot.jsonl`` (recorded
from the dispatch as it stood before the plan was split out: a change of any line is a
change of a library choice or a launch shape, and wants a measurement behind it)."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
GEMV, PERSIST = 7, 3


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("plan")
    # the sanitizer runtimes first, on a program of one line: only their absence skips;
    # a failure to build the check program itself is a failure
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_plan_matches_the_snapshot(plan_lines):
    with open(os.path.join(REPO, "tests", "plan", "gemm_plan_snapshot.jsonl")) as f:
        want = f.read().splitlines()
    assert len(plan_lines) == len(want)
    differ = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, plan_lines)) if w != g]
    assert not differ, f"{len(differ)} lines differ; first (line, snapshot, now): {differ[0]}"


def test_plan_properties(plan_lines):
    cases = [json.loads(l) for l in plan_lines]
    assert len(cases) > 600
    kernels = set()
    for c in cases:
        wrap, ns = c["c"][3], c["c"][4:]
        # every cfg that runs (and the one the entry validates) is valid for every non-empty weight
        assert c["v"] == 1, c
        # the library-choice size entries cover whatever the call checks the workspace
        # against (the grouped one for any group, the single one for one weight); given
        # the cfg of a launch over all the weights, the two entries agree
        assert c["ws"][2] >= c["need"], c
        if len(ns) == 1:
            assert c["ws"][0] >= c["need"], c
        if len(c["l"]) == 1:
            assert c["ws"][1] == c["ws"][3] <= c["ws"][2], c
        if c["rc"] == 0:
            assert c["l"], c
            # one launch over all the weights, or one per weight
            assert [l[5] for l in c["l"]] in ([len(ns)], [1] * len(ns)), c
        else:
            assert c["rc"] == 2 and 0 in ns and not c["l"], c
        for l in c["l"]:
            kernels.add(l[0])
            assert l[6] >= 1 and l[7] == 64 * l[1] and l[8] <= 160 * 1024, c
            if wrap:  # absmax wrapping inside a row: never the GEMV, never the persistent kernel
                assert l[0] not in (GEMV, PERSIST), c
    assert kernels == {1, 2, 3, 4, 5, 7}, kernels  # every family is somebody's choice
