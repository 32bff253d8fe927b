"""The host plan of the bitsandbytes-semantics GEMM entries, checked without a GPU:
``tests/plan/gemm_bnb_plan_check.cpp`` evaluates ``bnb_choice`` (csrc/nf4_gemm_plan.h) over
the reference plan check's single-weight (M, K, N) cases; it is built for the host under
AddressSanitizer + UBSan as test_gemm_plan_cpu.py builds its own, run, and every line checked:
the bnb choice is valid for the weight, names only families that have the mode, equals the
reference plan's launch wherever that family has it (blocksize 64) -- with the same grid,
block and dynamic LDS -- and its workspace need is covered by the size entry."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
K128, STREAM, PERSIST, XS, XR, GEMV = 1, 2, 3, 4, 5, 7
WITH_MODE = {K128, PERSIST, XR, GEMV}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("bnb_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_bnb_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_bnb_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def test_bnb_choice_is_valid_and_names_only_families_with_the_mode(cases):
    assert len(cases) > 400
    for c in cases:
        assert c["v"] == 1, c
        assert c["bnb"][0] in WITH_MODE and c["bnbs"][0] in WITH_MODE, c
        assert c["bnb"] == c["bnbs"], c  # nested and single: the same launch


def test_bnb_choice_is_the_reference_choice_where_the_family_has_the_mode(cases):
    same = sub = 0
    kernels = set()
    for c in cases:
        sh = c["c"][4]
        if sh == 0 and c["ref"][0] in WITH_MODE:
            assert c["bnb"] == c["ref"], c
            assert c["shape"][:3] == c["shape"][3:], c  # grid, block, dynamic LDS as the reference launch
            same += 1
            kernels.add(c["bnb"][0])
        else:
            assert c["bnb"][0] == K128, c  # the substitute: the 128-deep kernel
            assert sh > 0 or c["ref"][0] in (STREAM, XS), c
            sub += 1
    print(f"bnb plan: {same} cases run the reference launch, {sub} the 128-deep substitute")
    assert kernels == WITH_MODE, kernels  # each family with the mode is the library's choice somewhere
    assert sub > 0


def test_size_entry_covers_the_need(cases):
    for c in cases:
        assert c["ws"] >= c["need"], c
