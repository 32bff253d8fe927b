"""The host plan of nf4_gemm_bnb_grouped, checked without a GPU:
``tests/plan/gemm_bnb_grouped_plan_check.cpp`` evaluates ``bnb_grouped_choice`` and
``bnb_grouped_workspace`` (csrc/nf4_gemm_plan.h) over the Llama q/k/v and gate/up groups and a
small one, K in {1024, 2048, 4096, 14336}, the M list of the single-weight check, 256 and 64
CUs, blocksize 64 and 128.  It is built for the host under AddressSanitizer + UBSan as
test_gemm_bnb_plan_cpu.py builds its own, run, and every line checked."""
from __future__ import annotations

import ctypes
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
K128, STREAM, PERSIST, XS, XR, GEMV = 1, 2, 3, 4, 5, 7
GROUPED = {K128, PERSIST, XR}
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("bnb_grouped_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_bnb_grouped_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_bnb_grouped_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def cases(lines):
    return lines[1:]


def test_struct_layout_equals_the_ctypes_mirror(lines):
    from nf4_triton_dequantization_amd import _lib

    M = _lib.GemmBnbMat
    names = ["packed", "packed_len", "absmax_q", "nb", "code2", "absmax2", "n2", "offset", "blocksize", "blocksize2",
             "y", "N"]
    assert [f[0] for f in M._fields_] == names
    assert lines[0]["mat"] == [ctypes.sizeof(M)] + [getattr(M, n).offset for n in names]


def test_choice_is_valid_for_every_weight_and_names_only_families_with_the_mode(cases):
    assert len(cases) == 2 * 2 * 4 * 12 * 3
    for c in cases:
        assert c["v"] == 1, c
        assert c["bnb"][0] in GROUPED and c["bnbs"][0] in GROUPED, c
        assert c["bnb"] == c["bnbs"] and c["pw"] == c["pws"], c  # nested and single: the same launch


def test_choice_is_the_reference_grouped_launch_where_the_family_has_the_mode(cases):
    same = gemv = sub = 0
    kernels = set()
    for c in cases:
        sh, ref = c["c"][3], c["ref"][0]
        if sh == 1:
            assert c["bnb"][0] == K128 and c["pw"] == 0, c  # blocksize 128: the 128-deep kernel alone
            sub += 1
        elif ref == GEMV:
            assert c["bnb"][0] == PERSIST, c  # what the plan picked there before the GEMV existed
            gemv += 1
        elif ref in GROUPED:
            assert c["bnb"] == c["ref"] and c["pw"] == c["refpw"], c
            # grid and block as the reference-mode launch of that cfg; dynamic LDS too, but for the
            # nested register-resident launch, which adds one code2 table (1 KiB) per weight and
            # 32 bytes of offsets behind its held results (single mode adds nothing)
            assert c["shape"][0:2] == c["shape"][3:5] == c["shape"][6:8], c
            assert c["shape"][5] == c["shape"][8], c
            extra = c["tables"] * 1024 + 32 if c["tables"] else 0
            assert (c["tables"] > 0) == (ref == XR), c
            assert c["shape"][2] == c["shape"][8] + extra, c
            same += 1
            kernels.add(ref)
        else:
            assert ref in (STREAM, XS) and c["bnb"][0] == K128 and c["pw"] == 0, c  # the substitute
            sub += 1
        if not c["pw"]:
            assert c["lds"] <= LDS_PER_CU, c  # static + dynamic LDS of the launch that runs
    print(f"grouped bnb plan: {same} cases run the reference launch, {gemv} the persistent kernel for the GEMV, "
          f"{sub} the 128-deep substitute")
    assert kernels == GROUPED and gemv > 0 and sub > 0, (kernels, gemv, sub)


def test_per_weight_fallback_only_where_the_reference_plan_falls_back(cases):
    n = 0
    for c in cases:
        if c["pw"]:
            assert c["bnb"][0] == PERSIST and c["refpw"] == 1 and c["c"][3] == 0, c
            n += 1
    assert n > 0  # the persistent cfg's held outputs beyond the LDS: 64 CUs, wide groups


def test_size_entry_covers_every_need(cases):
    for c in cases:
        assert c["ws"] >= c["need"], c
