"""The host plan of the NF4 embedding gather (csrc/nf4_embed_plan.h) and the host entries'
guards, checked without a GPU: ``tests/plan/embed_plan_check.cpp`` (with
csrc/nf4_dequant_cpu.cpp compiled into it) is built for the host as a stand-alone program
under AddressSanitizer + UBSan, as test_gemm_bnb_plan_cpu.py builds its own, run, and every
line judged here.  Pinned: the form is aligned iff dim % 64 == 0 (with aligned pointers), the
launch tiles [0, count * dim) exactly once, the grid covers the work with at most one
workgroup to spare, every error rule, the too-large rule around 2^31 and 2^32 (refused,
never split), and that ids outside [0, rows) give zero rows from the host entries without
touching the tables (there a missing guard is a sanitizer report)."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
ALIGNED, GENERAL = 0, 1
WG = 256


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("embed_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "embed_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fno-fast-math", "-ffp-contract=off", "-pthread", *SAN,
           "-o", str(exe), os.path.join(REPO, "tests", "plan", "embed_plan_check.cpp"),
           os.path.join(REPO, "nf4_triton_dequantization_amd", "csrc", "nf4_dequant_cpu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def _plans(lines, tag=None):
    return [l for l in lines if l["k"] == "plan" and (tag is None or l["tag"] == tag)]


def test_form_is_aligned_iff_dim_is_a_multiple_of_64(lines):
    seen = set()
    for p in _plans(lines):
        if p["tag"].startswith("misaligned"):
            continue
        assert p["rc"] == OK and p["launches"] == 1, p
        assert (p["form"] == ALIGNED) == (p["dim"] % 64 == 0), p
        seen.add(p["form"])
    assert seen == {ALIGNED, GENERAL}
    # the aligned form loads dwords and stores 16 bytes: other pointers take the exact form
    for tag in ("misaligned_out", "misaligned_packed"):
        (p,) = _plans(lines, tag)
        assert p["rc"] == OK and p["form"] == GENERAL, p


def test_launches_tile_the_output_exactly_once(lines):
    assert len(_plans(lines)) > 600
    for p in _plans(lines):
        total = p["count"] * p["dim"]
        assert p["launches"] == 1 and (p["e0"], p["e1"]) == (0, total), p
        assert p["elems"] == total and p["block"] == WG, p
        if p["form"] == ALIGNED:
            assert p["blocks"] * 64 == total and p["bpr"] * 64 == p["dim"] and p["fd_ok"] == 1, p


def test_grid_covers_the_work_with_at_most_one_workgroup_to_spare(lines):
    for p in _plans(lines):
        per_wg = p["wg_blocks"] * 64 if p["form"] == ALIGNED else WG  # output elements per workgroup
        total = p["count"] * p["dim"]
        assert p["grid"] * per_wg >= total, p
        assert (p["grid"] - 1) * per_wg < total, p
        assert 1 <= p["grid"] < 2 ** 31, p


def test_blocks_per_lane_group(lines):
    """One 64-element block per 8-lane group up to 32768 output blocks (decode sizes), four above."""
    seen = set()
    for p in _plans(lines):
        if p["form"] == ALIGNED:
            assert p["steps"] == (1 if p["blocks"] <= 32768 else 4), p
            assert p["wg_blocks"] == WG // 8 * p["steps"], p
            seen.add(p["steps"])
        else:
            assert p["steps"] == 1, p
    assert seen == {1, 4}


def test_block_size_shifts(lines):
    (p,) = _plans(lines, "blocksizes")
    assert (p["bsh"], p["bsh2"]) == (12, 2), p
    (p,) = _plans(lines, "llama")
    assert (p["bsh"], p["bsh2"], p["form"], p["bpr"], p["blocks"]) == (6, 8, ALIGNED, 64, 32 * 64), p
    (p,) = _plans(lines, "rows0")  # an empty table: every id is out of range, the launch writes zeros
    assert p["rc"] == OK and p["launches"] == 1, p


def test_error_rules(lines):
    errs = {l["name"]: l for l in lines if l["k"] == "err"}
    want = {"arg_": ERR_ARG, "shape_": ERR_SHAPE, "too_large_": ERR_TOO_LARGE, "ok": OK}
    counts = dict.fromkeys(want, 0)
    for name, l in errs.items():
        prefix = next(p for p in want if name.startswith(p))
        assert l["rc"] == want[prefix], l
        counts[prefix] += 1
        if l["rc"] != OK or name.startswith("ok_count_0"):
            assert l["launches"] == 0, l  # an error or an empty call launches nothing
        else:
            assert l["launches"] == 1, l
    assert counts["arg_"] >= 17 and counts["shape_"] >= 8 and counts["ok"] >= 7, counts


def test_too_large_is_refused_never_split(lines):
    """count * dim <= 2^31 - 1 is one launch; anything above is NF4DQ_ERR_TOO_LARGE."""
    big = _plans(lines, "large_ok")
    assert len(big) == 3
    for p in big:
        assert p["rc"] == OK and p["launches"] == 1 and p["e1"] == p["count"] * p["dim"] <= 2 ** 31 - 1, p
    errs = {l["name"]: l for l in lines if l["k"] == "err" and l["name"].startswith("too_large")}
    assert {"too_large_2p31", "too_large_2p31_dim1", "too_large_2p32", "too_large_2p32_plus", "too_large_count_max",
            "too_large_table"} <= set(errs)
    for l in errs.values():
        assert l["rc"] == ERR_TOO_LARGE and l["launches"] == 0, l


def test_host_entries_zero_rows_for_ids_out_of_range(lines):
    cpu = [l for l in lines if l["k"] == "cpu"]
    assert len(cpu) == 18
    for l in cpu:
        assert l["rc"] == [OK, OK], l
        assert l["bad"] == (7 if l["ids64"] else 5), l
        assert l["zero_ok"] == 1 and l["same_ok"] == 1 and l["nonzero_valid"] == 1, l
