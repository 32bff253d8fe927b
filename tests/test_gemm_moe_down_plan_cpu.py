"""The host plan of the fused expert down projection with the routed sum
(csrc/nf4_gemm_moe_down_plan.h), checked without a GPU: ``tests/plan/gemm_moe_down_plan_check.cpp``
is built for the host as a stand-alone program under AddressSanitizer + UBSan, as
test_gemm_moe_plan_cpu.py builds its own, run, and every line judged here.  Pinned: every status
code and the order of the rules, a workspace that is never empty for a valid call and its layout
(header, slabs, 16-bit scratch), the limit of (experts + 1) x column tiles tickets, and that cfg,
default choice and geometry are the expert GEMM's but for the kernel id."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
MOE, MOE_DOWN = 9, 12
HEADER = 64 * 1024 + 256


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("gemm_moe_down_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_moe_down_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_moe_down_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def _plans(lines, named=None):
    return [l for l in lines if l["k"] == "plan" and l["rc"] == OK and (named is None or l["named"] == named)]


def test_status_codes_in_order(lines):
    errs = {l["name"]: l for l in lines if l["k"] == "err"}
    want = {"arg_": ERR_ARG, "shape_": ERR_SHAPE, "too_large_": ERR_TOO_LARGE, "ok_": OK}
    counts = dict.fromkeys(want, 0)
    for name, l in errs.items():
        prefix = next(p for p in want if name.startswith(p))
        assert l["rc"] == want[prefix], (name, l)
        assert l["launch"] == (1 if prefix == "ok_" and "_p0_" not in name else 0), (name, l)
        counts[prefix] += 1
    assert counts == {"arg_": 24, "shape_": 5, "too_large_": 3, "ok_": 11}, counts
    for rule in ("arg_topk_0", "arg_topk_not_dividing", "arg_topk_beyond_p", "arg_rw_dtype", "arg_rw_other_16_bit_dtype",
                 "arg_null_rw", "arg_misaligned_rw_f32", "arg_misaligned_rw_16", "arg_misaligned_y",
                 "arg_cfg_expert_gemm_id", "arg_one_slice_no_workspace", "arg_short_workspace",
                 "arg_short_workspace_one_slice", "shape_before_topk", "arg_rw_dtype_first",
                 "too_large_tickets_one_slice", "too_large_tickets_before_workspace", "ok_tickets_fill_the_header",
                 "ok_p0_nothing", "ok_exact_workspace", "ok_exact_workspace_one_slice"):
        assert rule in errs, rule


def test_cfg_choice_and_geometry_are_the_expert_gemms(lines):
    plans = _plans(lines)
    assert len(plans) > 200 and len(_plans(lines, named=0)) == 16 + 18
    for p in plans:
        assert p["cfg"][0] == MOE_DOWN and p["moe"][0] == MOE and p["cfg"][1:] == p["moe"][1:], p
        assert p["geo"] == p["mgeo"], p
    # spelled out for Mixtral's w2 on the 256 CUs of an MI355X: K slices at 1, 4, 16 and 64 tokens
    by = {tuple(p["c"]): p for p in _plans(lines, named=0)}
    for P, ks in {2: 8, 8: 2, 32: 2, 128: 1}.items():
        assert by[(256, P, 8, 4096, 14336)]["cfg"] == [MOE_DOWN, 4, 1, ks, 2], P


def test_workspace_is_never_empty_and_laid_out_as_documented(lines):
    seen = set()
    for p in _plans(lines):
        _, P, E, N, K = p["c"]
        ksplit = p["cfg"][3]
        tiles, tickets = p["geo"][3], p["geo"][7]
        assert tickets == E * tiles and p["counters"] == tickets + tiles == (E + 1) * tiles, p
        assert p["counters"] * 4 <= 64 * 1024, p          # the tile tickets follow the (expert, tile) tickets
        slab = ksplit * P * N * 4 if ksplit > 1 else 0
        assert p["slab"] == slab and p["scratch_at"] == HEADER + slab and p["scratch_at"] % 16 == 0, p
        assert p["need"] == p["ws"] == HEADER + slab + P * N * 2 > 0, p
        seen.add(ksplit > 1)
    assert seen == {True, False}
