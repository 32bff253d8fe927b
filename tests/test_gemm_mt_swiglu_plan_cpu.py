"""The host plan of the fused gate/up SwiGLU launch (csrc/nf4_gemm_mt_swiglu_plan.h), checked
without a GPU: ``tests/plan/gemm_mt_swiglu_plan_check.cpp`` is built for the host as a stand-alone
program under AddressSanitizer + UBSan, exactly as test_gemm_mt_plan_cpu.py builds its own, run,
and every line judged here.  Pinned: every validation code, the library's choice and the launch
geometry at (14336, 4096) and (11008, 4096) for 1, 33, 64 and 128 rows, LDS within 160 KiB for
every valid cfg, and that the workspace the launcher asks for is what the size entry answers."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
SWIGLU = 10
HEADER = 64 * 1024 + 256
LDS_PER_CU = 160 * 1024
SHAPES = [(14336, 4096), (11008, 4096), (4096, 4096), (1024, 8192)]  # (I, K)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("gemm_mt_swiglu_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_mt_swiglu_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_mt_swiglu_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def _plans(lines, named=None):
    return [l for l in lines if l["k"] == "plan" and (named is None or l["named"] == named)]


def test_validation_codes(lines):
    errs = {l["name"]: l["rc"] for l in lines if l["k"] == "err"}
    want = {"arg_": ERR_ARG, "shape_": ERR_SHAPE, "too_large_": ERR_TOO_LARGE, "ok_": OK}
    counts = dict.fromkeys(want, 0)
    for name, rc in errs.items():
        prefix = next(p for p in want if name.startswith(p))
        assert rc == want[prefix], (name, rc)
        counts[prefix] += 1
    assert counts == {"arg_": 48, "shape_": 30, "too_large_": 6, "ok_": 12}, counts
    # the rules of the issue's table, in both statistics modes; the per-weight ones on either weight
    for rule in ("shape_m0_", "shape_m129_", "shape_i96_", "shape_i0_", "shape_k1088_", "shape_k64_", "arg_act_",
                 "arg_misaligned_x_", "arg_misaligned_h_", "arg_no_workspace_", "arg_short_workspace_",
                 "arg_misaligned_workspace_", "arg_cfg_ksplit_", "arg_cfg_parent_family_", "too_large_i_",
                 "too_large_packed_", "too_large_workspace_"):
        assert rule + "n_" in errs and rule + "s_" in errs, rule
    for rule in ("shape_n_differ_", "shape_blocksize_128_", "shape_packed_len_", "shape_short_stats_",
                 "arg_misaligned_packed_", "arg_null_packed_", "arg_blocksize_"):
        for w in ("gate_", "up_"):
            assert rule + w + "n_" in errs and rule + w + "s_" in errs, (rule, w)


def _expected_choice(cus, I, K):
    """The row-tiled family's rule over this launch's tiles: four waves (64 columns of h), and as
    many K slices as keep the grid within the CUs, at most 16 and at most one per six chunks."""
    tiles = I // 64
    return [SWIGLU, 4, 1, max(1, min(cus // tiles, 16, K // 128 // 6)), 2]


def test_library_choice_and_geometry_at_the_mlp_shapes(lines):
    by = {tuple(p["c"]): p for p in _plans(lines, named=0)}
    for cus in (256, 64):
        for I, K in SHAPES:
            for M in (1, 33, 64, 128):
                p = by[(cus, M, I, K)]
                assert p["rc"] == OK and p["cfg"] == _expected_choice(cus, I, K), p
    # spelled out for the 256 CUs of an MI355X: [kernel, waves, K stage, K slices, strips per wave] and
    # [grid, block, LDS, tiles, chunks, chunks per slice, row tiles]
    for (I, K), (ks, tiles) in {(14336, 4096): (1, 224), (11008, 4096): (1, 172), (4096, 4096): (4, 64),
                                (1024, 8192): (10, 16)}.items():
        for M, rt in ((1, 2), (33, 4), (64, 4), (128, 8)):
            p = by[(256, M, I, K)]
            assert p["cfg"] == [SWIGLU, 4, 1, ks, 2], (I, K, M)
            assert p["geo"] == [tiles * ks, 256, 2 * rt * 16 * 256 + 2048 + 64 + 16, tiles, K // 128,
                                -(-(K // 128) // ks), rt], p
    # K slices never put more workgroups on the chip than it has CUs
    for p in by.values():
        if p["rc"] == OK and p["cfg"][3] > 1:
            assert p["geo"][0] <= p["c"][0], p


def test_launch_geometry(lines):
    plans = [p for p in _plans(lines) if p["rc"] == OK]
    assert len(plans) > 300
    for p in plans:
        cus, M, I, K = p["c"]
        kernel, waves, depth, ksplit, strips = p["cfg"]
        grid, block, dyn, tiles, chunks, cps, row_tiles = p["geo"]
        assert (kernel, depth, strips) == (SWIGLU, 1, 2) and waves in (2, 4), p
        assert tiles * 16 * waves == I and chunks * 128 == K, p   # the column tiles cover I exactly
        assert grid == tiles * ksplit and block == 64 * waves, p
        assert 1 <= ksplit <= min(chunks, 16), p
        assert cps == -(-chunks // ksplit) and cps * ksplit >= chunks, p  # the last slices short or empty
        assert row_tiles in (2, 4, 6, 8) and row_tiles * 16 >= M > (row_tiles - 2) * 16, p
        assert dyn == 2 * row_tiles * 16 * 256 + 2 * 1024 + 64 + 16 and dyn % 16 == 0, p  # a second code2 table
        assert tiles * 4 <= 64 * 1024, p                           # one ticket per tile among the counters


def test_lds_within_160_kib_for_every_valid_cfg(lines):
    groups = [l for l in lines if l["k"] == "cfgs"]
    assert len(groups) == 36
    for g in groups:
        _, M, I, K = g["c"]
        assert g["valid"] == 2 * 2 * min(K // 128, 16), g   # waves {2, 4} x strips {0, 2} x K slices
        assert 0 < g["lds_max"] <= LDS_PER_CU, g
    assert max(g["lds_max"] for g in groups) == 2 * 128 * 256 + 2048 + 64 + 16  # 128 rows
    for p in _plans(lines):
        if p["rc"] == OK:
            assert p["geo"][2] <= LDS_PER_CU, p


def test_workspace_need_is_what_the_launcher_uses(lines):
    seen = set()
    for p in _plans(lines):
        if p["rc"] != OK:
            continue
        _, M, I, K = p["c"]
        ksplit = p["cfg"][3]
        want = HEADER + ksplit * 2 * M * I * 4 if ksplit > 1 else 0   # two fp32 planes per slice
        assert p["need"] == p["ws"] == want, p
        seen.add(ksplit > 1)
    assert seen == {True, False}


def test_a_named_cfg_is_taken_as_it_is(lines):
    """Every valid cfg of the family's grid comes back unchanged (strips 0 reads as 2)."""
    named = _plans(lines, named=1)
    assert len(named) > 250
    for p in named:
        assert p["rc"] == OK and p["cfg"][0] == SWIGLU and p["cfg"][4] == 2, p
