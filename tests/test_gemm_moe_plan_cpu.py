"""The host plan of the fused expert GEMM (csrc/nf4_gemm_moe_plan.h), checked without a GPU:
``tests/plan/gemm_moe_plan_check.cpp`` is built for the host as a stand-alone program under
AddressSanitizer + UBSan, as test_gemm_mt_plan_cpu.py builds its own, run, and every line judged
here.  Pinned: every validation code, the library's choice and the launch geometry at the
Mixtral-8x7B shapes for 1, 4, 16 and 64 tokens, LDS within 160 KiB for every valid cfg, one ticket
per (expert, column tile) within the header, and that the workspace the launcher asks for is
what the size entry answers."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
MOE = 9
HEADER = 64 * 1024 + 256
LDS_PER_CU = 160 * 1024
MIXTRAL = [(14336, 4096), (4096, 14336)]  # (N, K); 8 experts


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("gemm_moe_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_moe_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_moe_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def _plans(lines, named=None):
    return [l for l in lines if l["k"] == "plan" and (named is None or l["named"] == named)]


def test_validation_codes(lines):
    errs = {l["name"]: l for l in lines if l["k"] == "err"}
    want = {"arg_": ERR_ARG, "shape_": ERR_SHAPE, "too_large_": ERR_TOO_LARGE, "ok_": OK}
    counts = dict.fromkeys(want, 0)
    for name, l in errs.items():
        prefix = next(p for p in want if name.startswith(p))
        assert l["rc"] == want[prefix], (name, l)
        # only an accepted call with pairs launches; P == 0 is OK with nothing launched
        assert l["launch"] == (1 if prefix == "ok_" and "_p0_" not in name else 0), (name, l)
        counts[prefix] += 1
    assert counts == {"arg_": 2 * 23 + 3, "shape_": 2 * 7 + 2, "too_large_": 4, "ok_": 2 * 12 + 2}, counts
    for rule in ("ok_p0_nothing_", "ok_p0_null_tensors_", "shape_p129_", "shape_n96_", "shape_k1088_",
                 "shape_packed_stride_", "shape_short_stats_", "shape_blocksize_128_", "arg_x_div_0_",
                 "arg_experts_0_", "arg_experts_257_", "arg_misaligned_packed_stride_", "arg_no_workspace_",
                 "arg_cfg_ksplit_", "arg_cfg_other_family_", "too_large_tickets_", "too_large_n_"):
        assert rule + "n_" in errs and rule + "s_" in errs, rule
    for rule in ("arg_null_a1", "arg_null_code2", "arg_blocksize2", "shape_short_nb", "shape_code2_stride"):
        assert rule in errs, rule


def _resident(P):
    """Workgroups a CU holds at once: two with two row tiles (at most 32 pairs), one beyond."""
    return 2 if P <= 32 else 1


def _expected_choice(cus, P, E, N, K):
    """128-column workgroups where N allows; the row-tiled family's K-slice rule on the grid of
    the experts the plan assumes active, min(P, E): as many slices as keep active x tiles x
    slices within what the CUs hold at once, at most 16 and at most one per six 128-deep chunks."""
    waves = 4 if N % 128 == 0 else 2
    tiles = N // (32 * waves) * min(P, E)
    return [MOE, waves, 1, max(1, min(cus * _resident(P) // tiles, 16, K // 128 // 6)), 2]


def test_library_choice_at_the_mixtral_shapes(lines):
    by = {tuple(p["c"]): p for p in _plans(lines, named=0)}
    for cus in (256, 64):
        for N, K in MIXTRAL:
            for P in (2, 8, 32, 128):
                p = by[(cus, P, 8, N, K)]
                assert p["rc"] == OK and p["cfg"] == _expected_choice(cus, P, 8, N, K), p
    # spelled out for the 256 CUs of an MI355X: K slices at 1, 4, 16 and 64 tokens (top-2)
    spelled = {(2, 14336, 4096): 2, (8, 14336, 4096): 1, (32, 14336, 4096): 1, (128, 14336, 4096): 1,
               (2, 4096, 14336): 8, (8, 4096, 14336): 2, (32, 4096, 14336): 2, (128, 4096, 14336): 1}
    for (P, N, K), ks in spelled.items():
        assert by[(256, P, 8, N, K)]["cfg"] == [MOE, 4, 1, ks, 2], (P, N, K)
    # the choice depends on (P, E, N, K, CUs) alone and K slices never put more working
    # workgroups on the chip than it holds at once under the assumed spread
    for p in by.values():
        if p["rc"] == OK and p["cfg"][3] > 1:
            cus, P, E = p["c"][:3]
            assert p["geo"][3] * min(P, E) * p["cfg"][3] <= cus * _resident(P), p


def test_launch_geometry(lines):
    plans = [p for p in _plans(lines) if p["rc"] == OK]
    assert len(plans) > 300
    for p in plans:
        cus, P, E, N, K = p["c"]
        kernel, waves, depth, ksplit, strips = p["cfg"]
        grid, block, dyn, tiles, chunks, cps, row_tiles, tickets = p["geo"]
        assert (kernel, depth, strips) == (MOE, 1, 2) and waves in (2, 4), p
        assert tiles * 32 * waves == N and chunks * 128 == K, p   # the column tiles cover N exactly
        assert tickets == E * tiles and grid == tickets * ksplit and block == 64 * waves, p
        assert 1 <= ksplit <= min(chunks, 16), p
        assert cps == -(-chunks // ksplit) and cps * ksplit >= chunks, p  # the last slices short or empty
        assert row_tiles in (2, 4, 6, 8) and row_tiles * 16 >= P > (row_tiles - 2) * 16, p  # one expert may get every pair
        assert dyn == 2 * row_tiles * 16 * 256 + 1024 + 64 + 16 + 2 * 4 * 128 and dyn % 16 == 0, p
        assert ksplit == 1 or tickets * 4 <= 64 * 1024, p         # one ticket per (expert, tile) among the counters


def test_lds_within_160_kib_for_every_valid_cfg(lines):
    groups = [l for l in lines if l["k"] == "cfgs"]
    assert len(groups) == 42
    for g in groups:
        _, P, E, N, K = g["c"]
        widths = 1 + (N % 128 == 0)
        assert g["valid"] == widths * 2 * min(K // 128, 16), g   # waves 2 (and 4) x strips {0, 2} x K slices
        assert 0 < g["lds_max"] <= LDS_PER_CU, g
    for p in _plans(lines):
        if p["rc"] == OK:
            assert p["geo"][2] <= LDS_PER_CU, p


def test_workspace_need_is_what_the_launcher_uses(lines):
    seen = set()
    for p in _plans(lines):
        if p["rc"] != OK:
            continue
        _, P, E, N, K = p["c"]
        ksplit = p["cfg"][3]
        want = HEADER + ksplit * P * N * 4 if ksplit > 1 else 0   # slabs indexed by pair: E does not enter
        assert p["need"] == p["ws"] == want, p
        seen.add(ksplit > 1)
    assert seen == {True, False}


def test_a_named_cfg_is_taken_as_it_is(lines):
    """Every valid cfg of the family's grid comes back unchanged (strips 0 reads as 2)."""
    named = _plans(lines, named=1)
    assert len(named) > 250
    for p in named:
        assert p["rc"] == OK and p["cfg"][0] == MOE and p["cfg"][4] == 2, p
