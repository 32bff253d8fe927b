"""The host plan of the expert GEMM in row blocks (csrc/nf4_gemm_moe_rb_plan.h), checked without
a GPU: ``tests/plan/gemm_moe_rb_plan_check.cpp`` is built for the host as a stand-alone program
under AddressSanitizer + UBSan, as test_gemm_moe_plan_cpu.py builds its own, run, and every line
judged here.  Pinned: every validation code in nf4_gemm_bnb_moe's order with this entry's pair
bound (1024), a cfg naming NF4DQ_GEMM_MOE is ERR_ARG, grid = experts x column tiles x K slices x
ceil(P / 128) row blocks, one ticket per (expert, column tile, row block) within the header, LDS
equal to the expert GEMM's at min(P, 128) pairs and within 160 KiB for every valid cfg, the
workspace the launcher asks for is what the size entry answers, and the library's K slices at
Mixtral's two shapes."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
MOE_RB = 13
HEADER = 64 * 1024 + 256
LDS_PER_CU = 160 * 1024
MIXTRAL = [(14336, 4096), (4096, 14336)]  # (N, K); 8 experts


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("gemm_moe_rb_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_moe_rb_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_moe_rb_plan_check.cpp")]
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
    assert counts == {"arg_": 2 * 25 + 3, "shape_": 2 * 7 + 2, "too_large_": 2 * 5, "ok_": 2 * 17 + 2}, counts
    for rule in ("ok_p0_nothing_", "ok_p0_null_tensors_", "shape_p1025_", "ok_p1024_", "ok_p129_", "ok_p128_", "ok_p1_",
                 "shape_n96_", "shape_k1088_", "shape_packed_stride_", "shape_short_stats_", "shape_blocksize_128_",
                 "arg_x_div_0_", "arg_experts_0_", "arg_experts_257_", "arg_misaligned_packed_stride_",
                 "arg_no_workspace_", "arg_cfg_ksplit_", "arg_cfg_other_family_", "arg_cfg_moe_",
                 "arg_cfg_moe_64_pairs_", "too_large_tickets_5_blocks_", "too_large_tickets_1_block_",
                 "ok_tickets_3_blocks_", "too_large_n_", "too_large_x_", "too_large_slab_", "ok_slab_below_4g_"):
        assert rule + "n_" in errs and rule + "s_" in errs, rule
    for rule in ("arg_null_a1", "arg_null_code2", "arg_blocksize2", "shape_short_nb", "shape_code2_stride"):
        assert rule in errs, rule


def _expected_choice(cus, P, E, N, K):
    """128-column workgroups where N allows; the row-tiled family's K-slice rule on the grid the
    plan assumes working: min(P, E) experts active, each with ceil(share / 128) live row blocks,
    against one resident workgroup a CU beyond 128 pairs (two up to 32 pairs, as nf4_gemm_bnb_moe):
    as many slices as keep that grid within the CUs, at most 16 and one per six 128-deep chunks."""
    waves = 4 if N % 128 == 0 else 2
    active = min(P, E)
    live = -(-(-(-P // active)) // 128)
    resident = 2 if P <= 32 else 1
    tiles = N // (32 * waves) * active * live
    return [MOE_RB, waves, 1, max(1, min(cus * resident // tiles, 16, K // 128 // 6)), 2]


def test_library_choice(lines):
    by = {tuple(p["c"]): p for p in _plans(lines, named=0)}
    for p in by.values():
        assert p["rc"] == OK and p["cfg"] == _expected_choice(*p["c"]), p
    # Mixtral's two shapes on the 256 CUs of an MI355X (and on 64): one K slice from 130 pairs on --
    # the assumed grid alone fills the CUs, and a slice's slab is P * N floats (58 MB at 1024 x 14336)
    for cus in (256, 64):
        for N, K in MIXTRAL:
            for P in (130, 256, 512, 1024):
                p = by[(cus, P, 8, N, K)]
                assert p["cfg"] == [MOE_RB, 4, 1, 1, 2] and p["ws"] == 0, p
    # up to 128 pairs the choice is nf4_gemm_bnb_moe's own (test_gemm_moe_plan_cpu.py spells these)
    spelled = {(2, 14336, 4096): 2, (8, 14336, 4096): 1, (32, 14336, 4096): 1, (128, 14336, 4096): 1,
               (2, 4096, 14336): 8, (8, 4096, 14336): 2, (32, 4096, 14336): 2, (128, 4096, 14336): 1}
    for (P, N, K), ks in spelled.items():
        assert by[(256, P, 8, N, K)]["cfg"] == [MOE_RB, 4, 1, ks, 2], (P, N, K)
    # K is split only where the assumed working grid leaves CUs idle, and never beyond them
    split = [p for p in by.values() if p["cfg"][3] > 1]
    assert any(p["c"][1] > 128 for p in split)
    for p in by.values():
        cus, P, E, N, K = p["c"]
        active = min(P, E)
        working = p["geo"][3] * active * -(-(-(-P // active)) // 128)
        if p["cfg"][3] > 1:
            assert working * p["cfg"][3] <= cus * (2 if P <= 32 else 1), p
        elif working >= cus:
            assert p["cfg"][3] == 1 and p["ws"] == 0, p


def test_launch_geometry(lines):
    plans = [p for p in _plans(lines) if p["rc"] == OK]
    assert len(plans) > 300
    blocks = set()
    for p in plans:
        cus, P, E, N, K = p["c"]
        kernel, waves, depth, ksplit, strips = p["cfg"]
        grid, block, dyn, tiles, chunks, cps, row_tiles, tickets, row_blocks = p["geo"]
        assert (kernel, depth, strips) == (MOE_RB, 1, 2) and waves in (2, 4), p
        assert tiles * 32 * waves == N and chunks * 128 == K, p   # the column tiles cover N exactly
        assert row_blocks == -(-P // 128), p
        assert tickets == E * tiles * row_blocks and grid == tickets * ksplit and block == 64 * waves, p
        assert 1 <= ksplit <= min(chunks, 16), p
        assert cps == -(-chunks // ksplit) and cps * ksplit >= chunks, p  # the last slices short or empty
        rows = min(P, 128)                                         # what one workgroup may stage
        assert row_tiles in (2, 4, 6, 8) and row_tiles * 16 >= rows > (row_tiles - 2) * 16, p
        assert P <= 128 or row_tiles == 8, p
        assert dyn == p["lds"] == 2 * row_tiles * 16 * 256 + 1024 + 64 + 16 + 2 * 4 * 128 and dyn % 16 == 0, p
        assert ksplit == 1 or tickets * 4 <= 64 * 1024, p         # the tickets among the counters
        blocks.add(row_blocks)
    assert blocks == {1, 2, 3, 4, 8}


def test_lds_within_160_kib_for_every_valid_cfg(lines):
    groups = [l for l in lines if l["k"] == "cfgs"]
    assert len(groups) == 45
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
        want = HEADER + ksplit * P * N * 4 if ksplit > 1 else 0   # slabs indexed by pair: E and the row blocks do not enter
        assert p["need"] == p["ws"] == want, p
        seen.add((ksplit > 1, P > 128))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


def test_a_named_cfg_is_taken_as_it_is(lines):
    """Every valid cfg of the family's grid comes back unchanged (strips 0 reads as 2)."""
    named = _plans(lines, named=1)
    assert len(named) > 250
    for p in named:
        assert p["rc"] == OK and p["cfg"][0] == MOE_RB and p["cfg"][4] == 2, p
