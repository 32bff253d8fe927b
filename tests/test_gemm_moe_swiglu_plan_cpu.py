"""The host plan of the fused expert SwiGLU launch (csrc/nf4_gemm_moe_swiglu_plan.h), checked without
a GPU: ``tests/plan/gemm_moe_swiglu_plan_check.cpp`` is built for the host as a stand-alone program
under AddressSanitizer + UBSan, as test_gemm_moe_plan_cpu.py builds its own, run, and every line
judged here.  Pinned: every validation code in both modes with the two-stack mismatches, the
library's choice and the launch geometry at Mixtral-8x7B's w1 / w3 for 1, 4, 16 and 64 tokens on
256 and 64 CUs, LDS within 160 KiB for every valid cfg, one ticket per (expert, column tile), that
the workspace the launcher asks for is what the size entry answers, and that a named cfg is
returned unchanged."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
MSG = 11
HEADER = 64 * 1024 + 256
LDS_PER_CU = 160 * 1024
MIXTRAL = (14336, 4096)  # (I, K) of w1 / w3; 8 experts


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("gemm_moe_swiglu_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "gemm_moe_swiglu_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "gemm_moe_swiglu_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def _plans(lines, named=None):
    return [l for l in lines if l["k"] == "plan" and (named is None or l["named"] == named)]


# rules of the call, tried in both modes (suffix _n nested, _s single)
CALL_RULES = ("ok", "arg_dtype", "arg_act", "arg_null_stacks", "arg_negative_p", "arg_null_x", "arg_null_ids", "arg_null_h",
              "arg_misaligned_x", "arg_misaligned_h", "arg_misaligned_ids", "arg_x_div_0", "ok_p0_nothing",
              "ok_p0_null_tensors", "shape_p129", "ok_p128", "ok_p1", "ok_x_div_beyond_p", "shape_i96", "shape_k1088",
              "shape_i0", "too_large_i", "ok_experts_256", "arg_no_workspace", "arg_misaligned_workspace",
              "arg_short_workspace", "ok_exact_workspace", "ok_one_slice_no_workspace", "arg_cfg_ksplit",
              "arg_cfg_expert_gemm", "arg_cfg_dense_swiglu", "ok_cfg_kernel_0", "too_large_tickets",
              "ok_one_slice_draws_no_ticket", "too_large_workspace", "ok_half_that_workspace")
# rules of a stack, tried on the gate stack (_g) and on the up stack (_u) in both modes
STACK_RULES = ("arg_null_packed", "arg_null_stats", "arg_misaligned_packed", "arg_misaligned_packed_stride",
               "arg_experts_0", "arg_experts_257", "arg_blocksize", "arg_negative_stride", "shape_blocksize_128",
               "shape_packed_stride", "ok_padded_packed_stride", "shape_short_stats", "shape_stacks_differ_in_n",
               "shape_stacks_differ_in_k", "shape_stacks_differ_in_experts", "shape_stacks_differ_in_single")
# rules of nested statistics, on either stack
NESTED_RULES = ("arg_null_a1", "arg_null_code2", "arg_blocksize2", "arg_misaligned_offset", "shape_short_nb",
                "shape_code2_stride", "ok_code2_stride", "ok_null_offset")


def test_validation_codes(lines):
    errs = {l["name"]: l for l in lines if l["k"] == "err"}
    want = {"arg_": ERR_ARG, "shape_": ERR_SHAPE, "too_large_": ERR_TOO_LARGE, "ok_": OK, "ok": OK}
    expected = ({f"{r}_{m}" for r in CALL_RULES for m in "ns"} | {f"{r}_{w}_{m}" for r in STACK_RULES for w in "gu" for m in "ns"}
                | {f"{r}_{w}" for r in NESTED_RULES for w in "gu"})
    assert set(errs) == expected, set(errs) ^ expected
    for name, l in errs.items():
        prefix = next(p for p in want if name.startswith(p))
        assert l["rc"] == want[prefix], (name, l)
        # only an accepted call with pairs launches; P == 0 is OK with nothing launched
        assert l["launch"] == (1 if prefix in ("ok_", "ok") and "_p0_" not in name else 0), (name, l)


def _resident(P):
    """Workgroups a CU holds at once: two with two row tiles (at most 32 pairs), one beyond."""
    return 2 if P <= 32 else 1


def _expected_choice(cus, P, E, I, K):
    """Four waves (64 columns of h: I % 64 == 0 always allows them); the expert GEMM's K-slice rule
    on this launch's column tiles, I / 64 per expert over the min(P, E) experts the plan assumes
    active: as many slices as keep active x tiles x slices within what the CUs hold at once, at
    most 16 and at most one per six 128-deep chunks."""
    tiles = I // 64 * min(P, E)
    return [MSG, 4, 1, max(1, min(cus * _resident(P) // tiles, 16, K // 128 // 6)), 2]


def test_library_choice_at_mixtrals_w1_w3(lines):
    by = {tuple(p["c"]): p for p in _plans(lines, named=0)}
    I, K = MIXTRAL
    for cus in (256, 64):
        for P in (2, 8, 32, 128):
            p = by[(cus, P, 8, I, K)]
            assert p["rc"] == OK and p["cfg"] == _expected_choice(cus, P, 8, I, K), p
            # spelled out: 224 column tiles per expert fill the chip from two active experts on
            assert p["cfg"] == [MSG, 4, 1, 1, 2] and p["need"] == p["ws"] == 0, p
            assert p["geo"][0] == 8 * 224 and p["geo"][3] == 224, p
    # the choice depends on (P, E, I, K, CUs) alone; on the small shapes it does split, and K slices
    # never put more working workgroups on the chip than it holds at once under the assumed spread
    split = 0
    for p in by.values():
        assert p["rc"] == OK and p["cfg"] == _expected_choice(*p["c"]), p
        if p["cfg"][3] > 1:
            cus, P, E = p["c"][:3]
            assert p["geo"][3] * min(P, E) * p["cfg"][3] <= cus * _resident(P), p
            split += 1
    assert split > 0


def test_launch_geometry(lines):
    plans = [p for p in _plans(lines) if p["rc"] == OK]
    assert len(plans) > 300
    for p in plans:
        cus, P, E, I, K = p["c"]
        kernel, waves, depth, ksplit, strips = p["cfg"]
        grid, block, dyn, tiles, chunks, cps, row_tiles, tickets = p["geo"]
        assert (kernel, depth, strips) == (MSG, 1, 2) and waves in (2, 4), p
        assert tiles * 16 * waves == I and chunks * 128 == K, p   # the column tiles cover I exactly
        assert tickets == E * tiles and grid == tickets * ksplit and block == 64 * waves, p
        assert 1 <= ksplit <= min(chunks, 16), p
        assert cps == -(-chunks // ksplit) and cps * ksplit >= chunks, p  # the last slices short or empty
        assert row_tiles in (2, 4, 6, 8) and row_tiles * 16 >= P > (row_tiles - 2) * 16, p  # one expert may get every pair
        assert dyn == 2 * row_tiles * 16 * 256 + 2048 + 64 + 16 + 1024 and dyn % 16 == 0, p
        assert ksplit == 1 or tickets * 4 <= 64 * 1024, p         # one ticket per (expert, tile) among the counters


def test_lds_within_160_kib_for_every_valid_cfg(lines):
    groups = [l for l in lines if l["k"] == "cfgs"]
    assert len(groups) == 42
    for g in groups:
        _, P, E, I, K = g["c"]
        assert g["valid"] == 2 * 2 * min(K // 128, 16), g   # waves {2, 4} x strips {0, 2} x K slices
        assert 0 < g["lds_max"] <= LDS_PER_CU, g
    assert max(g["lds_max"] for g in groups) == 2 * 8 * 16 * 256 + 2048 + 64 + 16 + 1024  # 128 pairs: eight row tiles
    for p in _plans(lines):
        if p["rc"] == OK:
            assert p["geo"][2] <= LDS_PER_CU, p


def test_workspace_need_is_what_the_launcher_uses(lines):
    seen = set()
    for p in _plans(lines):
        if p["rc"] != OK:
            continue
        _, P, E, I, K = p["c"]
        ksplit = p["cfg"][3]
        want = HEADER + ksplit * 2 * P * I * 4 if ksplit > 1 else 0   # two planes per slice, indexed by pair: E does not enter
        assert p["need"] == p["ws"] == want, p
        seen.add(ksplit > 1)
    assert seen == {True, False}


def test_a_named_cfg_is_taken_as_it_is(lines):
    """Every valid cfg of the family's grid comes back unchanged (strips 0 reads as 2)."""
    named = _plans(lines, named=1)
    assert len(named) > 250
    for p in named:
        assert p["rc"] == OK and p["cfg"][:4] == p["asked"][:4] and p["cfg"][0] == MSG, p
        assert p["asked"][4] in (0, 2) and p["cfg"][4] == 2, p
