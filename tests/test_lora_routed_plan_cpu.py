"""The host plan of the routed adapter launch (csrc/nf4_lora_routed_plan.h), checked without a GPU:
``tests/plan/lora_routed_plan_check.cpp`` is built for the host as a stand-alone program under
AddressSanitizer + UBSan, as test_lora_plan_cpu.py builds its own, run, and every line judged
here.  Pinned: every status code and the order of the rules (ARG before SHAPE before TOO_LARGE),
that a named cfg never falls back, the grid as (stack, slot < min(S, M), column tile), the kernel
instantiation (row tiles per block, r tiles), the LDS layout with the row list and that it
always fits, and the library's tile choice."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
OK, ERR_ARG, ERR_SHAPE, ERR_TOO_LARGE = 0, 1, 2, 3
LDS = 160 * 1024


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("lora_routed_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "lora_routed_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "lora_routed_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def test_status_codes_in_order(lines):
    errs = {l["name"]: l for l in lines if l["k"] == "err"}
    want = {"arg_": ERR_ARG, "shape_": ERR_SHAPE, "too_large_": ERR_TOO_LARGE, "ok_": OK}
    counts = dict.fromkeys(want, 0)
    for name, l in errs.items():
        prefix = next(p for p in want if name.startswith(p))
        assert l["rc"] == want[prefix], (name, l)
        counts[prefix] += 1
    assert counts == {"arg_": 29, "shape_": 24, "too_large_": 4, "ok_": 13}, counts
    for rule in ("arg_null_x", "arg_null_ids", "arg_null_stacks", "arg_dtype_f32", "arg_count_0", "arg_count_9",
                 "arg_adapters_0", "arg_adapters_65", "ok_adapters_64", "arg_null_A", "arg_null_B", "arg_null_scale",
                 "arg_null_y", "ok_null_base", "arg_r_4", "arg_r_136", "shape_r_12", "shape_n_120", "shape_m_0",
                 "shape_m_129", "shape_k_48", "shape_misaligned_x", "shape_misaligned_ids", "shape_misaligned_base",
                 "shape_a_stride_odd", "shape_b_stride_odd", "shape_a_stride_small", "shape_b_stride_small",
                 "shape_k_beyond_a_stride", "arg_r_before_shapes", "arg_adapters_before_shapes", "arg_cfg_before_shapes",
                 "shape_before_too_large", "shape_stride_before_too_large", "too_large_k", "too_large_n",
                 "too_large_a_stride", "too_large_b_stride", "arg_cfg_tile_48", "arg_cfg_waves_8"):
        assert rule in errs, rule


def _plans(lines, named=None):
    return [l for l in lines if l["k"] == "plan" and (named is None or l["named"] == named)]


def test_every_listed_cfg_is_admitted_and_geometry_is_as_documented(lines):
    plans = _plans(lines)
    assert len(plans) > 15000 and all(p["rc"] == OK for p in plans)
    assert {tuple(p["cfg"]) for p in _plans(lines, named=1)} == {(t, w) for t in (16, 32, 64, 128, 256) for w in (1, 2, 4)}
    seen_mb, seen_rt, seen_slots = set(), set(), set()
    for p in plans:
        _, M, K, S = p["c"]
        tile_n, waves = p["cfg"]
        grid, block, dyn, slots, mb, rt, m_pad, ts, t_bytes, part_bytes, list_bytes = p["geo"]
        assert slots == min(S, M)
        tiles = [slots * -(-n // tile_n) for n in p["N"]]        # (stack, slot, tile): slots * tiles blocks per stack
        assert p["tile0"] == [sum(tiles[:i]) for i in range(len(tiles) + 1)] and grid == sum(tiles), p
        assert block == 64 * waves
        r_max = max(p["r"])
        assert mb == (1 if M <= 16 else 2) and rt == next(v for v in (1, 2, 4, 8) if 16 * v >= r_max), p
        assert m_pad == -(-M // (16 * mb)) * 16 * mb and M <= m_pad < M + 16 * mb  # one adapter may own every row
        assert ts == -(-r_max // 32) * 32 + 8 and (2 * ts) % 16 == 0          # 16-byte rows, off the bank stride
        assert t_bytes == m_pad * ts * 2 and t_bytes % 16 == 0
        assert part_bytes == waves * 16 * mb * (16 * rt + 4) * 4 and part_bytes % 16 == 0
        assert list_bytes == 4 * m_pad                                        # one 32-bit entry per row of t
        assert dyn == t_bytes + part_bytes + list_bytes <= LDS, p
        seen_mb.add(mb)
        seen_rt.add(rt)
        seen_slots.add(slots)
    assert seen_mb == {1, 2} and seen_rt == {1, 2, 4, 8} and {1, 3, 5, 8, 16, 17, 64} <= seen_slots
    assert max(p["geo"][2] for p in plans) == 128 * 136 * 2 + 4 * 32 * 132 * 4 + 128 * 4


def test_the_librarys_choice(lines):
    for p in _plans(lines, named=0):
        cus, M, _, S = p["c"]
        n_sum = sum(p["N"])
        want = next((t for t in (64, 128, 256) if min(S, M) * -(-n_sum // t) <= cus), 256)
        assert p["cfg"] == [want, 4], p
    # spelled out on the 256 CUs of an MI355X
    by = {(p["c"][0], p["c"][1], p["c"][2], p["c"][3], tuple(p["N"])): p for p in _plans(lines, named=0)}
    one = by[(256, 1, 4096, 64, (4096,))]                 # one decode row: one adapter's worth of workgroups, not 64
    assert one["cfg"] == [64, 4] and one["geo"][0] == 64 and one["geo"][3] == 1
    assert by[(256, 64, 4096, 3, (4096,))]["cfg"] == [64, 4] and by[(256, 64, 4096, 3, (4096,))]["geo"][0] == 192
    assert by[(256, 64, 4096, 8, (4096,))]["cfg"] == [128, 4] and by[(256, 64, 4096, 8, (4096,))]["geo"][0] == 256
    assert by[(256, 64, 4096, 64, (4096,))]["cfg"] == [256, 4] and by[(256, 64, 4096, 64, (4096,))]["geo"][0] == 1024
    assert by[(256, 5, 4096, 8, (14336,))]["cfg"] == [256, 4] and by[(256, 5, 4096, 8, (14336,))]["geo"][0] == 5 * 56
