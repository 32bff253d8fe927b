"""The dequant library's host plan, pinned without a GPU.  ``csrc/nf4_dequant_plan.h`` is
plain C++: every entry point's validation, and for every launch of a call the kernel family,
its template parameters, grid, block and argument image.  ``tests/plan/dequant_plan_check.cpp``
prints all of it for a fixed list of cases; this builds it for the host under
AddressSanitizer + UBSan, runs it and compares line by line with
``tests/plan/dequant_plan_snapshot.jsonl`` (recorded from the dispatch as it stood when it
was moved out of nf4_dequant.hip, before it was restructured: a change of any line is a
change of a kernel choice, a launch shape or a kernel argument).  The tables of the GPU
tests name the kernel form each of their cases is there for; the last two tests hold the
plan to those names."""
from __future__ import annotations

import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-g"]
FLAT1, FLAT, DENSE, PIECE, PIECE32, CHUNK, ROWS, BNB_BYTES = range(8)
F16, BF16, F32 = 0, 1, 2
BATCH_MAX = 24


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    tmp = tmp_path_factory.mktemp("dqplan")
    # the sanitizer runtimes first, on a program of one line: only their absence skips;
    # a failure to build the check program itself is a failure
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *SAN, "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer runtime unavailable: {r.stderr[-300:]}")
    exe = tmp / "dequant_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *SAN, "-o", str(exe),
           os.path.join(REPO, "tests", "plan", "dequant_plan_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"build failed: {' '.join(cmd)}\n{r.stderr[-2000:]}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rc={r.returncode}\nstderr={r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def cases(plan_lines):
    return [json.loads(l) for l in plan_lines]


def test_plan_matches_the_snapshot(plan_lines):
    with open(os.path.join(REPO, "tests", "plan", "dequant_plan_snapshot.jsonl")) as f:
        want = f.read().splitlines()
    assert len(plan_lines) == len(want)
    differ = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, plan_lines)) if w != g]
    assert not differ, f"{len(differ)} lines differ; first (line, snapshot, now): {differ[0]}"


def test_plan_properties(cases):
    assert len(cases) > 700
    families, chunk_forms, piece_forms, piece32_forms = set(), set(), set(), set()
    segmented = flushed = 0
    for c in cases:
        dt = c["c"][3]
        if c["rc"] != 0:
            assert not c["l"], c  # everything is validated before anything is launched
        tile = 512 if dt == F32 else 1024  # packed bytes of a wave's tile
        obpp = 8 if dt == F32 else 4       # output bytes per packed byte
        cover = {}                         # matrix -> packed bytes its segments have covered so far
        for l in c["l"]:
            fam, ldt, _mode, p0, p1, grid, block, count = l["k"]
            families.add(fam)
            assert ldt == dt and 1 <= grid < 2 ** 31 and block == 256, c
            if fam == CHUNK:
                chunk_forms.add((p0, p1))
            elif fam == PIECE:
                piece_forms.add((p0, p1))
            elif fam == PIECE32:
                piece32_forms.add((p0, p1))
            if fam not in (FLAT1, FLAT):
                assert count == 1, c
                continue
            ds = l["d"]
            assert len(ds) == count and 1 <= count <= p0 and p0 in (1, BATCH_MAX), c
            assert fam == FLAT or p0 == 1, c
            tiles = 0
            for poff, ooff, nbytes, blk_base, tile_begin, blk_shift, _b2, _g, _nb, _n2, _bpr in ds:
                mat, at = poff >> 38, poff & (2 ** 38 - 1)
                # segments tile the matrix in order: no gap, no overlap, packed and output alike
                assert at == cover.get(mat, 0) and ooff == (mat << 40) + at * obpp, c
                assert 0 < nbytes < 2 ** 29 and nbytes % 4 == 0, c
                assert blk_base == at >> blk_shift and at % (1 << blk_shift) == 0, c
                assert tile_begin == tiles, c
                cover[mat] = at + nbytes
                tiles += -(-nbytes // tile)
            assert l["t"] == tiles, c
            if fam == FLAT1 or c["c"][2] != 1:  # (only nf4_dequant_ref_cfg caps a grid)
                assert grid == -(-tiles // 4), c
            else:
                assert grid <= -(-tiles // 4), c
        # a matrix on the flat path is covered exactly once (the error group gives no sizes)
        for mat, end in cover.items():
            assert c["c"][0] == 8 or end == c["pl"][mat], c
        flat_launches = [l for l in c["l"] if l["k"][0] in (FLAT1, FLAT)]
        segmented += any(pl >= 2 ** 29 and m in cover for m, pl in enumerate(c["pl"]))
        flushed += len(flat_launches) > 1
    assert segmented >= 30 and flushed >= 12  # the large-matrix split and its mid-walk flush are exercised
    # every family and every form in the code object is some case's choice
    assert families == set(range(8)), families
    assert chunk_forms == {(4, 16), (4, 4), (1, 16), (1, 4)}, chunk_forms
    both = {(re, tri) for re in (0, 1, 2) for tri in (0, 1)}
    assert piece_forms == both and piece32_forms == both, (piece_forms, piece32_forms)


def _form(launches):
    assert len(launches) == 1, launches
    fam, _dt, _mode, p0, p1 = launches[0]["k"][:5]
    return {DENSE: "dense", PIECE: "piece", PIECE32: "piece32", CHUNK: f"chunk{p0}.{p1}", ROWS: "rows",
            FLAT1: "flat1", FLAT: "flat"}[fam]


def test_chunk_cases_take_the_form_their_table_names(cases):
    """tests/test_gpu_chunks.py CASES: the plan sends each row, in both scale modes, to the form
    the row names for 16-bit and for fp32 output."""
    import test_gpu_chunks as T

    got = [c for c in cases if c["c"][0] == 3]
    assert len(got) == len(T.CASES) * 3 * 2
    for c in got:
        _, idx, _entry, dt, m, n, pad, pb, obytes = c["c"][:9]
        row = T.CASES[idx]
        assert (m, n, pad, pb, obytes) == (*row[:4], row[4] * (4 if dt == F32 else 2)), (c["c"], row)
        assert c["rc"] == 0 and _form(c["l"]) == (row[6] if dt == F32 else row[5]), (c["c"], row)


def test_edge_forms_take_the_kernel_their_table_names(cases):
    """tests/test_gpu_edges.py FORMS: the kernel kind of each entry for the dtypes it runs, and
    for the chunk-kernel entries whose name says so, the load and store form."""
    import test_gpu_edges as T

    names = sorted(T.FORMS)
    got = [c for c in cases if c["c"][0] == 4]
    assert len(got) == len(names) * 3 * 2
    dts = {"f16": F16, "bf16": BF16, "f32": F32}
    for c in got:
        _, idx, _entry, dt, _m, n, pad, pb, obytes = c["c"][:9]
        name = names[idx]
        fn, fpad, fpoff, fooff, fdts, kind = T.FORMS[name]
        assert (n, pad, pb, obytes) == (fn, fpad, fpoff, fooff * (4 if dt == F32 else 2)), (c["c"], name)
        if dt not in [dts[d] for d in fdts]:
            continue
        form = _form(c["l"])
        assert c["rc"] == 0 and (form if kind != "chunk" else form[:5].replace("dense", "chunk")) == kind, (c["c"], name)
        if name == "dense":
            assert form == "dense"
        for word, want in (("dword", "chunk4."), ("alignbyte", "chunk1."), ("_whole", ".16"), ("_staged", ".4")):
            if word in name:
                assert form.startswith(want) or form.endswith(want), (name, form)
