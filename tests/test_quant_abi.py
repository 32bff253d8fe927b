"""The quantizer's C entries (include/nf4_dequant.h): declared, bound, and rejecting bad
arguments on the host before any device work (no GPU needed; pointers are never read)."""
import os
import re

import pytest

from nf4_triton_dequantization_amd import _lib

import _quant_cases as Q

FAKE = 0x1000  # 16-byte aligned, never dereferenced: every call below ends in validation
NEW = ("nf4_quant_workspace_bytes", "nf4_quant_bnb", "nf4_quant_bnb_nested", "nf4_quant_bnb_cpu",
       "nf4_quant_bnb_nested_cpu")
BLOCKSIZES = (64, 128, 256, 512, 1024, 2048, 4096)


def test_entries_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name


def test_workspace_bytes():
    L = _lib.lib()
    for bs in BLOCKSIZES:
        for numel in (1, 63, 64 * 257, 1 << 24):
            nblk = -(-numel // bs)
            got = L.nf4_quant_workspace_bytes(numel, bs)
            assert got >= 4 * nblk + 8 and got % 8 == 0, (numel, bs, got)   # fp32 absmax + partial sums
            assert got <= 4 * nblk + 16 * 1024, (numel, bs, got)            # and little more
    assert L.nf4_quant_workspace_bytes(0, 64) == 0
    assert L.nf4_quant_workspace_bytes(-5, 64) == 0
    assert L.nf4_quant_workspace_bytes(1024, 96) == 0


def _single(L, cpu, w=FAKE, dt=_lib.BF16, numel=1024, bs=64, packed=FAKE, absmax=FAKE):
    fn = L.nf4_quant_bnb_cpu if cpu else L.nf4_quant_bnb
    return fn(w, dt, numel, bs, packed, absmax, 1 if cpu else None)


def _nested(L, cpu, w=FAKE, dt=_lib.BF16, numel=1024, bs=64, code2=FAKE, bs2=256, packed=FAKE, aq=FAKE, a2=FAKE,
            off=FAKE, ws=FAKE, wsz=None):
    if cpu:
        return L.nf4_quant_bnb_nested_cpu(w, dt, numel, bs, code2, bs2, packed, aq, a2, off, 1)
    if wsz is None:
        wsz = L.nf4_quant_workspace_bytes(numel, bs) if numel > 0 and bs in BLOCKSIZES else 1 << 20
    return L.nf4_quant_bnb_nested(w, dt, numel, bs, code2, bs2, packed, aq, a2, off, ws, wsz, None)


@pytest.mark.parametrize("cpu", [False, True], ids=["hip", "cpu"])
def test_single_validation(cpu):
    L = _lib.lib()
    assert _single(L, cpu, dt=7) == _lib.ERR_ARG                 # bad dtype
    assert _single(L, cpu, dt=-1) == _lib.ERR_ARG
    assert _single(L, cpu, numel=-1) == _lib.ERR_ARG             # negative size
    for bs in (0, 1, 32, 96, 8192, -64):                         # not a supported power of two
        assert _single(L, cpu, bs=bs) == _lib.ERR_ARG, bs
    assert _single(L, cpu, w=None) == _lib.ERR_ARG               # null pointers
    assert _single(L, cpu, packed=None) == _lib.ERR_ARG
    assert _single(L, cpu, absmax=None) == _lib.ERR_ARG
    # nothing to do, nothing launched (pointers may be null); a bad dtype is still an error
    assert _single(L, cpu, w=None, numel=0, packed=None, absmax=None) == _lib.OK
    assert _single(L, cpu, w=None, dt=9, numel=0, packed=None, absmax=None) == _lib.ERR_ARG


@pytest.mark.parametrize("cpu", [False, True], ids=["hip", "cpu"])
def test_nested_validation(cpu):
    L = _lib.lib()
    assert _nested(L, cpu, dt=3) == _lib.ERR_ARG
    assert _nested(L, cpu, numel=-7) == _lib.ERR_ARG
    for bs in (0, 48, 32, 8192):
        assert _nested(L, cpu, bs=bs) == _lib.ERR_ARG, bs
    for bs2 in (0, 64, 128, 255, 512, -256):                     # bitsandbytes' only value is 256
        assert _nested(L, cpu, bs2=bs2) == _lib.ERR_ARG, bs2
    for name in ("w", "code2", "packed", "aq", "a2", "off"):
        assert _nested(L, cpu, **{name: None}) == _lib.ERR_ARG, name
    assert _nested(L, cpu, w=None, numel=0, code2=None, packed=None, aq=None, a2=None, off=None, ws=None,
                   wsz=0) == _lib.OK
    assert _nested(L, cpu, numel=0, bs2=128) == _lib.ERR_ARG
    if not cpu:
        need = L.nf4_quant_workspace_bytes(1024, 64)
        assert _nested(L, cpu, ws=None) == _lib.ERR_ARG
        assert _nested(L, cpu, wsz=need - 1) == _lib.ERR_ARG     # a workspace that is too small
        assert _nested(L, cpu, wsz=0) == _lib.ERR_ARG
        assert _nested(L, cpu, ws=FAKE + 4) == _lib.ERR_ARG      # not 8-byte aligned


def test_misaligned_pointers_rejected():
    """An input not aligned to its own element, or an fp32 output not to 4 bytes, cannot be a
    tensor of that type: refused, never handed to a kernel."""
    L = _lib.lib()
    assert _single(L, False, w=FAKE + 1) == _lib.ERR_ARG
    assert _single(L, False, w=FAKE + 2, dt=_lib.F32) == _lib.ERR_ARG
    assert _single(L, False, absmax=FAKE + 2) == _lib.ERR_ARG


def test_case_sizes_use_the_kernel_constants():
    """tests/_quant_cases.py takes its tile and workgroup sizes from csrc/nf4_quant.hip."""
    src = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "nf4_triton_dequantization_amd", "csrc",
                            "nf4_quant.hip")).read()
    lane = int(re.search(r"constexpr int kQLane = (\d+);", src).group(1))
    wg = int(re.search(r"constexpr int kQWg = (\d+);", src).group(1))
    assert Q.LANE_ELEMS == lane and Q.TILE == 64 * lane and Q.WG_ELEMS == wg * lane
    assert "kQTile = 64 * kQLane" in src and "kQWaves = kQWg / 64" in src


def test_python_entry_is_lazy_and_loud():
    """Importing quantize loads no native code; a host tensor raises unless NF4_BACKEND=cpu;
    a missing library raises on the first call."""
    import subprocess
    import sys

    code = (
        "import torch\n"
        "from nf4_triton_dequantization_amd import nf4_quantize, _lib\n"
        "assert _lib._lib is None\n"
        "try:\n"
        "    nf4_quantize(torch.randn(4, 64))\n"
        "except RuntimeError as e:\n"
        "    assert 'ROCm device' in str(e), e\n"
        "    print('raised')\n"
    )
    env = dict(os.environ)
    env.pop("NF4_BACKEND", None)
    cwd = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=cwd)
    assert r.returncode == 0 and r.stdout.strip() == "raised", r.stderr
    code = (
        "import torch\n"
        "from nf4_triton_dequantization_amd import nf4_quantize\n"
        "try:\n"
        "    nf4_quantize(torch.randn(4, 64))\n"
        "except RuntimeError as e:\n"
        "    assert 'not built' in str(e), e\n"
        "    print('raised')\n"
    )
    env.update(NF4_BACKEND="cpu", NF4DQ_LIB_PATH="/nonexistent/libnf4dq.so")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=cwd)
    assert r.returncode == 0 and r.stdout.strip() == "raised", r.stderr
