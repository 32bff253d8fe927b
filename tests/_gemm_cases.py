"""Inputs, comparisons and configuration lists shared by the fused-GEMM suites
(test_gpu_gemm.py, test_gpu_gemm_exact.py, test_gpu_redzones.py, test_gpu_strided.py,
test_gpu_parity.py; test_gemm_cases_cpu.py checks this module itself on the host).

Three things live here.

* The float64 oracle's helpers (``bits_to_f64``, ``tol``, ``x_bits``) and ``check_close``:
  the comparison fails wherever ``abs(got - ref) <= tol`` is NOT true, so a NaN output (the
  split-K hand-off writes NaN when a reduction gives up) and an inf against a finite
  reference fail; ``abs(got - ref) > tol`` would let both through.

* ``gemm_cfgs``: every decomposition of every kernel family the tuning ABI may accept
  (invalid ones answer ERR_ARG and are skipped by the callers).

* The sensitive weights.  Every GEMM kernel multiplies x by the weights nf4_dequant_ref
  would write,

      w = RNE16(fp32(NF4[c] * fp32(fp32(q / 127) * a2))),

  and a float64 product inside the GEMM tolerance cannot tell that from a weight one
  16-bit ulp off.  ``sensitive_weight`` builds a real (packed, a1, a2) double-quant weight
  whose 64-blocks are filled with triples (q, a2, c) at which a near-miss restatement gives
  a different 16-bit value:

      single rounding    RNE16(NF4[c] * s)  with the product exact (one rounding, not two)
      reciprocal scale   q * fp32(1 / 127)  in place of q / 127
      reordered scale    (q * a2) / 127     in place of (q / 127) * a2

  Such triples are rare among random draws (a genuine bf16 single-rounding case about 7
  times per million), so the search is directed: the last product must land next to a
  16-bit rounding boundary, so a2 is solved for from a drawn boundary and its fp32
  neighbours are tried.  Everything is judged by evaluating the reference formula and the
  restatements; the aiming only makes hits frequent.
"""
from __future__ import annotations

import functools

import numpy as np

import nf4_oracle as O

KINDS = ("single_rounding", "reciprocal_scale", "reordered_scale")
_PREC = {"bf16": (8, -133), "f16": (11, -24)}  # significant bits, exponent of the subnormal spacing
_F127 = np.float32(127.0)
_R127 = np.float32(1.0) / _F127


# ---------------------------------------------------------------------------------------------
# float64 oracle and comparison
# ---------------------------------------------------------------------------------------------
def bits_to_f64(bits, dt):
    if dt == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def tol(ref, mag, dt):
    p, sub = (8, 2.0 ** -134) if dt == "bf16" else (10, 2.0 ** -25)
    return 2.0 ** -p * np.abs(ref) + 2.0 ** -20 * mag + sub


def x_bits(M, K, dt, seed):
    import torch

    x = O.normal_f32(seed, M * K, stream=9).reshape(M, K)
    t = torch.from_numpy(x).to(torch.float16 if dt == "f16" else torch.bfloat16)
    return t, t.view(torch.int16).numpy().view(np.uint16)


def check_close(got, ref, tol, what=""):
    """Fail on every element where ``abs(got - ref) <= tol`` is not true (NaN and +-inf
    outputs included); the message has the count and the worst finite error."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
        bad = ~(err <= tol)
    if bad.any():
        fin = err[np.isfinite(err)]
        worst = float(fin.max()) if fin.size else float("nan")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside tolerance "
                             f"({int(np.isnan(got).sum())} NaN, {int(np.isinf(got).sum())} inf); "
                             f"worst finite error {worst:.3g}")


def check_close_t(got, ref, tol, what=""):
    """``check_close`` on device tensors (got of any float dtype; ref and tol float64)."""
    import torch

    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    err = (g - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        fin = err[torch.isfinite(err)]
        worst = float(fin.max()) if fin.numel() else float("nan")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside tolerance "
                             f"({int(torch.isnan(g).sum())} NaN, {int(torch.isinf(g).sum())} inf); "
                             f"worst finite error {worst:.3g}")


def gemm_oracle(x_bits_, w_bits, dt):
    """(ref, tol) of x @ W.T in float64 from the 16-bit patterns of x and W."""
    xf, wf = bits_to_f64(x_bits_, dt), bits_to_f64(w_bits, dt)
    ref = xf @ wf.T
    return ref, tol(ref, np.abs(xf) @ np.abs(wf).T, dt)


def check_gemm(y, x_bits_, w_bits, dt, what=""):
    """A torch output against the float64 oracle of its 16-bit inputs."""
    import torch

    ref, bound = gemm_oracle(x_bits_, w_bits, dt)
    yb = y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    check_close(bits_to_f64(yb, dt).reshape(ref.shape), ref, bound, what)


# ---------------------------------------------------------------------------------------------
# decompositions
# ---------------------------------------------------------------------------------------------
GEMV_FORMS = [(8, 1), (8, 2), (8, 4), (16, 1), (16, 2), (16, 4)]  # (waves, rows per row group)


def gemm_cfgs(K, M):
    """Every decomposition of every family (the tuning ABI rejects the invalid ones with
    ERR_ARG); the decode GEMV's forms only at M = 1, its only domain."""
    from nf4_triton_dequantization_amd import _lib

    chunks = K // 128
    for kernel in (_lib.GEMM_PERSIST, _lib.GEMM_STREAM, _lib.GEMM_K128):
        for waves in (4, 8, 16):
            for depth in (1, 2, 4):
                for strips in (1, 2, 4):
                    for ks in (1, 2, 3):
                        yield _lib.GemmCfg(kernel, waves, depth, ks, strips)
    for waves in (4, 8):
        for kc in (2, 4, 8):
            yield _lib.GemmCfg(_lib.GEMM_XS, waves, kc, -(-chunks // kc), 1)
    for waves in (8, 16):
        for depth in (2, 4):
            for kpw in (1, 2, 4):
                yield _lib.GemmCfg(_lib.GEMM_XR, waves, depth, -(-chunks // (waves * kpw)), kpw)
    if M == 1:
        for waves, rows in GEMV_FORMS:
            for wgs in (0, 1, 2):  # workgroups per CU
                yield _lib.GemmCfg(_lib.GEMM_GEMV, waves, rows, 1, wgs)


def cfg_tuple(cfg):
    return (cfg.kernel, cfg.waves, cfg.depth, cfg.ksplit, cfg.strips)


# ---------------------------------------------------------------------------------------------
# rounding, the reference formula and its near misses
# ---------------------------------------------------------------------------------------------
def round_once_bits(x, dt):
    """16-bit pattern of float64 ``x`` rounded ONCE (RNE) to bf16 (8 significant bits) or
    fp16 (11), subnormals on their fixed grid; |x| below the format's overflow threshold."""
    p, emin = _PREC[dt]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                      # x = m 2^e, 0.5 <= |m| < 1
    qe = np.maximum(e - p, emin)            # exponent of the grid spacing at x
    r = np.ldexp(np.rint(np.ldexp(x, -qe)), qe)  # rint: ties to even
    r = np.where(x == 0, x, r)              # keeps the sign of zero
    return O.to_bits(r.astype(np.float32), O.BF16 if dt == "bf16" else O.F16)  # exact: r is representable


def round16_bits(p32, dt):
    return O.to_bits(np.asarray(p32, np.float32), O.BF16 if dt == "bf16" else O.F16)


def ref_scale(q, a2):
    """fp32(fp32(q / 127) * a2) (oracle/nf4_oracle.py::ref_scales)."""
    return ((q.astype(np.float32) / _F127) * a2.astype(np.float32)).astype(np.float32)


def weight_bits(scale, c, dt):
    """RNE16(fp32(NF4[c] * scale)) (oracle/nf4_oracle.py::_apply)."""
    return round16_bits((O.NF4_LUT[c] * scale.astype(np.float32)).astype(np.float32), dt)


def single_rounding_bits(scale, c, dt):
    return round_once_bits(O.NF4_LUT[c].astype(np.float64) * scale.astype(np.float64), dt)


def near_miss_bits(kind, q, a2, c, dt):
    q32, a2 = q.astype(np.float32), a2.astype(np.float32)
    if kind == "single_rounding":
        return single_rounding_bits(ref_scale(q, a2), c, dt)
    if kind == "reciprocal_scale":
        return weight_bits(((q32 * _R127).astype(np.float32) * a2).astype(np.float32), c, dt)
    if kind == "reordered_scale":
        return weight_bits(((q32 * a2).astype(np.float32) / _F127).astype(np.float32), c, dt)
    raise ValueError(kind)


def _boundaries(rng, n, dt):
    """Drawn midpoints between neighbouring 16-bit values, 2^-8 <= |t| < 2 (normal in both
    formats, the size of real weights)."""
    p, _ = _PREC[dt]
    mant = rng.integers(1 << (p - 1), 1 << p, n).astype(np.float64) + 0.5
    e = rng.integers(-8, 1, n)
    return np.ldexp(mant, e - (p - 1))


def _neighbours(v32, spread):
    """fp32 values within `spread` ulps of each v32 (positive normals), [n, 2 spread + 1]."""
    u = v32.view(np.uint32).astype(np.int64)[:, None] + np.arange(-spread, spread + 1)[None, :]
    return u.astype(np.uint32).view(np.float32)


_CODES = np.array([c for c in range(16) if c != 7])  # NF4[7] = 0: every formula gives 0


@functools.lru_cache(maxsize=None)
def double_rounding_cases(dt, count=64, seed=1):
    """(s fp32, c) with RNE16(fp32(NF4[c] * s)) != RNE16(exact NF4[c] * s): the reference
    rounds twice; a fused multiply-convert would round once and differ exactly here."""
    rng = np.random.default_rng(seed)
    found_s, found_c, seen = [], [], set()
    while len(found_s) < count:
        n = 4096
        c = rng.choice(_CODES[1:-1], n)  # NF4[0], NF4[15] = -+1: the product is exact
        t = _boundaries(rng, n, dt)
        s = _neighbours((t / np.abs(O.NF4_LUT[c].astype(np.float64))).astype(np.float32), 2)
        cc = np.repeat(c[:, None], s.shape[1], axis=1)
        hit = weight_bits(s, cc, dt) != single_rounding_bits(s, cc, dt)
        for sv, cv in zip(s[hit].tolist(), cc[hit].tolist()):
            if (sv, cv) not in seen:
                seen.add((sv, cv))
                found_s.append(sv)
                found_c.append(cv)
    return np.array(found_s[:count], np.float32), np.array(found_c[:count])


@functools.lru_cache(maxsize=None)
def sensitive_triples(dt, per_kind=96, seed=1):
    """{kind: (q uint8, a2 fp32, c)} -- at least `per_kind` distinct triples per near miss at
    which that restatement's 16-bit weight differs from the reference's."""
    rng = np.random.default_rng(seed)
    out = {k: ([], [], []) for k in KINDS}
    seen = {k: set() for k in KINDS}
    for _ in range(200):
        if all(len(out[k][0]) >= per_kind for k in KINDS):
            break
        n = 8192
        q = rng.integers(1, 256, n).astype(np.uint8)
        c = rng.choice(_CODES, n)
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
        t = _boundaries(rng, n, dt)
        s1 = (q.astype(np.float32) / _F127).astype(np.float64)
        a2 = _neighbours((t / (np.abs(O.NF4_LUT[c].astype(np.float64)) * s1)).astype(np.float32), 3) * sign[:, None]
        qq = np.repeat(q[:, None], a2.shape[1], axis=1)
        cc = np.repeat(c[:, None], a2.shape[1], axis=1)
        want = weight_bits(ref_scale(qq, a2), cc, dt)
        for k in KINDS:
            hit = near_miss_bits(k, qq, a2, cc, dt) != want
            for tr in zip(qq[hit].tolist(), a2[hit].tolist(), cc[hit].tolist()):
                if tr not in seen[k] and len(out[k][0]) < per_kind:
                    seen[k].add(tr)
                    for lst, v in zip(out[k], tr):
                        lst.append(v)
    for k in KINDS:
        assert len(out[k][0]) >= per_kind, (k, len(out[k][0]))
    return {k: (np.array(v[0], np.uint8), np.array(v[1], np.float32), np.array(v[2], np.int64))
            for k, v in out.items()}


def sensitive_weight(N, K, dt, seed=1):
    """(packed, a1, a2, kind_of_block): fresh copies of ``_sensitive_weight``'s arrays."""
    return tuple(a.copy() for a in _sensitive_weight(N, K, dt, seed))


@functools.lru_cache(maxsize=None)
def _sensitive_weight(N, K, dt, seed):
    """(packed, a1, a2, kind_of_block) of an N x K double-quant weight with full statistics
    (nb = N K / 64 absmax bytes, n2 = N ceil(K / 256) nested scales: no wrap).

    Four neighbouring 64-blocks of a row share one nested scale, so one block of each four
    (its position rotating) takes a found triple -- its absmax byte, the shared nested scale
    and all 64 codes -- and the other three take drawn bytes and codes under that scale.
    ``kind_of_block`` [N, K / 64] is the index into KINDS of a block's triple, or -1.
    Cached and read-only; ``sensitive_weight`` hands out copies.
    """
    assert K % 64 == 0
    tri = sensitive_triples(dt)
    rng = np.random.default_rng(1000 * seed + N + K)
    bpr = K // 64
    g = (bpr + 3) // 4
    a1 = rng.integers(0, 256, (N, bpr)).astype(np.uint8)
    codes = rng.integers(0, 16, (N, bpr, 64)).astype(np.uint8)
    a2 = np.empty((N, g), np.float32)
    kind_of_block = np.full((N, bpr), -1, np.int8)
    i = 0
    for r in range(N):
        for gi in range(g):
            k = i % len(KINDS)
            q, s, c = tri[KINDS[k]]
            j = (i // len(KINDS)) % len(q)
            b = min(4 * gi + (i + r) % 4, bpr - 1)
            a1[r, b], a2[r, gi], codes[r, b, :] = q[j], s[j], c[j]
            kind_of_block[r, b] = k
            i += 1
    flat = codes.reshape(N, K)
    packed = ((flat[:, 0::2] << 4) | flat[:, 1::2]).astype(np.uint8).reshape(-1)  # high nibble: even column
    out = (packed, a1.reshape(-1), a2.reshape(-1), kind_of_block)
    for a in out:
        a.setflags(write=False)
    return out
