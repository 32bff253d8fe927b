"""Activation-side cases of the fused-GEMM suites (test_gpu_gemm_activations.py;
test_activation_cases_cpu.py checks this module itself on the host).

The other suites feed the kernels N(0, 1) draws or rows of the identity.  Here selected rows of
such a draw are replaced, from bit patterns built on the host, by rows a kernel can get wrong
without any of those suites noticing:

    nan        one NaN at a drawn column, the rest drawn
    pinf ninf  one infinity at a column k0 in which EVERY weight in use has both zero and
               non-zero values (NF4 code 7 is exactly 0): the row's outputs are +-inf where the
               weight is non-zero and NaN (inf * 0) where it is zero
    zero       all +0                       negzero    all -0
    tiny       fp16 only: the drawn row times 2^-16, rounded to fp16; more than half subnormal
    small      bf16 only: the drawn row times 2^-100 (exact)
    huge       fp16: the drawn row times the power of two (exact) at which, for every weight in
               use, at least a quarter of the row's reference outputs lie above the fp16 overflow
               threshold 65520 and at least a quarter below the fp16 max 65504;
               bf16: the drawn row times 2^100 (exact); sum |x| |w| stays below FLT_MAX, so no
               fp32 partial can overflow

``special_x`` places them on both sides of a 16-row tile edge and on the last row (rows 0, M-1,
15, 16 where M admits), never on every row -- or on the rows its caller names (``at``: the
row-block expert GEMM's case, ``moe_rb_routing``, puts them on both sides of a row-block edge of
one expert's pair list).  ``judge`` compares an output with the float64
reference by class -- finite within the suites' own bound (``_gemm_cases.tol``, unchanged), the
reference's infinity, NaN -- and ``isolated`` demands that every row not replaced is bitwise what
the same call gives on the plain draw: nothing of a special row may reach a neighbour.

Borderline elements (the bound's band straddles the overflow threshold, so either a finite value
within the bound or the infinity passes) may be at most 5 % of a case.  The reference alone, over
every case test_gpu_gemm_activations.py uses (test_activation_cases_cpu.py recomputes it): at most
2.34 % (three elements of a 1 x 128 output whose only row is the ``huge`` one), 0.07 % on average
over the fp16 cases with a ``huge`` row, none in bf16 and none without a ``huge`` row.
"""
from __future__ import annotations

import numpy as np

from _gemm_cases import bits_to_f64, tol, x_bits

FINITE = {"f16": ("zero", "negzero", "tiny", "huge"), "bf16": ("zero", "negzero", "small", "huge")}
NONFINITE = ("nan", "pinf", "ninf")
BORDERLINE_CAP = 0.05
_NAN = {"f16": 0x7E00, "bf16": 0x7FC0}
_INF = {"f16": 0x7C00, "bf16": 0x7F80}
# the largest finite value, and the threshold from which round-to-nearest-even gives infinity
FMAX = {"f16": 65504.0, "bf16": (2.0 - 2.0 ** -7) * 2.0 ** 127}
OVERFLOW = {"f16": 65520.0, "bf16": (2.0 - 2.0 ** -8) * 2.0 ** 127}
_FLT_MAX = float(np.finfo(np.float32).max)


def kinds_of(dt, which):
    """The kinds of one group: "finite" or "nonfinite"."""
    return FINITE[dt] if which == "finite" else NONFINITE


def scaled_nested(w, f):
    """A nested weight (packed, a1, code2, a2, offset, ...) with absmax2 and the offset times the
    power of two ``f``: every dequantized weight times f exactly (no value leaves the normal
    range at the scales used here).  Drawn statistics give weights of about 0.015, too small for
    an fp16 output to overflow from an fp16 activation."""
    assert f > 0 and np.log2(f) == np.round(np.log2(f))
    packed, a1, code2, a2, off = w[:5]
    f32 = np.float32(f)
    off = None if off is None else float(np.float32(off) * f32)
    return (packed, a1, code2, (np.asarray(a2, np.float32) * f32).astype(np.float32), off) + tuple(w[5:])


def positions(M, n):
    """Rows for n special rows among M: both sides of the 16-row tile edge and the last row
    first (0, M-1, 15, 16), then their neighbours; one row stays plain unless M = 1."""
    assert (M == 1 and n == 1) or n < M, (M, n)
    out = []
    for r in (0, M - 1, 15, 16, 1, M - 2, 14, 17):
        if 0 <= r < M and r not in out:
            out.append(r)
    return out[:n]


def _to_f16_bits(v64):
    with np.errstate(over="ignore"):
        return np.asarray(v64, np.float64).astype(np.float16).view(np.uint16)


def _to_bf16_bits_exact(v64):
    f = np.asarray(v64, np.float64).astype(np.float32)
    b = f.view(np.uint32)
    assert ((b & 0xFFFF) == 0).all() and (f.astype(np.float64) == v64).all(), "not a bf16 value"
    return (b >> 16).astype(np.uint16)


def _row_ref(xrow64, w64):
    """The float64 reference of one row by elementwise product and sum (no BLAS: a routine that
    skips zero operands would lose 0 * inf = NaN), and sum |x| |w|."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (xrow64[None, :] * w64).sum(1), (np.abs(xrow64)[None, :] * np.abs(w64)).sum(1)


def reference(x_bits_, w_bits, dt):
    """(ref, mag) [M, N] in float64 of x @ W.T from 16-bit patterns, row by row."""
    xf, wf = bits_to_f64(np.asarray(x_bits_, np.uint16), dt), bits_to_f64(np.asarray(w_bits, np.uint16), dt)
    ref, mag = np.empty((xf.shape[0], wf.shape[0])), np.empty((xf.shape[0], wf.shape[0]))
    for m in range(xf.shape[0]):
        ref[m], mag[m] = _row_ref(xf[m], wf)
    return ref, mag


def _huge_row(base64, ws64, dt):
    if dt == "bf16":
        row = base64 * 2.0 ** 100
        for w in ws64:
            assert _row_ref(row, w)[1].max() < _FLT_MAX  # no fp32 partial sum can overflow
        return _to_bf16_bits_exact(row)
    best = None
    for p in range(0, 16):
        row = base64 * 2.0 ** p
        if np.abs(row).max() > FMAX["f16"]:
            break
        worst = 1.0
        for w in ws64:
            ref, mag = _row_ref(row, w)
            t = tol(ref, mag, dt)
            over, under = np.abs(ref) - t > OVERFLOW["f16"], np.abs(ref) + t < FMAX["f16"]
            worst = min(worst, float(over.mean()), float(under.mean()))
        if best is None or worst > best[0]:
            best = (worst, p)
    assert best is not None and best[0] >= 0.25, f"no power of two overflows a quarter and keeps a quarter: {best}"
    bits = _to_f16_bits(base64 * 2.0 ** best[1])
    assert (bits_to_f64(bits, dt) == base64 * 2.0 ** best[1]).all()  # exact
    return bits


def special_x(M, K, dt, seed, kinds, w_bits, at=None):
    """(x_bits, base_bits, rows): ``base_bits`` [M, K] the ordinary ``_gemm_cases.x_bits`` draw,
    ``x_bits`` the same with ``len(kinds)`` rows replaced, ``rows`` {row: kind}.  ``w_bits``: the
    16-bit matrix [N, K] of the weight in use, or a list of them (a group, the experts); the
    conditions on k0 and on the ``huge`` power hold for each.  At M = 1 one kind at a time.
    ``at``: the rows to replace, in the order of ``kinds`` (default: ``positions(M, len(kinds))``)."""
    ws = [w_bits] if isinstance(w_bits, np.ndarray) else list(w_bits)
    ws64 = [bits_to_f64(np.asarray(w, np.uint16), dt) for w in ws]
    assert all(w.shape[1] == K and np.isfinite(w).all() for w in ws64)
    base = x_bits(M, K, dt, seed)[1].copy()
    x = base.copy()
    rng = np.random.default_rng(seed)
    if at is None:
        at = positions(M, len(kinds))
    assert len(at) >= len(kinds) and len(set(at)) == len(at) and all(0 <= r < M for r in at), (M, at, kinds)
    rows = dict(zip(at, kinds))
    for r, kind in rows.items():
        b64 = bits_to_f64(base[r], dt)
        if kind == "nan":
            x[r, rng.integers(0, K)] = _NAN[dt]
        elif kind in ("pinf", "ninf"):
            start = int(rng.integers(0, K))
            k0 = next((k % K for k in range(start, start + K)
                       if all((w[:, k % K] == 0).any() and (w[:, k % K] != 0).any() for w in ws64)), None)
            assert k0 is not None, "no column with zero and non-zero weights in every weight"
            x[r, k0] = _INF[dt] | (0x8000 if kind == "ninf" else 0)
        elif kind == "zero":
            x[r] = 0
        elif kind == "negzero":
            x[r] = 0x8000
        elif kind == "tiny":
            assert dt == "f16"
            x[r] = _to_f16_bits(b64 * 2.0 ** -16)
            sub = ((x[r] & 0x7C00) == 0) & ((x[r] & 0x7FFF) != 0)
            assert sub.mean() > 0.5, sub.mean()
        elif kind == "small":
            assert dt == "bf16"
            x[r] = _to_bf16_bits_exact(b64 * 2.0 ** -100)
        elif kind == "huge":
            x[r] = _huge_row(b64, ws64, dt)
        else:
            raise ValueError(kind)
    for a in (x, base):
        a.setflags(write=False)
    return x, base, rows


def classify(ref, mag, dt):
    """(below, above, border) over the finite references: the bound's band wholly below the
    format's max, wholly above the overflow threshold, or straddling."""
    with np.errstate(invalid="ignore"):
        t = tol(ref, mag, dt)
        fin = np.isfinite(ref)
        below = fin & (np.abs(ref) + t < FMAX[dt])
        above = fin & (np.abs(ref) - t > OVERFLOW[dt])
    return below, above, fin & ~below & ~above


def borderline_share(x_bits_, w_bits, dt):
    ref, mag = reference(x_bits_, w_bits, dt)
    return float(classify(ref, mag, dt)[2].mean())


def judge(y_bits, x_bits_, w_bits, dt, what="", rows=None, ref=None):
    """Fail unless every element of ``y_bits`` [M, N] has the class and value the float64
    reference of (x_bits_, w_bits) demands; returns the borderline share (capped at 5 %).
    ``ref``: a precomputed ``reference(x_bits_, w_bits, dt)``.  ``rows`` {row: kind}: a ``zero``
    or ``negzero`` row must be 0 by value (either sign)."""
    y = bits_to_f64(np.asarray(y_bits, np.uint16), dt)
    ref, mag = reference(x_bits_, w_bits, dt) if ref is None else ref
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    below, above, border = classify(ref, mag, dt)
    with np.errstate(invalid="ignore"):
        close = np.abs(y - ref) <= tol(ref, mag, dt)          # False for a NaN or inf y
        same_inf = np.isinf(y) & (np.sign(y) == np.sign(ref))
    ok = np.where(np.isnan(ref), np.isnan(y),
                  np.where(np.isinf(ref), same_inf,
                           np.where(below, close, np.where(above, same_inf, close | same_inf))))
    for r, kind in (rows or {}).items():
        if kind in ("zero", "negzero"):
            ok[r] &= y[r] == 0
    if not ok.all():
        bad = np.argwhere(~ok)
        m, n = (int(v) for v in bad[0])
        kind = (rows or {}).get(m, "plain")
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} outputs wrong ({int(np.isnan(y).sum())} NaN, "
                             f"{int(np.isinf(y).sum())} inf; reference {int(np.isnan(ref).sum())} NaN, "
                             f"{int(np.isinf(ref).sum())} inf), rows {sorted(set(bad[:, 0].tolist()))[:8]}; first at "
                             f"({m}, {n}), a {kind} row: got {y[m, n]!r} reference {ref[m, n]!r}")
    share = float(border.mean())
    assert share <= BORDERLINE_CAP, f"{what}: {share:.2%} of the outputs straddle the overflow threshold (cap 5 %)"
    return share


def isolated(y_special_bits, y_base_bits, rows, what=""):
    """Every row not replaced must be bitwise what the same call gave on the plain draw (the
    same cfg sums in the same order, so nothing but a leak can change it)."""
    ys, yb = np.asarray(y_special_bits, np.uint16), np.asarray(y_base_bits, np.uint16)
    assert ys.shape == yb.shape, (what, ys.shape, yb.shape)
    plain = np.array([m for m in range(ys.shape[0]) if m not in rows], dtype=np.int64)
    diff = (ys[plain] != yb[plain]).any(axis=1) if plain.size else np.zeros(0, bool)
    assert not diff.any(), (f"{what}: plain rows {plain[diff].tolist()[:8]} changed when rows "
                            f"{dict(sorted(rows.items()))} were replaced")


# ---------------------------------------------------------------------------------------------
# the cases of test_gpu_gemm_activations.py: shapes, decompositions and the weights in use
# ---------------------------------------------------------------------------------------------
K128, STREAM, PERSIST, XS, XR, GEMV = 1, 2, 3, 4, 5, 7   # NF4DQ_GEMM_* numbers
GEMM_N, GEMM_MS = 128, (1, 8, 32)
GROUPED_REF = {"Ns": (128, 64, 64), "K": 2048, "Ms": (1, 8)}     # M = 1: the grouped GEMV
GROUPED_BNB = {"Ns": (64, 192, 64), "K": 2048, "Ms": (1, 16)}
MT = {"N": 192, "K": 768, "Ms": (17, 33, 100)}
MOE = {"E": 4, "N": 192, "K": 768, "P": 33, "x_div": 2}
MOE_RB = {"P": 300, "x_div": 2}   # nf4_gemm_bnb_moe_rb on the MOE stack: three row blocks in the grid
SWIGLU = {"I": 192, "K": 1152, "M": 48}
API_LINEAR = {"N": 128, "K": 1024, "Ms": (1, 32, 33, 128, 129)}
DRAWN_SCALE = 32.0  # drawn nested statistics times 2^5: outputs of about 16 for N(0, 1) activations


def decode_cfgs(M, reference_mode):
    """[(K, cfg tuple or None)]: the library's choice and one or two members of
    ``_gemm_cases.gemm_cfgs`` per family, with 1, 2 and 3 K slices each at the smallest K where
    the family admits that split (N = 128).  The persistent kernel takes up to 16 rows; its
    slices must divide the 256-deep chunks evenly (three slices: K = 1536).  The register-resident
    kernel's slices follow from K: 8 waves of one 128-deep chunk give 1, 2 and 3 slices at
    K = 1024, 2048 (the hand-off by exchange) and 3072 (ticket and slice-order reduction).  The
    GEMV is M = 1, K = 2048.  The streaming and shared-activation kernels exist in the reference
    semantics only (XS: slices = ceil(chunks / depth))."""
    out = [(1024, None)]
    out += [(1024, (K128, 4, 1, ks, 1)) for ks in (1, 2, 3)]
    if M <= 16:
        out += [(1024, (PERSIST, 4, 2, 1, 2)), (1024, (PERSIST, 4, 2, 2, 4)), (1536, (PERSIST, 4, 2, 3, 4))]
    out += [(1024, (XR, 8, 2, 1, 1)), (2048, (XR, 8, 2, 2, 1)), (3072, (XR, 8, 2, 3, 1))]
    if M == 1:
        out += [(2048, None), (2048, (GEMV, 8, 1, 1, 0)), (2048, (GEMV, 16, 4, 1, 0))]
    if reference_mode:
        out += [(1024, (STREAM, 4, 2, ks, 1)) for ks in (1, 2, 3)]
        out += [(1024, (XS, 4, 8, 1, 1)), (1024, (XS, 4, 4, 2, 1)), (1536, (XS, 4, 4, 3, 1))]
    return out


def x_seed(M, K):
    return 1000 + 7 * M + K


def moe_rb_routing():
    """(ids[300], special tokens) of the row-block case (test_gpu_gemm_moe_rb_activations.py): 150
    tokens of two pairs.  Every token has one pair on expert 1 -- its odd pair, its even one where
    t % 7 == 0 -- and tokens 0 .. 8 both, so expert 1's ascending list has 159 entries: row block 0
    full, row block 1 with 31 rows (a partly filled last row tile), its entries 127 and 128 (the last
    staged row of block 0, the first of block 1) in the middle of a ballot round, in tokens 118 and
    119, and its last entry pair 299 = P - 1.  The other pairs go round experts 0, 2, 3 (at least
    45 each: at least 20 rows per pair of any one special token in every expert's subset, so with
    one ``huge`` token no subset's borderline share can exceed BORDERLINE_CAP whatever the values),
    but token 118's, which has the invalid id E, and plain token 60's, which has -1.  The special
    tokens, in the order of the kinds: 118, 119, 149 (last entry, pair P - 1), 0 (pair 0)."""
    E, P = MOE["E"], MOE_RB["P"]
    ids = np.empty(P, np.int64)
    other = 0
    for t in range(P // 2):
        mine, rest = (2 * t, 2 * t + 1) if t % 7 == 0 else (2 * t + 1, 2 * t)
        ids[mine] = 1
        if t < 9:
            ids[rest] = 1
        else:
            ids[rest] = (0, 2, 3)[other % 3]
            other += 1
    ids[2 * 118] = E
    ids[2 * 60 + (60 % 7 == 0)] = -1
    return ids, [118, 119, 149, 0]


def moe_rb_passes(kinds, tokens):
    """The orders in which a kind set goes onto the special tokens: a set with fewer kinds than
    tokens runs a second time from the other end, so that every special token gets a kind."""
    return [list(tokens)] if len(kinds) >= len(tokens) else [list(tokens), list(tokens)[::-1]]


def kind_sets(M, dt, which):
    """The kinds of one call: all of the group at once, or one at a time at M = 1."""
    kinds = kinds_of(dt, which)
    return [(k,) for k in kinds] if M == 1 else [kinds]


def decode_weight(mode, N, K):
    """The host arrays of the weight the decode entries use: "nested" (drawn statistics times
    DRAWN_SCALE), "single" (fp32 absmax) or "ref" (the reference semantics' double quantization)."""
    import nf4_oracle as O
    from _gemm_bnb_cases import drawn_weight_bnb, single_weight_bnb

    if mode == "nested":
        return scaled_nested(drawn_weight_bnb(N, K, seed=N + K), DRAWN_SCALE)
    if mode == "single":
        return single_weight_bnb(N, K, seed=N + K + 1)
    return O.make_inputs(N, K, seed=N + K, a2_kind="normal")


def mt_weight(mode, dt):
    """The row-tiled entries' weight [192, 768]: the sensitive nested weight (blocksize2 16), or
    fp32 statistics times 2 (outputs of about 16)."""
    from _gemm_bnb_cases import sensitive_weight_bnb, single_weight_bnb

    N, K = MT["N"], MT["K"]
    if mode == "nested":
        return sensitive_weight_bnb(N, K, dt)[:5]
    packed, absmax = single_weight_bnb(N, K, seed=N + K + 1)
    return packed, (absmax * np.float32(2.0)).astype(np.float32)


def swiglu_weights():
    """(gate, up) host arrays [192, 1152]: drawn statistics times DRAWN_SCALE; the up weight with
    blocksize2 16, the reversed code2 table times 0.75 and a negative offset."""
    from _gemm_bnb_cases import code2_np, drawn_weight_bnb

    I, K = SWIGLU["I"], SWIGLU["K"]
    gate = scaled_nested(drawn_weight_bnb(I, K, seed=I + K), DRAWN_SCALE)
    p, a1, _, a2, _ = drawn_weight_bnb(I, K, seed=I + K + 5, blocksize2=16)
    c2u = (code2_np()[::-1] * np.float32(0.75)).astype(np.float32).copy()
    return gate, scaled_nested((p, a1, c2u, a2, -0.0371), DRAWN_SCALE)


def grouped_bnb_weights(dt):
    """``nested_group`` with the two drawn weights' statistics times DRAWN_SCALE, which brings
    their outputs near the sensitive weight's (one activation row must overflow a quarter of all
    three and keep a quarter)."""
    from _gemm_bnb_grouped_cases import nested_group

    g = nested_group(GROUPED_BNB["Ns"], GROUPED_BNB["K"], dt)
    return (scaled_nested(g[0], DRAWN_SCALE), g[1], scaled_nested(g[2], DRAWN_SCALE))


API_EXPERTS = {"E": 4, "N": 128, "K": 256, "T": 17, "k": 2}


def experts_weights():
    """E nested host weights [128, 256] for an ``Experts4bit`` (one code2 table, blocksize2 256):
    drawn statistics times 2^8 (K is short), every expert its own draw."""
    from _gemm_bnb_cases import drawn_weight_bnb

    N, K = API_EXPERTS["N"], API_EXPERTS["K"]
    return [scaled_nested(drawn_weight_bnb(N, K, seed=400 + e), 256.0) for e in range(API_EXPERTS["E"])]


def host_cases(coracle, dt):
    """(label, M, K, [w_bits, ...]) of every activation matrix test_gpu_gemm_activations.py
    builds (``special_x(M, K, dt, x_seed(M, K), kinds, w_bits)`` for every ``kind_sets``); the MoE
    stack comes from test_gpu_gemm_moe._Stack and is added by the caller."""
    import nf4_oracle as O

    N = GEMM_N
    for mode in ("nested", "single", "ref"):
        for M in GEMM_MS:
            for K in sorted({K for K, _ in decode_cfgs(M, mode == "ref")}):
                yield f"decode {mode}", M, K, [bits_of(coracle, decode_weight(mode, N, K), N, K, dt)]
    K = GROUPED_REF["K"]
    ws = [bits_of(coracle, O.make_inputs(n, K, seed=n + K + 11 * i, a2_kind="normal"), n, K, dt)
          for i, n in enumerate(GROUPED_REF["Ns"])]
    for M in GROUPED_REF["Ms"]:
        yield "grouped ref", M, K, ws
    K = GROUPED_BNB["K"]
    ws = [bits_of(coracle, w, n, K, dt) for w, n in zip(grouped_bnb_weights(dt), GROUPED_BNB["Ns"])]
    for M in GROUPED_BNB["Ms"]:
        yield "grouped bnb", M, K, ws
    for mode in ("nested", "single"):
        w = bits_of(coracle, mt_weight(mode, dt), MT["N"], MT["K"], dt, bs2=16)
        for M in MT["Ms"]:
            yield f"row-tiled {mode}", M, MT["K"], [w]
    yield "swiglu", SWIGLU["M"], SWIGLU["K"], [bits_of(coracle, w, SWIGLU["I"], SWIGLU["K"], dt, bs2)
                                               for w, bs2 in zip(swiglu_weights(), (256, 16))]
    w = bits_of(coracle, decode_weight("nested", API_LINEAR["N"], API_LINEAR["K"]), API_LINEAR["N"], API_LINEAR["K"], dt)
    for M in API_LINEAR["Ms"]:
        yield "nf4_linear_bnb", M, API_LINEAR["K"], [w]
    yield "Experts4bit", API_EXPERTS["T"], API_EXPERTS["K"], [bits_of(coracle, w, API_EXPERTS["N"], API_EXPERTS["K"], dt)
                                                              for w in experts_weights()]


def bits_of(coracle, w, N, K, dt, bs2=256):
    """The oracle's 16-bit matrix [N, K] of a host weight: nested (5 or 6 arrays), single (2) or
    reference semantics (3)."""
    import nf4_oracle as O

    code = O.BF16 if dt == "bf16" else O.F16
    if len(w) == 2:
        return coracle.dequant_bnb_single(w[0], w[1], N * K, code, 64).reshape(N, K)
    if len(w) == 3:
        return coracle.dequant_ref(w[0], w[1], w[2], N, K, code).reshape(N, K)
    off = 0.0 if w[4] is None else float(w[4])
    return coracle.dequant_bnb(w[0], w[1], w[2], w[3], off, N * K, code, 64, w[5] if len(w) > 5 else bs2).reshape(N, K)
