"""The activation side of every fused GEMM entry on the GPU (``-m gpu``): NaN, infinities, zero
rows, fp16 subnormals, rows that overflow the fp16 output and bf16 rows of extreme magnitude
(tests/_activation_cases.py builds them and test_activation_cases_cpu.py proves the checks on the
host).

Every call has NaN-prefilled outputs and is made twice, on the matrix with the special rows and
on the plain draw it was made from.  ``judge`` compares the first with the float64 reference by
class and value -- a NaN reference must be NaN, an infinite one the same infinity, a finite one
inside the suites' own bound or, where the bound lies above the overflow threshold, the infinity
of its sign -- and ``isolated`` demands that every plain row has the same bits in both calls: a
special value stays in its own token.  After every call the workspace is all zero and
nf4_gemm_check_workspace is clean: a NaN partial is a value on the split-K wire, not a timeout.

The finite kinds (zero, negzero, tiny / small, huge) run before the non-finite ones.
"""
import ctypes

import numpy as np
import pytest
import torch

import _activation_cases as A
import nf4_oracle as O
import test_gpu_gemm_bnb as BNB
import test_gpu_gemm_bnb_grouped as GRP
import test_gpu_gemm_moe as MOET
import test_gpu_gemm_mt as MTT
import test_gpu_gemm_mt_swiglu as SG
from _gemm_cases import bits_to_f64
from _swiglu_cases import accept

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _dev(bits, dt, gpu):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu).view(_tdt(dt))


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _code(_lib, dt):
    return _lib.BF16 if dt == "bf16" else _lib.F16


def _lib_and_L():
    from nf4_triton_dequantization_amd import _lib

    return _lib, _lib.lib()


def _run(calls, M, K, dt, which, ws_bits, gpu, what):
    """``calls`` {name: f(x on the device) -> [y per weight]}: every call on the special matrix of
    each kind set and on its plain draw; the references are computed once per kind set."""
    shares = []
    for kinds in A.kind_sets(M, dt, which):
        xs, base, rows = A.special_x(M, K, dt, A.x_seed(M, K), kinds, ws_bits)
        refs = [A.reference(xs, w, dt) for w in ws_bits]
        xd, bd = _dev(xs, dt, gpu), _dev(base, dt, gpu)
        for name, call in calls.items():
            tag = f"{what} M={M} K={K} {dt} {name} rows {rows}"
            yb = [_bits(y) for y in call(bd)]
            ys = [_bits(y) for y in call(xd)]
            assert len(ys) == len(ws_bits)
            for i, w in enumerate(ws_bits):
                shares.append(A.judge(ys[i], xs, w, dt, f"{tag} weight {i}", rows=rows, ref=refs[i]))
                A.isolated(ys[i], yb[i], rows, f"{tag} weight {i}")
    print(f"{what} M={M} K={K} {dt} {which}: {len(calls)} calls per kind set, borderline share at most {max(shares):.3%}")


def _finish(L, ws, wsz, sp, what):
    assert L.nf4_gemm_check_workspace(ws.data_ptr() if wsz else None, wsz, sp) == 0, f"{what}: the split-K error word is set"
    if wsz:
        assert int(ws.count_nonzero()) == 0, f"{what}: tickets or slab entries left set"


# ---- the decode entries: nf4_gemm_bnb, nf4_gemm_bnb_single, nf4_gemm (reference semantics) ----
def _decode_call(mode, t, xd, M, N, K, dt, cfg):
    """One call of the entry of ``mode`` with cfg (a tuple, or None for the library's choice) on a
    fresh zeroed workspace; the explicit cfgs are valid for their shapes, so rc must be 0."""
    _lib, L = _lib_and_L()
    c = None if cfg is None else _lib.GemmCfg(*cfg)
    cp = ctypes.byref(c) if c is not None else None
    sp = torch.cuda.current_stream().cuda_stream
    y = torch.full((M, N), float("nan"), dtype=_tdt(dt), device=xd.device)
    code = _code(_lib, dt)
    if mode == "ref":
        wsz = L.nf4_gemm_workspace_bytes(M, N, K) if c is None else L.nf4_gemm_workspace_bytes_cfg(M, N, K, cp)
    else:
        wsz = L.nf4_gemm_bnb_workspace_bytes(M, N, K, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=xd.device)
    wp = ws.data_ptr() if wsz else None
    if mode == "nested":
        q, a1, c2, a2, off = t
        rc = L.nf4_gemm_bnb(xd.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                            a2.data_ptr(), a2.numel(), off.data_ptr(), 64, 256, y.data_ptr(), code, N, K, wp, wsz, cp, sp)
    elif mode == "single":
        q, am = t
        rc = L.nf4_gemm_bnb_single(xd.data_ptr(), M, q.data_ptr(), q.numel(), am.data_ptr(), am.numel(), 64, y.data_ptr(),
                                   code, N, K, wp, wsz, cp, sp)
    else:
        q, a1, a2 = t
        args = (xd.data_ptr(), M, q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(), a2.numel(),
                y.data_ptr(), code, N, K, wp, wsz)
        rc = L.nf4_gemm_ref(*args, sp) if c is None else L.nf4_gemm_ref_cfg(*args, cp, sp)
    assert rc == 0, (mode, M, K, cfg, _lib.strerror(rc))
    _finish(L, ws, wsz, sp, f"{mode} M={M} K={K} cfg {cfg}")
    return y


def _decode(coracle, gpu, dt, which, mode, M):
    N = A.GEMM_N
    by_K = {}
    for K, cfg in A.decode_cfgs(M, mode == "ref"):
        by_K.setdefault(K, []).append(cfg)
    for K, cfgs in by_K.items():
        w = A.decode_weight(mode, N, K)
        wb = A.bits_of(coracle, w, N, K, dt)
        if mode == "nested":
            t = BNB._dev_nested(w, gpu)
        else:
            t = [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in w]
        calls = {f"cfg {cfg}": (lambda xd, cfg=cfg: [_decode_call(mode, t, xd, M, N, K, dt, cfg)]) for cfg in cfgs}
        _run(calls, M, K, dt, which, [wb], gpu, f"decode {mode}")


# ---- the grouped entries ------------------------------------------------------------------------
def _grouped_ref(coracle, gpu, dt, which, M):
    """nf4_gemm_ref_grouped, Ns = (128, 64, 64), K = 2048, the library's choice: the grouped GEMV
    at M = 1."""
    _lib, L = _lib_and_L()
    Ns, K = A.GROUPED_REF["Ns"], A.GROUPED_REF["K"]
    hosts = [O.make_inputs(n, K, seed=n + K + 11 * i, a2_kind="normal") for i, n in enumerate(Ns)]
    wbs = [A.bits_of(coracle, w, n, K, dt) for w, n in zip(hosts, Ns)]
    ts = [[torch.from_numpy(v).to(gpu) for v in w] for w in hosts]

    def call(xd):
        ys = [torch.full((M, n), float("nan"), dtype=_tdt(dt), device=gpu) for n in Ns]
        mats = (_lib.GemmMat * len(Ns))()
        for i, (t, n, y) in enumerate(zip(ts, Ns, ys)):
            mats[i] = _lib.GemmMat(t[0].data_ptr(), t[0].numel(), t[1].data_ptr(), t[1].numel(), t[2].data_ptr(),
                                   t[2].numel(), y.data_ptr(), n)
        wsz = L.nf4_gemm_grouped_workspace_bytes(M, K, mats, len(Ns), None)
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=gpu)
        sp = torch.cuda.current_stream().cuda_stream
        rc = L.nf4_gemm_ref_grouped(xd.data_ptr(), M, K, mats, len(Ns), _code(_lib, dt), ws.data_ptr() if wsz else None,
                                    wsz, None, sp)
        assert rc == 0, _lib.strerror(rc)
        _finish(L, ws, wsz, sp, f"grouped ref M={M}")
        return ys

    _run({"library choice": call}, M, K, dt, which, wbs, gpu, "grouped ref")


def _grouped_bnb(coracle, gpu, dt, which, M):
    """nf4_gemm_bnb_grouped over the three-weight nested group (own code2 tables, offsets and
    blocksize2), the library's choice."""
    _lib, L = _lib_and_L()
    Ns, K = A.GROUPED_BNB["Ns"], A.GROUPED_BNB["K"]
    grp = GRP.Group(coracle, gpu, Ns, K, dt, weights=A.grouped_bnb_weights(dt))

    def call(xd):
        ys = [torch.full((M, n), float("nan"), dtype=_tdt(dt), device=gpu) for n in Ns]
        arr = grp.mats([y.data_ptr() for y in ys])
        mp = ctypes.cast(arr, ctypes.c_void_p)
        wsz = L.nf4_gemm_bnb_grouped_workspace_bytes(M, K, mp, len(Ns), 0, None)
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=gpu)
        sp = torch.cuda.current_stream().cuda_stream
        rc = L.nf4_gemm_bnb_grouped(xd.data_ptr(), M, K, mp, len(Ns), 0, _code(_lib, dt), ws.data_ptr() if wsz else None,
                                    wsz, None, sp)
        assert rc == 0, _lib.strerror(rc)
        _finish(L, ws, wsz, sp, f"grouped bnb M={M}")
        return ys

    _run({"library choice": call}, M, K, dt, which, grp.bits, gpu, "grouped bnb")


# ---- the row-tiled entries ------------------------------------------------------------------------
def _row_tiled(coracle, gpu, dt, which, mode, M):
    N, K = A.MT["N"], A.MT["K"]
    W = MTT._Weight(coracle, gpu, mode, A.mt_weight(mode, dt), N, K, dt, bs2=16)
    calls = {"library choice": lambda xd: [MTT._gemm(W, xd, M)],
             "waves 2, ksplit 3": lambda xd: [MTT._gemm(W, xd, M, MTT._cfg(2, 3))]}
    _run(calls, M, K, dt, which, [W.bits], gpu, f"row-tiled {mode}")


# ---- the expert GEMM --------------------------------------------------------------------------------
def _moe(coracle, gpu, dt, which):
    """P = 33 pairs over 17 tokens (x_div 2): a special token feeds two pairs, of different
    experts under both routings; each pair is judged against its own expert's weights, and a pair
    with an invalid id reads as zero bits even when its token row is NaN or Inf."""
    E, N, K, P, x_div = (A.MOE[k] for k in ("E", "N", "K", "P", "x_div"))
    S = MOET._stack(coracle, gpu, "nested", "sensitive", E, N, K, dt)
    T = -(-P // x_div)
    tok = np.arange(P) // x_div
    pats = MOET._patterns(P, E)
    for kinds in A.kind_sets(T, dt, which):
        xs, base, rows = A.special_x(T, K, dt, A.x_seed(T, K), kinds, S.bits)
        pair_rows = {p: rows[tok[p]] for p in range(P) if tok[p] in rows}
        refs = [A.reference(xs, S.bits[e], dt) for e in range(E)]
        xd, bd = _dev(xs, dt, gpu), _dev(base, dt, gpu)
        for name in ("round robin", "-1 and E among valid ids"):
            ids = np.asarray(pats[name])
            valid = (ids >= 0) & (ids < E)
            if name != "round robin":
                assert any(not valid[p] for p in pair_rows), "no invalid id on a special token"
            for cfg in (None, MOET._cfg(2, 3)):
                tag = f"moe {name} {dt} cfg {cfg and (cfg.waves, cfg.ksplit)} rows {rows}"
                yb, ys = _bits(MOET._moe(S, bd, ids, x_div, cfg)), _bits(MOET._moe(S, xd, ids, x_div, cfg))
                assert (ys[~valid] == 0).all() and (yb[~valid] == 0).all(), f"{tag}: rows of invalid ids are not zero bits"
                for e in range(E):
                    sel = np.nonzero(ids == e)[0]
                    ref = tuple(a[tok[sel]] for a in refs[e])
                    sel_rows = {i: pair_rows[p] for i, p in enumerate(sel) if p in pair_rows}
                    A.judge(ys[sel], xs[tok[sel]], S.bits[e], dt, f"{tag} expert {e}", rows=sel_rows, ref=ref)
                A.isolated(ys, yb, pair_rows, tag)


# ---- the fused gate/up SwiGLU launch ------------------------------------------------------------
def _swiglu_pair(coracle, gpu, dt):
    I, K = A.SWIGLU["I"], A.SWIGLU["K"]
    g, u = A.swiglu_weights()
    return SG._Weight(coracle, gpu, "nested", g[:5], I, K, dt), SG._Weight(coracle, gpu, "nested", u[:5], I, K, dt, bs2=16)


def _swiglu(coracle, gpu, dt, which):
    """h against the chain of the bits nf4_gemm_bnb_mt returns for gate and up at the same ksplit
    (the library's choice is one K slice), with the acceptance extended to non-finite g and u; the
    special rows drive g and u to NaN, +-inf, |g| far beyond 89 and 0."""
    I, K, M = A.SWIGLU["I"], A.SWIGLU["K"], A.SWIGLU["M"]
    G, U = _swiglu_pair(coracle, gpu, dt)
    for kinds in A.kind_sets(M, dt, which):
        xs, base, rows = A.special_x(M, K, dt, A.x_seed(M, K), kinds, [G.bits, U.bits])
        xd, bd = _dev(xs, dt, gpu), _dev(base, dt, gpu)
        for cfg, ksplit in ((None, 1), (SG._cfg(2, 3), 3)):
            tag = f"swiglu {dt} ksplit {ksplit} rows {rows}"
            g, u = _bits(SG._mt(G, xd, M, ksplit)), _bits(SG._mt(U, xd, M, ksplit))
            A.judge(g, xs, G.bits, dt, f"{tag} gate", rows=rows)
            A.judge(u, xs, U.bits, dt, f"{tag} up", rows=rows)
            gf = bits_to_f64(g, dt)
            if which == "nonfinite":
                assert np.isnan(gf).any() and (gf == np.inf).any() and (gf == -np.inf).any()
            else:
                r = next(m for m, k in rows.items() if k == "huge")
                assert (gf[r] < -89).any() and (gf[r] > 89).any()
            h, hb = _bits(SG._swiglu(G, U, xd, M, cfg)), _bits(SG._swiglu(G, U, bd, M, cfg))
            accept(h, g, u, dt, tag, nonfinite=True)
            A.isolated(h, hb, rows, tag)


# =================================================================================================
# finite kinds: zero, negzero, tiny (fp16) / small (bf16), huge
# =================================================================================================
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["nested", "single", "ref"])
@pytest.mark.parametrize("M", A.GEMM_MS)
def test_finite_rows_decode_entries(coracle, gpu, dt, mode, M):
    """nf4_gemm_bnb, nf4_gemm_bnb_single and nf4_gemm at N = 128: the library's choice and the
    explicit decompositions of _activation_cases.decode_cfgs (every family the entry accepts, 1, 2
    and 3 K slices: direct stores, the hand-off by exchange, ticket and slice-order reduction)."""
    _decode(coracle, gpu, dt, "finite", mode, M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", A.GROUPED_REF["Ms"])
def test_finite_rows_grouped_reference_entry(coracle, gpu, dt, M):
    _grouped_ref(coracle, gpu, dt, "finite", M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", A.GROUPED_BNB["Ms"])
def test_finite_rows_grouped_bnb_entry(coracle, gpu, dt, M):
    _grouped_bnb(coracle, gpu, dt, "finite", M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("M", A.MT["Ms"])
def test_finite_rows_row_tiled_entries(coracle, gpu, dt, mode, M):
    """nf4_gemm_bnb_mt / _mt_single, N = 192, K = 768: rows beyond M are zeros in LDS and the
    special rows sit on both sides of a 16-row tile edge and on the last row."""
    _row_tiled(coracle, gpu, dt, "finite", mode, M)


@pytest.mark.parametrize("dt", DTS)
def test_finite_rows_expert_gemm(coracle, gpu, dt):
    _moe(coracle, gpu, dt, "finite")


@pytest.mark.parametrize("dt", DTS)
def test_finite_rows_swiglu(coracle, gpu, dt):
    _swiglu(coracle, gpu, dt, "finite")


def test_swiglu_identity_windows_with_g_across_the_expf_overflow(coracle, gpu):
    """bf16, the statistics scaled so that the largest gate weight is 112: g covers [-110, -80] and
    [80, 110] with finite, exactly known values on both sides of -88.72, where the chain's fp32
    ``expf(-g)`` overflows and s becomes -0 (the identity walk of test_gpu_gemm_mt_swiglu.py)."""
    dt = "bf16"
    G1, _ = SG._pair(coracle, gpu, "nested", 64, 256, dt)
    scale = float(np.float32(112.0 / np.abs(bits_to_f64(G1.bits, dt)).max()))
    G, U = SG._pair(coracle, gpu, "nested", 64, 256, dt, scale=scale)
    g = bits_to_f64(G.bits, dt)
    for lo, hi in ((-110, -89), (-88.5, -80), (80, 88.5), (89, 110)):
        assert ((g >= lo) & (g <= hi)).sum() >= 16, (lo, hi)
    SG._identity_walk(G, U, gpu, dt, (None, SG._cfg(4, 2)), "g across the expf overflow")


# ---- the Python API -------------------------------------------------------------------------------
def _api(coracle, gpu, dt, which, monkeypatch):
    from nf4_triton_dequantization_amd import Experts4bit, check_gemm_workspaces, nf4_linear_bnb, nf4_swiglu_bnb

    # nf4_linear_bnb: the decode kernels (1, 32), the row-tiled entry (33, 128), dequantize + matmul (129)
    N, K = A.API_LINEAR["N"], A.API_LINEAR["K"]
    w = A.decode_weight("nested", N, K)
    wb = A.bits_of(coracle, w, N, K, dt)
    mod = BNB._module_nested(w, N, K, dt, gpu)
    with torch.no_grad():
        for M in A.API_LINEAR["Ms"]:
            _run({"nf4_linear_bnb": lambda xd: [nf4_linear_bnb(xd, mod)]}, M, K, dt, which, [wb], gpu, "nf4_linear_bnb")
        assert check_gemm_workspaces() is None
        # one captured call at M = 32 whose static x is overwritten between replays
        M = 32
        (kinds,) = A.kind_sets(M, dt, which)
        xs, base, rows = A.special_x(M, K, dt, A.x_seed(M, K), kinds, [wb])
        x = _dev(base, dt, gpu)
        eager = _bits(nf4_linear_bnb(x, mod))  # (also the warm-up)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = nf4_linear_bnb(x, mod)
        seen = {}
        for name, bits in (("plain", base), ("special", xs), ("plain again", base)):
            x.copy_(_dev(bits, dt, gpu))
            y.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            seen[name] = _bits(y)
        assert np.array_equal(seen["plain"], eager) and np.array_equal(seen["plain again"], eager)
        A.judge(seen["special"], xs, wb, dt, f"replay {dt} rows {rows}", rows=rows)
        A.isolated(seen["special"], seen["plain"], rows, f"replay {dt}")
        assert check_gemm_workspaces() is None

        # Experts4bit.forward: 17 tokens, two choices each, one -1 and one E among the ids
        E, N, K, T, k = (A.API_EXPERTS[n] for n in ("E", "N", "K", "T", "k"))
        hosts = A.experts_weights()
        ebits = [A.bits_of(coracle, h, N, K, dt) for h in hosts]
        stack = lambda i, dtype: torch.from_numpy(np.stack([np.asarray(h[i], dtype) for h in hosts])).to(gpu)
        ex = Experts4bit(K, N, stack(0, np.uint8), stack(1, np.uint8), stack(3, np.float32),
                         torch.from_numpy(hosts[0][2]).to(gpu), torch.tensor([h[4] for h in hosts], dtype=torch.float32,
                                                                             device=gpu), _tdt(dt))
        ids = (np.arange(T * k) % E).reshape(T, k)
        ids[0, 1], ids[T - 1, 0] = -1, E
        idt = torch.from_numpy(ids).to(gpu)
        (kinds,) = A.kind_sets(T, dt, which)
        xs, base, rows = A.special_x(T, K, dt, A.x_seed(T, K), kinds, ebits)
        assert 0 in rows and T - 1 in rows
        ys, yb = (_bits(ex(_dev(b, dt, gpu), idt)).reshape(T * k, N) for b in (xs, base))
        flat, tok = ids.reshape(-1), np.arange(T * k) // k
        pair_rows = {p: rows[tok[p]] for p in range(T * k) if tok[p] in rows}
        valid = (flat >= 0) & (flat < E)
        assert (ys[~valid] == 0).all(), "Experts4bit: rows of invalid ids are not zero bits"
        for e in range(E):
            sel = np.nonzero(flat == e)[0]
            sel_rows = {i: pair_rows[p] for i, p in enumerate(sel) if p in pair_rows}
            A.judge(ys[sel], xs[tok[sel]], ebits[e], dt, f"Experts4bit {dt} expert {e} rows {rows}", rows=sel_rows)
        A.isolated(ys, yb, pair_rows, f"Experts4bit {dt}")
        assert check_gemm_workspaces() is None

        # nf4_swiglu_bnb at 48 rows: the fused launch (every composite route raises)
        I, K, M = A.SWIGLU["I"], A.SWIGLU["K"], A.SWIGLU["M"]
        G, U = _swiglu_pair(coracle, gpu, dt)
        gw, uw = A.swiglu_weights()
        gate, up = BNB._module_nested(gw, I, K, dt, gpu), BNB._module_nested(uw, I, K, dt, gpu, 64, 16)
        (kinds,) = A.kind_sets(M, dt, which)
        xs, base, rows = A.special_x(M, K, dt, A.x_seed(M, K), kinds, [G.bits, U.bits])
        xd, bd = _dev(xs, dt, gpu), _dev(base, dt, gpu)
        g, u = _bits(SG._mt(G, xd, M, 1)), _bits(SG._mt(U, xd, M, 1))
        from nf4_triton_dequantization_amd import kernel

        def unfused(*a, **k):
            raise AssertionError("a composite route answered inside the fused launch's domain")

        monkeypatch.setattr(kernel, "dequantize_nf4_bnb", unfused)
        monkeypatch.setattr(kernel, "nf4_linear_bnb_grouped", unfused)
        h, hb = _bits(nf4_swiglu_bnb(xd, gate, up)), _bits(nf4_swiglu_bnb(bd, gate, up))
        accept(h, g, u, dt, f"nf4_swiglu_bnb {dt} rows {rows}", nonfinite=True)
        A.isolated(h, hb, rows, f"nf4_swiglu_bnb {dt}")
        assert check_gemm_workspaces() is None


@pytest.mark.parametrize("dt", DTS)
def test_finite_rows_python_api(coracle, gpu, monkeypatch, dt):
    """nf4_linear_bnb at M in {1, 32, 33, 128, 129}, one captured-and-replayed call at M = 32,
    Experts4bit.forward and nf4_swiglu_bnb, each judged like the entries beneath them; the
    library's cached workspaces read clean afterwards."""
    _api(coracle, gpu, dt, "finite", monkeypatch)


# =================================================================================================
# non-finite kinds: nan, pinf, ninf
# =================================================================================================
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["nested", "single", "ref"])
@pytest.mark.parametrize("M", A.GEMM_MS)
def test_nonfinite_rows_decode_entries(coracle, gpu, dt, mode, M):
    """A NaN partial travels the split-K hand-offs as a value (bitwise NOT on the wire, never the
    empty entry 0): it must come out as NaN with the error word clear and the workspace zero;
    inf * 0 is NaN, inf * w the infinity of the product's sign."""
    _decode(coracle, gpu, dt, "nonfinite", mode, M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", A.GROUPED_REF["Ms"])
def test_nonfinite_rows_grouped_reference_entry(coracle, gpu, dt, M):
    _grouped_ref(coracle, gpu, dt, "nonfinite", M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M", A.GROUPED_BNB["Ms"])
def test_nonfinite_rows_grouped_bnb_entry(coracle, gpu, dt, M):
    _grouped_bnb(coracle, gpu, dt, "nonfinite", M)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["nested", "single"])
@pytest.mark.parametrize("M", A.MT["Ms"])
def test_nonfinite_rows_row_tiled_entries(coracle, gpu, dt, mode, M):
    _row_tiled(coracle, gpu, dt, "nonfinite", mode, M)


@pytest.mark.parametrize("dt", DTS)
def test_nonfinite_rows_expert_gemm(coracle, gpu, dt):
    _moe(coracle, gpu, dt, "nonfinite")


@pytest.mark.parametrize("dt", DTS)
def test_nonfinite_rows_swiglu(coracle, gpu, dt):
    _swiglu(coracle, gpu, dt, "nonfinite")


@pytest.mark.parametrize("dt", DTS)
def test_nonfinite_rows_python_api(coracle, gpu, monkeypatch, dt):
    _api(coracle, gpu, dt, "nonfinite", monkeypatch)
