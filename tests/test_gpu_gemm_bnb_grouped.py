"""The grouped fused GEMM in bitsandbytes semantics (nf4_gemm_bnb_grouped,
nf4_linear_bnb_grouped) on the GPU (``-m gpu``).

Method: the identity walk of test_gpu_gemm_bnb.py.  With x = rows k0 .. k0+M-1 of the K x K
identity every output is one weight plus exact zeros, so walking k0 over K recovers, for every
weight of the group, the dequantized matrix the kernel multiplied by.  It is compared with the C
oracle's ``dequant_bnb`` / ``dequant_bnb_single`` BY VALUE WITH NO TOLERANCE (-0 == +0 allowed,
NaN never).  After each walk ``nf4_gemm_check_workspace`` is clean and the whole workspace is
back at zero.  The weights of a group (tests/_gemm_bnb_grouped_cases.py) differ in offset, code2
and blocksize2, and test_gemm_bnb_grouped_cases_cpu.py proves on the oracle alone that sharing
any of them between weights, or numbering a weight's blocks from the launch-wide row, changes
every 16-row strip -- so a wrong kernel cannot pass a walk.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nf4_oracle as O
from _gemm_bnb_cases import drawn_weight_bnb
from _gemm_bnb_grouped_cases import SMALL_NS, nested_group, offset_value, single_group
from _gemm_cases import bits_to_f64, cfg_tuple, check_close, check_gemm, gemm_cfgs, gemm_oracle, tol, x_bits

pytestmark = pytest.mark.gpu

FAMILY = {1: "K128", 2: "STREAM", 3: "PERSIST", 4: "XS", 5: "XR", 7: "GEMV"}  # NF4DQ_GEMM_* numbers
GROUPED = {"K128", "PERSIST", "XR"}
WIDE_NS = (4096, 1024, 2048)  # the shape of test_persistent_grouped_gemm: 448 strips against 256 CUs


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _code(dt):
    return O.BF16 if dt == "bf16" else O.F16


def _to_dev(bits, dt, gpu):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu).view(_tdt(dt))


def _starts(K, M):
    return [min(k0, K - M) for k0 in range(0, K, M)]


def _assemble(Y, starts, N, K, M):
    rec = torch.empty((N, K), dtype=Y.dtype, device=Y.device)
    full = K // M
    rec[:, :full * M] = Y[:full].permute(2, 0, 1).reshape(N, full * M)
    if K % M:
        rec[:, K - M:] = Y[-1].t()
    return rec


def _assert_exact(rec, want, what):
    ok = rec == want  # by value: -0 == +0, NaN equal to nothing
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} weights differ "
                             f"({int(torch.isnan(rec.float()).sum())} NaN); first at row {r} column {c}: "
                             f"got {float(rec[r, c])!r} want {float(want[r, c])!r}; rows "
                             f"{sorted(set(bad[:, 0].tolist()))[:8]} columns {sorted(set(bad[:, 1].tolist()))[:8]}")


def _identity(K, dt, gpu):
    return torch.eye(K, dtype=_tdt(dt), device=gpu)


# ---- a group on the device ------------------------------------------------------------------
class Group:
    """The weights of one call on the device, the oracle's matrices beside them."""

    def __init__(self, coracle, gpu, Ns, K, dt, single=False, weights=None, blocksizes=None):
        self.Ns, self.K, self.dt, self.single, self.gpu = tuple(Ns), K, dt, single, gpu
        if weights is None:
            weights = single_group(self.Ns, K) if single else nested_group(self.Ns, K, dt)
        self.weights = weights
        self.bs = list(blocksizes) if blocksizes else [64] * len(Ns)
        self.dev, self.want, self.bits = [], [], []
        self.pad = torch.zeros(64, dtype=torch.uint8, device=gpu)  # non-null pointers for an empty weight's fields
        for w, N, bs in zip(weights, Ns, self.bs):
            if N == 0:  # an empty weight: nothing to dequantize
                self.dev.append(None)
                self.bits.append(np.zeros((0, K), np.uint16))
                self.want.append(torch.empty((0, K), dtype=_tdt(dt), device=gpu))
                continue
            if single:
                packed, absmax = w
                bits = coracle.dequant_bnb_single(packed, absmax, N * K, _code(dt), bs)
                t = [torch.from_numpy(np.array(v)).to(gpu) for v in (packed, absmax)]
            else:
                packed, a1, code2, a2, off, bs2 = w
                bits = coracle.dequant_bnb(packed, a1, code2, a2, offset_value(off), N * K, _code(dt), bs, bs2)
                t = [torch.from_numpy(np.array(v)).to(gpu) for v in (packed, a1, code2, a2)]
                t.append(None if off is None else torch.tensor([off], dtype=torch.float32, device=gpu))
            bits = bits.reshape(N, K)
            assert np.isfinite(bits_to_f64(bits, dt)).all()  # 0 x inf would not be exact
            self.dev.append(t)
            self.bits.append(bits)
            self.want.append(_to_dev(bits, dt, gpu))

    def mats(self, ys):
        from nf4_triton_dequantization_amd import _lib

        arr = (_lib.GemmBnbMat * len(self.Ns))()
        for i, (t, N, y) in enumerate(zip(self.dev, self.Ns, ys)):
            if N == 0:
                p = self.pad.data_ptr()
                arr[i] = _lib.GemmBnbMat(p, 0, p, 0, p, p, 0, None, 64, 16, y, 0)
                continue
            if self.single:
                q, am = t
                arr[i] = _lib.GemmBnbMat(q.data_ptr(), q.numel(), None, 0, None, am.data_ptr(), am.numel(), None,
                                         self.bs[i], 0, y, N)
            else:
                q, a1, c2, a2, off = t
                arr[i] = _lib.GemmBnbMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), c2.data_ptr(),
                                         a2.data_ptr(), a2.numel(), off.data_ptr() if off is not None else None,
                                         self.bs[i], self.weights[i][5], y, N)
        return arr

    def modules(self):
        from nf4_triton_dequantization_amd import QuantState

        mods = []
        for t, N, bs, w in zip(self.dev, self.Ns, self.bs, self.weights):
            if self.single:
                q, am = t
                qs = QuantState(absmax=am, shape=torch.Size((N, self.K)), blocksize=bs, quant_type="nf4",
                                dtype=_tdt(self.dt))
            else:
                q, a1, c2, a2, off = t
                st2 = QuantState(absmax=a2, code=c2, blocksize=w[5], dtype=torch.float32)
                qs = QuantState(absmax=a1, shape=torch.Size((N, self.K)), blocksize=bs, quant_type="nf4",
                                dtype=_tdt(self.dt), offset=None if off is None else off.reshape(()), state2=st2)
            mods.append(SimpleNamespace(weight=SimpleNamespace(data=q.view(-1, 1), quant_state=qs), out_features=N,
                                        in_features=self.K, bias=None))
        return mods


def _walk_cfg(L, _lib, eye, grp, M, cfg, accept=(0,)):
    """Every weight of the group recovered through nf4_gemm_bnb_grouped with `cfg` (None = the
    library's choice); or the return code if the first call answers one not in `accept`.  After
    the walk: the split-K error word clean (it is sticky) and the whole workspace back at 0."""
    K, Ns = grp.K, grp.Ns
    starts = _starts(K, M)
    Ys = [torch.full((len(starts), M, N), float("nan"), dtype=eye.dtype, device=eye.device) for N in Ns]
    cp = ctypes.byref(cfg) if cfg is not None else None
    single = 1 if grp.single else 0
    arr = grp.mats([0] * len(Ns))
    mp = ctypes.cast(arr, ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_grouped_workspace_bytes(M, K, mp, len(Ns), single, cp)
    ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=eye.device)
    sp = torch.cuda.current_stream().cuda_stream
    for s, k0 in enumerate(starts):
        for i, Y in enumerate(Ys):
            arr[i].y = Y[s].data_ptr() if Ns[i] else eye.data_ptr()  # an empty weight: any non-null pointer
        rc = L.nf4_gemm_bnb_grouped(eye.data_ptr() + k0 * K * 2, M, K, mp, len(Ns), single,
                                    _lib.BF16 if grp.dt == "bf16" else _lib.F16, ws.data_ptr() if wsz else None, wsz,
                                    cp, sp)
        if rc not in accept and s == 0:
            return rc
        assert rc == 0, (cfg and cfg_tuple(cfg), k0, _lib.strerror(rc))
    assert L.nf4_gemm_check_workspace(ws.data_ptr() if wsz else None, wsz, sp) == 0, cfg and cfg_tuple(cfg)
    if wsz:
        assert int(ws.count_nonzero()) == 0, f"tickets or slab entries left set, cfg {cfg and cfg_tuple(cfg)}"
    return [_assemble(Y, starts, N, K, M) for Y, N in zip(Ys, Ns)]


def _walk_linear(eye, mods, Ns, K, M):
    from nf4_triton_dequantization_amd import nf4_linear_bnb_grouped

    starts = _starts(K, M)
    outs = [nf4_linear_bnb_grouped(eye[k0:k0 + M], mods) for k0 in starts]
    return [_assemble(torch.stack([o[i] for o in outs]), starts, N, K, M) for i, N in enumerate(Ns)]


def _assert_group_exact(recs, grp, what):
    assert isinstance(recs, list), f"{what}: rejected with code {recs}"
    for i, (rec, want) in enumerate(zip(recs, grp.want)):
        _assert_exact(rec, want, f"{what}, weight {i}")


class _RefGroupedAccepts:
    """Which cfgs nf4_gemm_bnb_grouped must accept for a group: a family with the grouped mode
    and a decomposition nf4_gemm_ref_grouped itself accepts there (asked of that entry with one
    real launch on reference-mode statistics of full size, so nothing wraps)."""

    def __init__(self, L, _lib, Ns, K, dt, gpu):
        self.L, self._lib, self.Ns, self.K, self.dt = L, _lib, Ns, K, dt
        bpr = K // 64
        self.t = [(torch.zeros(N * K // 2, dtype=torch.uint8, device=gpu),
                   torch.ones(N * bpr, dtype=torch.uint8, device=gpu),
                   torch.ones(N * (-(-bpr // 4)), dtype=torch.float32, device=gpu),
                   torch.empty((32, N), dtype=_tdt(dt), device=gpu)) for N in Ns]
        self.x = torch.zeros((32, K), dtype=_tdt(dt), device=gpu)
        self.mats = (_lib.GemmMat * len(Ns))()
        for i, ((q, a1, a2, y), N) in enumerate(zip(self.t, Ns)):
            self.mats[i] = _lib.GemmMat(q.data_ptr(), q.numel(), a1.data_ptr(), a1.numel(), a2.data_ptr(), a2.numel(),
                                        y.data_ptr(), N)

    def __call__(self, cfg, M):
        L, _lib = self.L, self._lib
        if FAMILY.get(cfg.kernel) not in GROUPED:
            return False
        wsz = L.nf4_gemm_grouped_workspace_bytes(M, self.K, self.mats, len(self.Ns), ctypes.byref(cfg))
        ws = torch.zeros(max(wsz, 16), dtype=torch.uint8, device=self.x.device)
        rc = L.nf4_gemm_ref_grouped(self.x.data_ptr(), M, self.K, self.mats, len(self.Ns),
                                    _lib.BF16 if self.dt == "bf16" else _lib.F16, ws.data_ptr() if wsz else None, wsz,
                                    ctypes.byref(cfg), torch.cuda.current_stream().cuda_stream)
        assert rc in (0, _lib.ERR_ARG), (cfg_tuple(cfg), _lib.strerror(rc))
        return rc == 0


# ---- the small group ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [5, 32])
def test_small_group_every_accepted_cfg_recovers_exact_weights(coracle, gpu, dt, M):
    """Ns = (64, 192, 64), K = 1024: every entry of the shared decomposition list.  The grouped
    entry accepts exactly those of a family with the grouped mode that nf4_gemm_ref_grouped
    accepts for the group (every other one: ERR_ARG), K128 and XR among them and the persistent
    kernel at M = 5, and every accepted one recovers every weight exactly."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    K = 1024
    grp = Group(coracle, gpu, SMALL_NS, K, dt)
    eye = _identity(K, dt, gpu)
    expected = _RefGroupedAccepts(L, _lib, SMALL_NS, K, dt, gpu)
    ran = {}
    for cfg in gemm_cfgs(K, M):
        recs = _walk_cfg(L, _lib, eye, grp, M, cfg)
        accepted = isinstance(recs, list)
        assert accepted or recs == _lib.ERR_ARG, (cfg_tuple(cfg), recs)
        assert accepted == expected(cfg, M), f"accepted {accepted}: {FAMILY[cfg.kernel]} {cfg_tuple(cfg)} M={M}"
        if not accepted:
            continue
        _assert_group_exact(recs, grp, f"{FAMILY[cfg.kernel]} cfg {cfg_tuple(cfg)} M={M} {dt}")
        ran[FAMILY[cfg.kernel]] = ran.get(FAMILY[cfg.kernel], 0) + 1
    print(f"grouped bnb exact {dt} M={M}: configurations run {ran}")
    assert set(ran) <= GROUPED, ran
    for fam in ("K128", "XR") + (("PERSIST",) if M == 5 else ()):
        assert ran.get(fam, 0) >= 1, (fam, ran)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 4, 12, 17, 32])
def test_small_group_library_choice_through_the_module_entry(coracle, gpu, dt, M):
    """Ns = (64, 192, 64), K = 2048 through nf4_linear_bnb_grouped: the library's choice."""
    K = 2048
    grp = Group(coracle, gpu, SMALL_NS, K, dt)
    recs = _walk_linear(_identity(K, dt, gpu), grp.modules(), SMALL_NS, K, M)
    _assert_group_exact(recs, grp, f"library choice M={M} {dt}")


# ---- a weight boundary inside a workgroup's walk --------------------------------------------
@pytest.fixture(scope="module")
def wide_group(coracle, gpu):
    """Ns = (4096, 1024, 2048), K = 4096, bf16: built once, shared and unchanged."""
    return Group(coracle, gpu, WIDE_NS, 4096, "bf16"), _identity(4096, "bf16", gpu)


@pytest.mark.parametrize("M,cfg", [(16, None), (16, (3, 8, 2, 2, 4)), (8, (3, 8, 2, 1, 1)), (32, None),
                                   (32, (5, 16, 2, 1, 2))])
def test_weight_boundary_inside_a_workgroups_walk(wide_group, M, cfg):
    """448 strips against 256 CUs: a workgroup's strips (persistent: strip groups j0, j0 + G, ...;
    register-resident: per_wg consecutive strips) lie in more than one weight, each with its own
    offset, code2 and blocksize2.  M = 16: the library's choice (persistent, two K slices, two
    strip groups per workgroup) and an explicit persistent cfg with K slices; M = 8: the
    persistent kernel over whole K, one strip per group (448 groups over 256 workgroups);
    M = 32: the library's choice and an explicit register-resident cfg (16 waves, no K slices)."""
    from nf4_triton_dequantization_amd import _lib

    grp, eye = wide_group
    c = _lib.GemmCfg(*cfg) if cfg else None
    recs = _walk_cfg(_lib.lib(), _lib, eye, grp, M, c)
    _assert_group_exact(recs, grp, f"wide group M={M} cfg {cfg}")


# ---- single mode ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_single_mode_group(coracle, gpu, dt):
    """Three weights with fp32 absmax, K = 2048: the library's choice at M = 1, 8, 17 through
    nf4_linear_bnb_grouped, and one explicit cfg per family through the C entry."""
    from nf4_triton_dequantization_amd import _lib

    K = 2048
    grp = Group(coracle, gpu, SMALL_NS, K, dt, single=True)
    eye = _identity(K, dt, gpu)
    mods = grp.modules()
    for M in (1, 8, 17):
        _assert_group_exact(_walk_linear(eye, mods, SMALL_NS, K, M), grp, f"single library choice M={M} {dt}")
    for M, cfg in ((5, (_lib.GEMM_K128, 4, 2, 2, 1)), (5, (_lib.GEMM_PERSIST, 4, 2, 1, 1)),
                   (17, (_lib.GEMM_XR, 8, 2, 1, 2))):
        recs = _walk_cfg(_lib.lib(), _lib, eye, grp, M, _lib.GemmCfg(*cfg))
        _assert_group_exact(recs, grp, f"single cfg {cfg} M={M} {dt}")


# ---- block sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 8])
def test_blocksize_128_and_4096_in_one_group(coracle, gpu, dt, M):
    """blocksize 128, 4096 (a 4096-block spans four rows of K = 1024) and 64 in one nested group
    (blocksize2 4, 4, 256): the 128-deep kernel, each weight with its own shift."""
    Ns, K, bss, bs2s = (64, 128, 64), 1024, (128, 4096, 64), (4, 4, 256)
    ws = []
    for i, (N, bs, bs2) in enumerate(zip(Ns, bss, bs2s)):
        packed, a1, code2, a2, off = drawn_weight_bnb(N, K, seed=90 + i, blocksize=bs, blocksize2=bs2)
        ws.append((packed, a1, code2, a2, (0.0123, None, 0.05)[i], bs2))
    grp = Group(coracle, gpu, Ns, K, dt, weights=ws, blocksizes=bss)
    recs = _walk_linear(_identity(K, dt, gpu), grp.modules(), Ns, K, M)
    _assert_group_exact(recs, grp, f"blocksizes {bss} M={M} {dt}")


# ---- an empty weight ------------------------------------------------------------------------
def test_empty_weight_owns_nothing(coracle, gpu):
    """An N == 0 weight in a K128-cfg group is accepted and owns nothing (its neighbours come out
    exact); the same group under a persistent cfg answers ERR_SHAPE, as in reference mode."""
    from nf4_triton_dequantization_amd import _lib

    K, dt, M = 1024, "bf16", 5
    full = nested_group(SMALL_NS, K, dt)
    grp = Group(coracle, gpu, (64, 0, 64), K, dt, weights=(full[0], None, full[2]))
    eye = _identity(K, dt, gpu)
    recs = _walk_cfg(_lib.lib(), _lib, eye, grp, M, _lib.GemmCfg(_lib.GEMM_K128, 4, 2, 2, 1))
    assert isinstance(recs, list), recs
    _assert_exact(recs[0], grp.want[0], "weight before the empty one")
    _assert_exact(recs[2], grp.want[2], "weight after the empty one")
    assert recs[1].numel() == 0
    rc = _walk_cfg(_lib.lib(), _lib, eye, grp, M, _lib.GemmCfg(_lib.GEMM_PERSIST, 4, 2, 1, 2))  # valid at K = 1024
    assert rc == _lib.ERR_SHAPE, rc


# ---- the offsets live on the device ---------------------------------------------------------
@pytest.mark.parametrize("M", [1, 8, 32])
def test_offsets_are_read_on_the_device_at_every_call(coracle, gpu, M):
    """After one walk, weight 1's offset is changed in place on the device; the next walk's
    weights follow it and only that weight changes: nothing was cached or read on the host."""
    K, dt = 2048, "bf16"
    grp = Group(coracle, gpu, SMALL_NS, K, dt)
    eye, mods = _identity(K, dt, gpu), grp.modules()
    _assert_group_exact(_walk_linear(eye, mods, SMALL_NS, K, M), grp, f"first offsets M={M}")
    new = float(np.float32(0.0625))
    mods[1].weight.quant_state.offset.fill_(new)
    w = grp.weights[1]
    bits = coracle.dequant_bnb(w[0], w[1], w[2], w[3], new, SMALL_NS[1] * K, _code(dt), 64, w[5]).reshape(SMALL_NS[1], K)
    want1 = _to_dev(bits, dt, gpu)
    assert not bool((want1 == grp.want[1]).all())
    recs = _walk_linear(eye, mods, SMALL_NS, K, M)
    _assert_exact(recs[0], grp.want[0], f"weight 0 after weight 1's offset changed, M={M}")
    _assert_exact(recs[1], want1, f"weight 1 with its new offset, M={M}")
    _assert_exact(recs[2], grp.want[2], f"weight 2 after weight 1's offset changed, M={M}")


# ---- the product's own quantizer: random x, biases, fall-backs, capture ---------------------
def _oracle_bits_of(coracle, mod, dt):
    qs = mod.weight.quant_state
    N, K = int(mod.out_features), int(mod.in_features)
    if getattr(qs, "state2", None) is None:
        return coracle.dequant_bnb_single(mod.weight.data.view(-1).cpu().numpy(), qs.absmax.cpu().numpy(), N * K,
                                          _code(dt), int(qs.blocksize)).reshape(N, K)
    return coracle.dequant_bnb(mod.weight.data.view(-1).cpu().numpy(), qs.absmax.cpu().numpy(),
                               qs.state2.code.cpu().numpy(), qs.state2.absmax.cpu().numpy(), float(qs.offset),
                               N * K, _code(dt), int(qs.blocksize), int(qs.state2.blocksize)).reshape(N, K)


def _from_float(gpu, N, K, dt, seed, nested=True, bias=True):
    from nf4_triton_dequantization_amd import Linear4bit

    wf = torch.from_numpy(O.normal_f32(seed, N * K, stream=9).reshape(N, K)).to(gpu) * 0.05
    b = torch.from_numpy(O.normal_f32(seed + 1, N, stream=9)).to(gpu) if bias else None
    return Linear4bit.from_float(wf, compute_dtype=_tdt(dt), bias=b, compress_statistics=nested)


@pytest.fixture(scope="module")
def float_modules(gpu):
    """Three quantized modules per dtype (N = 256, 128, 64; K = 1024; with biases), shared and unchanged."""
    K = 1024
    return {dt: [_from_float(gpu, N, K, dt, 100 + 10 * i) for i, N in enumerate((256, 128, 64))]
            for dt in ("bf16", "f16")}, K


def _with_bias(ref, bound, bias64, dt):
    """y = RNE16(RNE16(x . W^T) + b): the oracle plus the bias, and the GEMM's bound plus the
    one more rounding of the 16-bit add (half an ulp of the result), as test_gpu_gemm_bnb.py."""
    p = 8 if dt == "bf16" else 11
    exp = ref + bias64[None, :]
    return exp, bound + 2.0 ** -p * np.abs(exp)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_random_x_against_the_float64_oracle(coracle, gpu, float_modules, dt):
    """x [2, 3, K] (M = 6): without biases through check_gemm, the suite's own tolerance; with
    the modules' biases against the oracle plus the bias; shapes and dtypes right."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_grouped

    mods_by_dt, K = float_modules
    mods = mods_by_dt[dt]
    xt, xb = x_bits(6, K, dt, seed=3)
    x = xt.to(gpu).reshape(2, 3, K)
    with torch.no_grad():
        plain = nf4_linear_bnb_grouped(x, mods)
        biased = nf4_linear_bnb_grouped(x, mods, [m.bias for m in mods])
    for i, mod in enumerate(mods):
        N = int(mod.out_features)
        wb = _oracle_bits_of(coracle, mod, dt)
        for y in (plain[i], biased[i]):
            assert y.shape == (2, 3, N) and y.dtype == _tdt(dt)
        check_gemm(plain[i].reshape(6, N), xb, wb, dt, f"grouped, weight {i} {dt}")
        ref, bound = gemm_oracle(xb, wb, dt)
        b16 = mod.bias.detach().to(_tdt(dt)).view(torch.int16).cpu().numpy().view(np.uint16)
        exp, bound = _with_bias(ref, bound, bits_to_f64(b16, dt), dt)
        yb = biased[i].reshape(6, N).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        check_close(bits_to_f64(yb, dt), exp, bound, f"grouped with bias, weight {i} {dt}")


def _per_module(x, mods, biases=None):
    from nf4_triton_dequantization_amd import nf4_linear_bnb

    biases = biases or [None] * len(mods)
    return [nf4_linear_bnb(x, m, b) for m, b in zip(mods, biases)]


def test_fallbacks_give_the_per_module_results(coracle, gpu, float_modules, monkeypatch):
    """A mixed nested and single group, different in_features, nine modules and M = 40 each give
    what nf4_linear_bnb gives per module -- and never reach the grouped entry."""
    from nf4_triton_dequantization_amd import _lib, nf4_linear_bnb_grouped

    mods_by_dt, K = float_modules
    dt = "bf16"
    mods = mods_by_dt[dt]
    x = x_bits(6, K, dt, seed=5)[0].to(gpu)
    single = _from_float(gpu, 64, K, dt, 300, nested=False, bias=False)
    other_k = _from_float(gpu, 64, 2 * K, dt, 310, bias=False)
    cases = {"mixed nested and single": (x, [mods[0], single, mods[2]]),
             "nine modules": (x, [mods[i % 3] for i in range(9)]),
             "M = 40": (x_bits(40, K, dt, seed=6)[0].to(gpu), mods)}
    handle, calls = _lib.lib(), []

    class _Spy:  # the loaded library, noting every lookup of the grouped entry
        def __getattr__(self, name):
            if name == "nf4_gemm_bnb_grouped":
                calls.append(name)
            return getattr(handle, name)

    with torch.no_grad():
        want = {k: _per_module(xx, mm) for k, (xx, mm) in cases.items()}
        monkeypatch.setattr(_lib, "lib", lambda: _Spy())
        for k, (xx, mm) in cases.items():
            got = nf4_linear_bnb_grouped(xx, mm)
            assert len(got) == len(mm)
            for g, w in zip(got, want[k]):
                assert torch.equal(g, w), k
        assert not calls, calls
        # different in_features: per module, where the module that does not fit x raises as nf4_linear_bnb does
        with pytest.raises(RuntimeError, match="features"):
            nf4_linear_bnb_grouped(x, [mods[0], other_k])
        got = nf4_linear_bnb_grouped(x, mods)  # ... and the spy does see a group that fuses
        assert calls == ["nf4_gemm_bnb_grouped"] and len(got) == 3


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gradients_take_the_differentiable_path(coracle, gpu, float_modules, dt):
    """x.requires_grad_(): every result is differentiable, the forward values are the per-module
    ones, and x.grad = sum_i dy_i @ W_i within the GEMM tolerance."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb_grouped

    mods_by_dt, K = float_modules
    mods = mods_by_dt[dt]
    xt, xb = x_bits(6, K, dt, seed=4)
    x = xt.to(gpu).requires_grad_()
    ys = nf4_linear_bnb_grouped(x, mods)
    gref = np.zeros((6, K))
    gmag = np.zeros((6, K))
    dys = []
    for i, (y, mod) in enumerate(zip(ys, mods)):
        assert y.requires_grad and y.grad_fn is not None
        wb = _oracle_bits_of(coracle, mod, dt)
        check_gemm(y.detach(), xb, wb, dt, f"forward with grad, weight {i} {dt}")
        dyt, dyb = x_bits(6, int(mod.out_features), dt, seed=50 + i)
        dys.append(dyt.to(gpu))
        dy64, w64 = bits_to_f64(dyb, dt), bits_to_f64(wb, dt)
        gref += dy64 @ w64
        gmag += np.abs(dy64) @ np.abs(w64)
    torch.autograd.backward(ys, dys)
    assert x.grad is not None and x.grad.shape == x.shape
    # three 16-bit partial gradients summed in 16 bits: each sum rounds once more
    p = 8 if dt == "bf16" else 11
    bound = tol(gref, gmag, dt) + 3 * 2.0 ** -p * gmag
    check_close(x.grad.double().cpu().numpy(), gref, bound, f"x.grad {dt}")


@pytest.mark.parametrize("M", [1, 8])
def test_grouped_call_is_capturable_and_never_falls_back(gpu, monkeypatch, M):
    """Three from_float modules at decode sizes: with the unfused path made to raise the grouped
    call still runs, and it can be captured into a graph -- a host read of an offset would
    synchronise, which a capture refuses -- whose replay gives the eager result."""
    from nf4_triton_dequantization_amd import Linear4bit, kernel, nf4_linear_bnb_grouped

    K = 2048
    mods = [Linear4bit.from_float(torch.nn.Linear(K, N, bias=True, device=gpu, dtype=torch.bfloat16))
            for N in (256, 64, 128)]
    x = torch.randn((M, K), device=gpu, dtype=torch.bfloat16)

    def unfused(*a, **k):
        raise AssertionError("nf4_linear_bnb_grouped fell back to dequantize + matmul at a decode size")

    monkeypatch.setattr(kernel, "dequantize_nf4_bnb", unfused)
    biases = [m.bias for m in mods]
    with torch.no_grad():
        y0 = nf4_linear_bnb_grouped(x, mods, biases)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ys = nf4_linear_bnb_grouped(x, mods, biases)
        g.replay()
        torch.cuda.synchronize()
    for y, e, N in zip(ys, y0, (256, 64, 128)):
        assert y.shape == (M, N) and bool(torch.isfinite(y.float()).all())
        assert torch.equal(y, e)


# ---- guard bands ----------------------------------------------------------------------------
GUARD = 64 * 1024
PAT = 0xA5


class Guarded:
    """``nbytes`` usable bytes between two guard bands (offset 64 KiB: 256-B aligned), the
    pattern of test_gpu_redzones_bnb.py: a NaN band (0xFF bytes) below, a 0xA5 band above."""

    def __init__(self, nbytes, device, fill=PAT):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + max(self.n, 1),), PAT, dtype=torch.uint8, device=device)
        self.buf[:GUARD].fill_(0xFF)
        if fill != PAT:
            self.buf[GUARD:GUARD + self.n].fill_(fill)

    @classmethod
    def of(cls, arr, device):
        arr = np.ascontiguousarray(arr)
        g = cls(arr.nbytes, device)
        g.src = arr.reshape(-1).view(np.uint8).copy()
        g.buf[GUARD:GUARD + g.n].copy_(torch.from_numpy(g.src))
        return g

    def body(self, dtype=torch.uint8):
        return self.buf[GUARD:GUARD + self.n].view(dtype)

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def bands_intact(self):
        return bool((self.buf[:GUARD] == 0xFF).all()) and bool((self.buf[GUARD + self.n:] == PAT).all())

    def unchanged(self):
        return np.array_equal(self.body().cpu().numpy(), self.src)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [5, 32])
def test_grouped_call_between_guard_bands(coracle, gpu, dt, M):
    """Every weight's packed bytes, statistics, code2, offset and y, x and the workspace lie
    between a NaN band and a 0xA5 band.  After one grouped call (the library's choice): the
    bands intact, the inputs unchanged, the outputs fully written and within the GEMM
    tolerance of the float64 oracle, the workspace all zero."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    K, Ns = 1024, SMALL_NS
    ws_ = nested_group(Ns, K, dt)
    _, xb = x_bits(M, K, dt, seed=40 + M)
    gx = Guarded.of(xb, gpu)
    inputs, ys = {"x": gx}, []
    arr = (_lib.GemmBnbMat * len(Ns))()
    for i, (w, N) in enumerate(zip(ws_, Ns)):
        packed, a1, code2, a2, off, bs2 = w
        g = {"packed": Guarded.of(packed, gpu), "absmax_q": Guarded.of(a1, gpu), "code2": Guarded.of(code2, gpu),
             "absmax2": Guarded.of(a2, gpu)}
        if off is not None:
            g["offset"] = Guarded.of(np.array([off], np.float32), gpu)
        y = Guarded(M * N * 2, gpu, fill=0xFF)  # 0xFFFF: a NaN in both formats -- an unwritten output shows
        ys.append(y)
        arr[i] = _lib.GemmBnbMat(g["packed"].ptr(), packed.size, g["absmax_q"].ptr(), a1.size, g["code2"].ptr(),
                                 g["absmax2"].ptr(), a2.size, g["offset"].ptr() if off is not None else None, 64, bs2,
                                 y.ptr(), N)
        inputs.update({f"{k}[{i}]": v for k, v in g.items()})
    mp = ctypes.cast(arr, ctypes.c_void_p)
    wsz = L.nf4_gemm_bnb_grouped_workspace_bytes(M, K, mp, len(Ns), 0, None)
    ws = Guarded(wsz, gpu, fill=0)
    sp = torch.cuda.current_stream().cuda_stream
    rc = L.nf4_gemm_bnb_grouped(gx.ptr(), M, K, mp, len(Ns), 0, _lib.BF16 if dt == "bf16" else _lib.F16,
                                ws.ptr() if wsz else None, wsz, None, sp)
    torch.cuda.synchronize()
    assert rc == 0, _lib.strerror(rc)
    for name, g in inputs.items():
        assert g.bands_intact(), f"band of {name} overwritten"
        assert g.unchanged(), f"{name} modified"
    assert ws.bands_intact(), "write outside the workspace"
    assert L.nf4_gemm_check_workspace(ws.ptr() if wsz else None, wsz, sp) == 0
    assert int(ws.body().count_nonzero()) == 0, "workspace not all zero"
    for i, (y, w, N) in enumerate(zip(ys, ws_, Ns)):
        assert y.bands_intact(), f"write outside y[{i}]"
        wb = coracle.dequant_bnb(w[0], w[1], w[2], w[3], offset_value(w[4]), N * K, _code(dt), 64, w[5]).reshape(N, K)
        ref, bound = gemm_oracle(xb, wb, dt)
        yb = y.body(torch.int16).cpu().numpy().view(np.uint16).reshape(M, N)
        check_close(bits_to_f64(yb, dt), ref, bound, f"y[{i}] M={M} {dt}")  # NaN (unwritten) fails
