"""The drawn cases of _family_draws.py on the device (``-m gpu``): nf4_gemm_bnb_mt,
nf4_gemm_bnb_mt_swiglu, nf4_gemm_bnb_moe, nf4_gemm_bnb_moe_swiglu and nf4_gemm_bnb_moe_down through
the C ABI, up to 256 experts.  What the draw covers is checked on the CPU by
test_family_draws_cpu.py; here every drawn call of an (entry, dtype) runs in drawn order on ONE
workspace, sized to the largest need of the sequence, zero-filled once and never cleared again -- as
kernel.py's ``_gemm_workspace`` serves calls of different layouts one after another
(``_moe_down_workspace`` for nf4_gemm_bnb_moe_down, whose sequence has a workspace of its own here
too).  For every call:

  * the return code is NF4DQ_OK: a rejected draw fails, nothing is skipped;
  * the output is NaN-prefilled between two sentinel bands of 8 rows, which stay intact; x is followed
    by NaN rows in the same buffer, which never reach the result;
  * afterwards nf4_gemm_check_workspace is clean and the shared workspace reads 0 over its whole
    length, not only over this call's need.  nf4_gemm_bnb_moe_down leaves its 16-bit products behind
    its slabs ("don't-care" by the header), so there: the ticket header, and every byte that no call
    of the sequence so far had as its product scratch, and in its own slabs every row of a pair with
    a valid id (an earlier call of another layout may have left products there: include/nf4_dequant.h);
  * the result is judged by the entry's own judge, imported from its suite -- ``check_gemm``
    (_gemm_cases.py, as test_gpu_gemm_mt.py uses it), ``_check_chain`` (test_gpu_gemm_mt_swiglu.py), ``_check`` of
    test_gpu_gemm_moe.py and of test_gpu_gemm_moe_swiglu.py (rows of invalid ids: zero bits), and for
    nf4_gemm_bnb_moe_down ``_same`` against ``_moe_down_cases.chain`` of what nf4_gemm_bnb_moe stores
    under the same (waves, ksplit), bit for bit -- and those products themselves by test_gpu_gemm_moe.py's
    ``_check``, so the float64 oracle sees these stacks too.  No tolerance of this file's own;
  * the call is issued again at once, on the used workspace, into a fresh NaN-prefilled output: the
    two outputs are equal bit for bit ("a function of the inputs and the cfg alone").

A failure names (entry, dtype, seed, index) and the case's fields.  ``Runner`` is also what
tools/fuzz_gemm.py --semantics family drives with other seeds."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _family_draws as D
import test_gpu_gemm_moe as MOE
import test_gpu_gemm_moe_down as DOWN
import test_gpu_gemm_moe_swiglu as MSG
import test_gpu_gemm_mt_swiglu as SG
from _gemm_cases import check_gemm
from _moe_down_cases import chain, rn16, widen

pytestmark = pytest.mark.gpu

BAND = 8
HEADER = 64 * 1024 + 256
KERNEL = {"mt": 8, "mt_swiglu": 10, "moe": 9, "moe_swiglu": 11, "moe_down": 12}
_tdt = MOE._tdt

_STACKS = {}


def _build(coracle, gpu, spec, dt, up):
    """The device stack of a drawn ``Stack`` (its up half through _UpStack), once per process."""
    key = (spec, dt, up)
    if key not in _STACKS:
        kw = dict(bs2=spec.bs2 or None, shared_code2=spec.code2_stride == 0, null_offset=not spec.offset, pads=spec.pads)
        if up:
            kw["bs2"] = spec.bs2 or 16
            _STACKS[key] = MSG._UpStack(coracle, gpu, spec.mode, spec.E, spec.N, spec.K, dt, **kw)
        else:
            _STACKS[key] = MOE._Stack(coracle, gpu, spec.mode, "drawn", spec.E, spec.N, spec.K, dt, **kw)
    return _STACKS[key]


def _mat(S, e):
    """Expert e of a stack as one weight of the dense entries (nf4_gemm_bnb_mat)."""
    from nf4_triton_dequantization_amd import _lib

    nblk = S.N * S.K // 64
    q = S.t[0][e, :S.N * S.K // 2]
    if S.mode == "single":
        return _lib.GemmBnbMat(q.data_ptr(), q.numel(), None, 0, None, S.t[1][e].data_ptr(), nblk, None, 64, 0, None, S.N)
    _, a1, c2, a2, off = S.t
    return _lib.GemmBnbMat(q.data_ptr(), q.numel(), a1[e].data_ptr(), nblk, c2[0 if S.shared_code2 else e].data_ptr(),
                           a2[e].data_ptr(), -(-nblk // S.bs2), None if S.null_offset else off[e:e + 1].data_ptr(), 64, S.bs2,
                           None, S.N)


class Runner:
    """The calls of one (entry, dtype) on one workspace.  ``prepare`` builds the stacks and the
    workspace for a list of cases; ``run`` issues one case and raises AssertionError if it fails."""

    def __init__(self, entry, dt, coracle, gpu):
        from nf4_triton_dequantization_amd import _lib

        self.entry, self.dt, self.coracle, self.gpu = entry, dt, coracle, gpu
        self._lib, self.L = _lib, _lib.lib()
        self.code = _lib.BF16 if dt == "bf16" else _lib.F16
        self.ws = self.scratch_seen = None
        self.stale_slab_calls = 0  # moe_down: calls that found, before their launch, bytes set in their own slab region

    # -- the pieces of a case ---------------------------------------------------------------------------
    def stacks(self, c):
        S = _build(self.coracle, self.gpu, c.stack, self.dt, False)
        return (S, _build(self.coracle, self.gpu, c.stack.up, self.dt, True)) if c.stack.up else (S,)

    def cfg(self, c):
        return None if c.cfg is None else self._lib.GemmCfg(KERNEL[self.entry], c.cfg[0], 1, c.cfg[1], 2)

    def need(self, c):
        L, cfg, st = self.L, self.cfg(c), self.stacks(c)
        cp = ctypes.byref(cfg) if cfg is not None else None
        if self.entry == "mt":
            return L.nf4_gemm_bnb_mt_workspace_bytes(c.P, c.stack.N, c.stack.K, cp)
        if self.entry == "mt_swiglu":
            return L.nf4_gemm_bnb_mt_swiglu_workspace_bytes(c.P, c.stack.N, c.stack.K, cp)
        descs = (self._lib.MoeExperts * len(st))(*[s.desc() for s in st])
        fn = {"moe": L.nf4_gemm_bnb_moe_workspace_bytes, "moe_swiglu": L.nf4_gemm_bnb_moe_swiglu_workspace_bytes,
              "moe_down": L.nf4_gemm_bnb_moe_down_workspace_bytes}[self.entry]
        return fn(c.P, ctypes.cast(descs, ctypes.c_void_p), cp)

    def prepare(self, cases):
        """One workspace for the whole sequence: zero-filled here, never again."""
        size = max([HEADER] + [self.need(c) for c in cases])
        if self.ws is None or self.ws.numel() < size:
            self.ws = torch.zeros(size, dtype=torch.uint8, device=self.gpu)
            self.scratch_seen = torch.zeros(size, dtype=torch.bool, device=self.gpu)

    def rows(self, c):
        return c.P // c.topk if self.entry == "moe_down" else c.P

    def rw(self, c):
        w = D.routing_weights(c)
        return w if c.rw_dtype == "f32" else rn16(w, self.dt)

    # -- one launch -------------------------------------------------------------------------------------
    def launch(self, c, xbuf, ids, rwt, wsz):
        """The case's call on the shared workspace into a fresh buffer [band | NaN rows | band]."""
        L, _lib, st, cfg = self.L, self._lib, self.stacks(c), self.cfg(c)
        cp = ctypes.byref(cfg) if cfg is not None else None
        R, N = self.rows(c), c.stack.N
        buf = torch.full((BAND + R + BAND, N), 0x5A5B, dtype=torch.int16, device=self.gpu)
        buf[BAND:BAND + R] = torch.full((R, N), float("nan"), dtype=_tdt(self.dt), device=self.gpu).view(torch.int16)
        y = buf[BAND:BAND + R]
        wp = self.ws.data_ptr() if wsz else None
        sp = torch.cuda.current_stream().cuda_stream
        if self.entry == "mt":
            m = _mat(st[0], c.expert)
            if c.stack.mode == "nested":
                rc = L.nf4_gemm_bnb_mt(xbuf.data_ptr(), c.P, m.packed, m.packed_len, m.absmax_q, m.nb, m.code2, m.absmax2, m.n2,
                                       m.offset, 64, m.blocksize2, y.data_ptr(), self.code, N, c.stack.K, wp, wsz, cp, sp)
            else:
                rc = L.nf4_gemm_bnb_mt_single(xbuf.data_ptr(), c.P, m.packed, m.packed_len, m.absmax2, m.n2, 64, y.data_ptr(),
                                              self.code, N, c.stack.K, wp, wsz, cp, sp)
        elif self.entry == "mt_swiglu":
            mats = (_lib.GemmBnbMat * 2)(_mat(st[0], c.expert), _mat(st[1], c.expert))
            rc = L.nf4_gemm_bnb_mt_swiglu(xbuf.data_ptr(), c.P, c.stack.K, ctypes.cast(mats, ctypes.c_void_p),
                                          1 if c.stack.mode == "single" else 0, _lib.ACT_SILU, y.data_ptr(), self.code, wp, wsz,
                                          cp, sp)
        elif self.entry == "moe":
            MOE._call(st[0], xbuf.data_ptr(), ids, c.P, c.x_div, y.data_ptr(), cfg, ws=self.ws)
            rc = 0
        elif self.entry == "moe_swiglu":
            MSG._call(st[0], st[1], xbuf.data_ptr(), ids, c.P, c.x_div, y.data_ptr(), cfg, ws=self.ws)
            rc = 0
        else:
            d = st[0].desc()
            rc = L.nf4_gemm_bnb_moe_down(xbuf.data_ptr(), ids.data_ptr(), c.P, c.x_div, c.topk, rwt.data_ptr(),
                                         _lib.F32 if c.rw_dtype == "f32" else self.code, ctypes.cast(ctypes.pointer(d), ctypes.c_void_p),
                                         y.data_ptr(), self.code, wp, wsz, cp, sp)
        assert rc == _lib.OK, f"rejected: {_lib.strerror(rc)}"
        return buf, y

    def after(self, c, buf, wsz, which, ids_np):
        """Bands, error word and the workspace after a launch."""
        R = self.rows(c)
        sp = torch.cuda.current_stream().cuda_stream
        assert self.L.nf4_gemm_check_workspace(self.ws.data_ptr(), self.ws.numel(), sp) == 0, f"{which}: workspace error word"
        assert bool((buf[:BAND] == 0x5A5B).all()) and bool((buf[BAND + R:] == 0x5A5B).all()), f"{which}: a sentinel band was written"
        if self.entry != "moe_down":
            left = int(self.ws.count_nonzero())
            assert left == 0, f"{which}: {left} bytes of the shared workspace left set (need {wsz} of {self.ws.numel()})"
            return
        scratch_at = wsz - c.P * c.stack.N * 2
        assert scratch_at >= HEADER and scratch_at % 16 == 0
        self.scratch_seen[scratch_at:wsz] = True
        assert int(self.ws[:HEADER].count_nonzero()) == 0, f"{which}: tickets left set"
        left = int((self.ws != 0).logical_and(~self.scratch_seen).sum())
        assert left == 0, f"{which}: {left} bytes outside every product scratch so far left set"
        if scratch_at > HEADER:  # whatever lay there before: the slab rows of this call's valid pairs were read and cleared
            slabs = self.ws[HEADER:scratch_at].view(torch.int32).view(-1, c.P, c.stack.N)
            valid = torch.from_numpy((ids_np >= 0) & (ids_np < c.stack.E)).to(self.gpu)
            left = int(slabs[:, valid].count_nonzero())
            assert left == 0, f"{which}: {left} slab entries of valid pairs left set"

    # -- the judges, each from its entry's own suite ---------------------------------------------------------
    def judge(self, c, y, xbuf, xb, ids_np, what):
        st = self.stacks(c)
        if self.entry == "mt":
            check_gemm(y.view(_tdt(self.dt)), xb, st[0].bits[c.expert], self.dt, what)
        elif self.entry == "mt_swiglu":
            G, U = (SimpleNamespace(bits=s.bits[c.expert]) for s in st)
            SG._check_chain(y.view(_tdt(self.dt)), xb, G, U, self.dt, what)
        elif self.entry == "moe":
            MOE._check(st[0], y.view(_tdt(self.dt)), xb, ids_np, c.x_div, what)
        elif self.entry == "moe_swiglu":
            MSG._check(st[0], st[1], y.view(_tdt(self.dt)), xb, ids_np, c.x_div, what)
        else:
            got = DOWN._bits(y)
            dy = MOE._moe(st[0], xbuf, ids_np, c.x_div, None if c.cfg is None else MOE._cfg(*c.cfg))
            MOE._check(st[0], dy, xb, ids_np, c.x_div, f"{what}: the products of nf4_gemm_bnb_moe on this stack")
            d = DOWN._bits(dy)
            DOWN._same(got, chain(d, ids_np, c.stack.E, self.rw(c), c.topk, self.dt), what)
            assert np.isfinite(widen(got, self.dt)).all(), f"{what}: NaN or inf in y (finite weights, finite x rows)"
            valid = ((ids_np >= 0) & (ids_np < c.stack.E)).reshape(-1, c.topk).any(axis=1)
            assert (got[~valid] == 0).all(), f"{what}: a token without a valid id must be a row of +0 bits"

    def run(self, c):
        what = f"{self.entry} {self.dt} seed {c.seed} case {c.index}"
        try:
            self._run(c, what)
        except AssertionError as e:
            raise AssertionError(f"{what}: {c.fields()}\n{e}") from None

    def _run(self, c, what):
        assert (c.entry, c.dt) == (self.entry, self.dt)
        wsz = self.need(c)
        assert self.ws is not None and wsz <= self.ws.numel(), "prepare() the sequence first"
        M, K = -(-c.P // c.x_div), c.stack.K
        xt, xb = MOE._x(M, K, self.dt)
        xbuf = torch.full((M + 16, K), float("nan"), dtype=_tdt(self.dt), device=self.gpu)
        xbuf[:M] = xt.to(self.gpu)
        ids_np = ids = rwt = None
        if c.routing is not None:
            ids_np = D.routing_ids(c)
            ids = torch.from_numpy(ids_np.astype(np.int32)).to(self.gpu)
        if self.entry == "moe_down":
            rw = self.rw(c)
            rwt = torch.from_numpy(rw.view(np.int16) if rw.dtype == np.uint16 else rw).to(self.gpu)
        if self.entry == "moe_down" and int(self.ws[HEADER:wsz - c.P * c.stack.N * 2].count_nonzero()):
            self.stale_slab_calls += 1  # an earlier call of another layout left its products where this one has its slabs
        buf, y = self.launch(c, xbuf, ids, rwt, wsz)
        self.after(c, buf, wsz, "first call", ids_np)
        buf2, y2 = self.launch(c, xbuf, ids, rwt, wsz)
        self.after(c, buf2, wsz, "second call", ids_np)
        self.judge(c, y, xbuf, xb, ids_np, what)
        assert torch.equal(y, y2), f"the same call on the used workspace gave other bits in {int((y != y2).sum())} elements"


@pytest.mark.parametrize("dt", D.DTYPES)
@pytest.mark.parametrize("entry", D.ENTRIES)
def test_drawn_calls_on_one_workspace(coracle, gpu, entry, dt):
    cases = D.draws(entry, dt, D.TEST_SEED)
    assert len(cases) == D.DEFAULT_CASES
    R = Runner(entry, dt, coracle, gpu)
    R.prepare(cases)
    for c in cases:
        R.run(c)
    if entry == "moe_down":  # the draw has what include/nf4_dequant.h says of one workspace under changing layouts
        assert R.stale_slab_calls > 0, "no call of the sequence found an earlier call's products in its slabs"
