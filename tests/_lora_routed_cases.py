"""Routed cases of nf4_lora_add_routed, shared by test_gpu_lora_routed.py and
test_gpu_multilora_api.py: one case of _lora_cases.py per adapter present (drawn, exact probe or
rounding probe, seeded by the adapter), the rows interleaved as the id vector says, so every
adapter group keeps its own oracle, bound and expected bits.  Rows whose id is outside 0..S-1 are
drawn rows with a base of their own; adapters no row names are drawn too.

``a_pad`` / ``b_pad`` (elements, multiples of 8) put adapter s at A + s * (r * K + a_pad) and
B + s * (N * r + b_pad), the padding filled with the 16-bit NaN pattern 0x7FFF: ``a_stride`` and
``b_stride`` are what the descriptor must name, and ``A`` / ``B`` are strided views of the padded
buffers.  ``poison_absent`` makes everything the launch must not use a NaN: the A, B and scale of
every adapter no valid id names, and the x rows of the rows without an adapter.  No expected output
changes: those rows are the base bit for bit and an absent adapter contributes nothing.  ``scales``
replaces ``scale_of`` (one per adapter)."""
from __future__ import annotations

import numpy as np
import torch

from _lora_cases import TDT, check, drawn_case, exact_case, f32, lora_oracle, rounding_case

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ROUTINGS = ("one", "distinct", "zero_absent", "only_63", "mixed", "all_invalid")


def routing(name, M, S, seed=0):
    """(S, ids) of a named routing; the S asked for is raised where the routing needs more adapters."""
    rng = np.random.default_rng([seed, M, S, ROUTINGS.index(name)])
    if name == "one":
        return S, [S - 1] * M
    if name == "distinct":                      # every row its own adapter, in a fixed shuffled order
        S = max(S, M)
        assert S <= 64
        return S, [int(v) for v in rng.permutation(S)[:M]]
    if name == "zero_absent":
        S = max(S, 3)
        return S, [int(v) for v in rng.integers(1, S, M)]
    if name == "only_63":
        return 64, [63] * M
    if name == "mixed":
        ids = [int(v) for v in rng.integers(0, S, M)]
        bad = (-1, S, INT32_MIN, INT32_MAX)
        for i, p in enumerate(rng.permutation(M)[:max(1, M // 4)]):
            ids[int(p)] = bad[i % 4]
        return S, ids
    assert name == "all_invalid"
    bad = (-1, S, INT32_MIN, INT32_MAX, S + 7, -64)
    return S, [bad[i % 6] for i in range(M)]


def scale_of(a):
    """Adapter a's scale: of both signs, none a power of two."""
    return f32((0.3 + 0.37 * (a % 7)) * (-1.0) ** a)


PAD_BITS = 0x7FFF                                   # a NaN in both 16-bit formats


def _padded(t, pad, dev):
    """[S, a, b] on the device as a view of a buffer [S, a * b + pad] whose padding is PAD_BITS."""
    S, a, b = t.shape
    buf = torch.full((S, a * b + pad), PAD_BITS, dtype=torch.int16)
    buf[:, :a * b] = t.reshape(S, a * b).view(torch.int16)
    view = buf.to(dev).view(t.dtype)[:, :a * b].unflatten(1, (a, b))
    assert view.stride()[1:] == (b, 1) and (S == 1 or view.stride(0) == a * b + pad)
    return view


class Routed:
    """One routed call's inputs on the device with the references of every adapter group."""

    def __init__(self, dev, K, r, N, dt, S, ids, kind="drawn", own_r=None, seed=0, a_pad=0, b_pad=0, poison_absent=False,
                 scales=None):
        self.M, self.K, self.r, self.N, self.dt, self.S, self.kind = len(ids), K, r, N, dt, S, kind
        self.id_list = list(ids)
        own_r = r if own_r is None else own_r           # the adapters' own rank, zero-padded to the stack's r
        self.own_r = own_r
        M = self.M
        x = torch.zeros(M, K, dtype=TDT[dt])
        base = torch.zeros(M, N, dtype=TDT[dt])
        A = torch.zeros(S, r, K, dtype=TDT[dt])
        B = torch.zeros(S, N, r, dtype=TDT[dt])
        self.groups = {}                                 # adapter -> ascending rows
        for m, a in enumerate(ids):
            if 0 <= a < S:
                self.groups.setdefault(a, []).append(m)
        self.none = [m for m, a in enumerate(ids) if not 0 <= a < S]
        self.scales = [0.5 if kind == "exact" else scale_of(a) for a in range(S)] if scales is None else [f32(v) for v in scales]
        assert len(self.scales) == S and a_pad >= 0 and b_pad >= 0 and a_pad % 8 == 0 and b_pad % 8 == 0
        self.a_stride, self.b_stride = r * K + a_pad, N * r + b_pad
        self.want = {}                                   # adapter -> (y_want, v_want) of the probes
        for a in range(S):
            rows = self.groups.get(a)
            n = len(rows) if rows else 1
            if kind == "exact" and rows:
                xa, Aa, Ba, ba, yw, vw = exact_case(n, K, own_r, N, dt, seed + a)
                self.want[a] = (yw, vw)
            elif kind == "rounding" and rows:
                xa, Aa, Ba, ba, yw, vw = rounding_case(n, K, own_r, N, dt, self.scales[a], seed + a)
                self.want[a] = (yw, vw)
            else:
                xa, Aa, Ba, ba = drawn_case(n, K, own_r, N, dt, seed + a)
            A[a, :own_r], B[a, :, :own_r] = Aa, Ba
            if rows:
                x[rows], base[rows] = xa, ba
        if self.none:
            xa, _, _, ba = drawn_case(len(self.none), K, own_r, N, dt, seed + 99)
            x[self.none], base[self.none] = xa, ba
            base[self.none[0], ::2] = -0.0               # a -0 base stays -0
        dev_scales = list(self.scales)
        if poison_absent:                                # NaN values in mapped memory: whatever reads them shows
            for a in range(S):
                if a not in self.groups:
                    A[a], B[a], dev_scales[a] = float("nan"), float("nan"), float("nan")
            if self.none:
                x[self.none] = float("nan")
        self.x, self.base = x.to(dev), base.to(dev)
        self.A = A.to(dev) if not a_pad else _padded(A, a_pad, dev)
        self.B = B.to(dev) if not b_pad else _padded(B, b_pad, dev)
        self.scale = torch.tensor(dev_scales, dtype=torch.float32, device=dev)
        self.ids = torch.tensor(self.id_list, dtype=torch.int32, device=dev)
        self.ref = {}
        for a, rows in self.groups.items():
            xr, br = self.x[rows], self.base[rows]
            Aa, Ba = self.A[a, :own_r], self.B[a, :, :own_r].contiguous()
            self.ref[a] = {"null": lora_oracle(xr, Aa, Ba, self.scales[a], dt)}
            self.ref[a]["inplace"] = self.ref[a]["separate"] = lora_oracle(xr, Aa, Ba, self.scales[a], dt, br)

    def judge(self, y, mode, what=""):
        """Every adapter group within its oracle's bound (the probes: bit for bit); the rows without
        an adapter the base bit for bit -- untouched memory when in place -- or +0 under base NULL."""
        for a, rows in self.groups.items():
            got = y[rows]
            if a in self.want:
                want = self.want[a][1 if mode == "null" else 0].to(y.device)
                bad = got.view(torch.int16) != want.view(torch.int16)
                assert not bool(bad.any()), f"{what} adapter {a}: {int(bad.sum())} of {bad.numel()} outputs differ from the expected bits"
            else:
                check(got, *self.ref[a][mode], f"{what} adapter {a} rows {rows[:4]}..")
        if self.none:
            got = y[self.none].view(torch.int16)
            want = torch.zeros_like(got) if mode == "null" else self.base[self.none].view(torch.int16)
            assert torch.equal(got, want), f"{what}: rows without an adapter ({mode})"
