"""``nf4_linear_multilora_bnb``, ``nf4_linear_multilora_bnb_grouped`` and ``MultiLoraLinear4bit`` on the
GPU (``-m gpu``).  ``kernel.MULTILORA_ROUTED_*`` is set through monkeypatch to force each route; a
counting wrapper on the C entry shows which one a call took.  Both routes are judged per adapter
group by _lora_cases.py's oracle over the base the call itself computed (``nf4_linear_bnb``, which
is the same tensor on both routes), for single and grouped calls, int32 and int64 ids and x given
as ``[B, T, K]``; a captured graph of the fused route is replayed with the ids buffer overwritten
in place -- a new routing, then all -1, then all one adapter -- and must match an eager call with
those ids bit for bit; fp32 adapters, a recorded gradient, S = 65 and misaligned views take the
composite."""
import pytest
import torch

from _gemm_bnb_cases import drawn_weight_bnb
from _lora_cases import check, lora_oracle

pytestmark = pytest.mark.gpu

DT, TDT = "bf16", torch.bfloat16
K = 256
NSIZES = (128, 64, 192)
S = 6


def _module(gpu, n, seed=0, bias=False):
    from types import SimpleNamespace

    from nf4_triton_dequantization_amd import QuantState

    packed, a1, code2, a2, offset = drawn_weight_bnb(n, K, seed=seed)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    st2 = QuantState(absmax=t(a2), code=t(code2), blocksize=256, dtype=torch.float32)
    qs = QuantState(absmax=t(a1), shape=torch.Size((n, K)), blocksize=64, quant_type="nf4", dtype=TDT,
                    offset=torch.tensor(offset, dtype=torch.float32, device=gpu), state2=st2)
    b = torch.randn(n, generator=torch.Generator().manual_seed(seed + 40)).to(gpu).to(TDT) if bias else None
    return SimpleNamespace(weight=SimpleNamespace(data=t(packed).view(-1, 1), quant_state=qs), out_features=n,
                           in_features=K, bias=b)


_MODS = {}


def _mods(gpu):
    """Three modules over one K (one with a bias), never changed."""
    if not _MODS:
        _MODS["m"] = [_module(gpu, n, s, bias=(s == 1)) for s, n in enumerate(NSIZES)]
    return _MODS["m"]


def _stack(gpu, n, r, seed, s=S, dtype=TDT):
    g = torch.Generator().manual_seed(700 + seed)
    A = (torch.randn(s, r, K, generator=g) / K ** 0.5).to(dtype).to(gpu)
    B = (torch.randn(s, n, r, generator=g) * 4 / r ** 0.5).to(dtype).to(gpu)  # a delta of the base's size
    scaling = torch.tensor([0.5 + 0.25 * i for i in range(s)], dtype=torch.float32, device=gpu)
    return A, B, scaling


def _x(gpu, M, seed=0):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(900 + seed + M)).to(TDT).to(gpu)


def _ids(gpu, M, seed=0, dtype=torch.int32, s=S):
    ids = torch.randint(-1, s + 1, (M,), generator=torch.Generator().manual_seed(30 + seed + M))
    return ids.to(dtype).to(gpu)


def _judge(y, x, mod, A, B, scaling, ids, what):
    """Per adapter group against the oracle over the base ``nf4_linear_bnb`` gives (both routes start
    from that very tensor); rows without an adapter are that base bit for bit."""
    from nf4_triton_dequantization_amd import nf4_linear_bnb

    with torch.no_grad():
        base = nf4_linear_bnb(x, mod, mod.bias).reshape(-1, y.shape[-1])
    y2, x2, flat = y.reshape(base.shape), x.reshape(-1, K), ids.reshape(-1).tolist()
    for a in range(A.shape[0]):
        rows = [m for m, v in enumerate(flat) if v == a]
        if rows:
            ref, by = lora_oracle(x2[rows], A[a].to(TDT), B[a].to(TDT), float(scaling[a]), DT, base[rows])
            check(y2[rows], ref, by, f"{what} adapter {a}")
    none = [m for m, v in enumerate(flat) if not 0 <= v < A.shape[0]]
    if none:
        assert torch.equal(y2[none].view(torch.int16), base[none].view(torch.int16)), f"{what}: rows without an adapter"


@pytest.fixture
def calls(monkeypatch):
    """(M, adapters, stacks) of every nf4_lora_add_routed call, counted on the C entry itself."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    seen, real = [], L.nf4_lora_add_routed

    def counting(x, ids, M, K_, adapters, stacks, count, *rest):
        seen.append((int(M), int(adapters), int(count)))
        return real(x, ids, M, K_, adapters, stacks, count, *rest)

    monkeypatch.setattr(L, "nf4_lora_add_routed", counting)
    return seen


@pytest.fixture
def fused(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MIN_M", 1)
    monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MAX_M", 128)


@pytest.fixture
def composite(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MIN_M", 1)
    monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MAX_M", 0)


@pytest.mark.parametrize("M", [1, 8, 65, 128])
@pytest.mark.parametrize("r", [16, 64])
def test_both_routes_against_the_judge(gpu, calls, monkeypatch, M, r):
    from nf4_triton_dequantization_amd import kernel, nf4_linear_multilora_bnb

    x = _x(gpu, M)
    for mod in _mods(gpu)[:2]:                           # without and with a bias
        A, B, scaling = _stack(gpu, mod.out_features, r, seed=r)
        for idt in (torch.int32, torch.int64):
            ids = _ids(gpu, M, seed=r, dtype=idt)
            for hi, want_calls in ((128, [(M, S, 1)]), (0, [])):
                monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MIN_M", 1)
                monkeypatch.setattr(kernel, "MULTILORA_ROUTED_MAX_M", hi)
                del calls[:]
                with torch.no_grad():
                    y = nf4_linear_multilora_bnb(x.reshape(1, M, K), mod, A, B, scaling, ids.reshape(1, M), mod.bias)
                assert calls == want_calls and y.shape == (1, M, mod.out_features) and y.dtype == TDT
                _judge(y, x, mod, A, B, scaling, ids, f"M={M} r={r} {idt} fused={bool(hi)}")


@pytest.mark.parametrize("M", [1, 33])
def test_grouped_is_one_launch_for_all_stacks(gpu, calls, fused, M):
    from nf4_triton_dequantization_amd import nf4_linear_bnb_grouped, nf4_linear_multilora_bnb, nf4_linear_multilora_bnb_grouped

    mods = _mods(gpu)
    biases = [m.bias for m in mods]
    stacks = [_stack(gpu, NSIZES[0], 16, 1), None, _stack(gpu, NSIZES[2], 64, 2)]
    x, ids = _x(gpu, M, seed=1), _ids(gpu, M, seed=1, dtype=torch.int64)
    with torch.no_grad():
        base = nf4_linear_bnb_grouped(x, mods, biases)
        ys = nf4_linear_multilora_bnb_grouped(x, mods, stacks, ids, biases)
    assert calls == [(M, S, 2)]                          # ONE launch for the two stacks
    assert torch.equal(ys[1], base[1])                   # no stack: the base's result
    for y, mod, st in zip(ys, mods, stacks):
        if st is not None:
            _judge(y, x, mod, *st, ids, f"grouped M={M}")
    # a stack in fp32 takes the composite beside the launch of the other two
    del calls[:]
    st32 = _stack(gpu, NSIZES[1], 16, 3, dtype=torch.float32)
    with torch.no_grad():
        ys2 = nf4_linear_multilora_bnb_grouped(x, mods, [stacks[0], st32, stacks[2]], ids, biases)
        assert calls == [(M, S, 2)]
        want = nf4_linear_multilora_bnb(x, mods[1], *st32, ids, biases[1])
    assert calls == [(M, S, 2)]
    assert torch.equal(ys2[1], want) and torch.equal(ys2[0], ys[0]) and torch.equal(ys2[2], ys[2])


def test_grouped_composite_agrees(gpu, calls, composite):
    from nf4_triton_dequantization_amd import nf4_linear_multilora_bnb_grouped

    mods = _mods(gpu)
    stacks = [_stack(gpu, NSIZES[0], 16, 1), _stack(gpu, NSIZES[1], 8, 4), _stack(gpu, NSIZES[2], 64, 2)]
    x, ids = _x(gpu, 33, seed=1), _ids(gpu, 33, seed=1)
    with torch.no_grad():
        ys = nf4_linear_multilora_bnb_grouped(x, mods, stacks, ids, [m.bias for m in mods])
    assert calls == []
    for y, mod, st in zip(ys, mods, stacks):
        _judge(y, x, mod, *st, ids, "grouped composite")


def test_the_committed_range_routes_as_it_says(gpu, calls):
    """Without any patch of the range: M inside [MULTILORA_ROUTED_MIN_M, MULTILORA_ROUTED_MAX_M]
    always reaches the C entry, M outside it never does."""
    from nf4_triton_dequantization_amd import kernel, nf4_linear_multilora_bnb

    lo, hi = kernel.MULTILORA_ROUTED_MIN_M, kernel.MULTILORA_ROUTED_MAX_M
    mod = _mods(gpu)[0]
    A, B, scaling = _stack(gpu, mod.out_features, 16, 4)
    for M in (1, 8, 32, 64, 128, 129):
        x, ids = _x(gpu, M, seed=2), _ids(gpu, M, seed=2)
        before = len(calls)
        with torch.no_grad():
            y = nf4_linear_multilora_bnb(x, mod, A, B, scaling, ids)
        assert (len(calls) == before + 1) == (lo <= M <= min(hi, 128)), (M, lo, hi)
        _judge(y, x, mod, A, B, scaling, ids, f"committed range M={M}")


def test_graph_replay_follows_the_ids_buffer(gpu, calls, fused):
    """The capability the feature exists for: one captured launch, the routing read at replay."""
    from nf4_triton_dequantization_amd import nf4_linear_multilora_bnb

    M = 24
    mod = _mods(gpu)[1]
    A, B, scaling = _stack(gpu, mod.out_features, 16, 8)
    x = _x(gpu, M, seed=5)
    routings = [_ids(gpu, M, seed=11), torch.full((M,), -1, dtype=torch.int32, device=gpu),
                torch.full((M,), 4, dtype=torch.int32, device=gpu)]
    first = _ids(gpu, M, seed=12)
    with torch.no_grad():
        eager = [nf4_linear_multilora_bnb(x, mod, A, B, scaling, i, mod.bias).clone() for i in routings]  # (also the warm-up)
        assert not eager[0].equal(eager[1]) and not eager[1].equal(eager[2])
        ids = first.clone()
        torch.cuda.synchronize()
        del calls[:]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = nf4_linear_multilora_bnb(x, mod, A, B, scaling, ids, mod.bias)
    assert calls == [(M, S, 1)]
    for i, r in enumerate(routings):
        ids.copy_(r)                                     # overwritten in place: the graph holds the buffer
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), eager[i].view(torch.int16)), f"replay {i} differs from the eager call"
        _judge(y, x, mod, A, B, scaling, r, f"replay {i}")
    assert calls == [(M, S, 1)]                          # nothing but replays since the capture


@pytest.mark.parametrize("case", ["fp32", "requires_grad", "S65", "misaligned_A", "strided_B", "M129"])
def test_outside_the_rules_takes_the_composite(gpu, calls, fused, case):
    from nf4_triton_dequantization_amd import kernel, nf4_linear_bnb, nf4_linear_multilora_bnb

    M = 129 if case == "M129" else 8
    s = 65 if case == "S65" else S
    mod = _mods(gpu)[1]
    n = mod.out_features
    x = _x(gpu, M, seed=3)
    ids = _ids(gpu, M, seed=3, s=s)
    A, B, scaling = _stack(gpu, n, 16, 5, s=s, dtype=torch.float32 if case == "fp32" else TDT)
    if case == "misaligned_A":                           # a view 2 bytes into a buffer: contiguous, not 16-byte aligned
        buf = torch.zeros(A.numel() + 1, dtype=TDT, device=gpu)
        buf[1:] = A.reshape(-1)
        A = buf[1:].view(A.shape)
        assert A.is_contiguous() and A.data_ptr() % 16
    if case == "strided_B":
        B = torch.cat([B, B], dim=2)[:, :, :16]
        assert not B.is_contiguous()
    if case == "requires_grad":
        A.requires_grad_()
        B.requires_grad_()
        y = nf4_linear_multilora_bnb(x, mod, A, B, scaling, ids, mod.bias)
        assert y.grad_fn is not None
        y.float().sum().backward()
        assert A.grad is not None and B.grad is not None and bool(B.grad.float().abs().sum() > 0)
        y, A, B = y.detach(), A.detach(), B.detach()
    else:
        with torch.no_grad():
            y = nf4_linear_multilora_bnb(x, mod, A, B, scaling, ids, mod.bias)
    assert calls == [], case
    with torch.no_grad():
        want = kernel._multilora_composite(nf4_linear_bnb(x, mod, mod.bias), x, A, B, scaling, ids)
    assert y.dtype == want.dtype and torch.equal(y, want), case
    if case != "fp32":                                   # (fp32 adapters: t and u are not rounded to 16 bits)
        _judge(y, x, mod, A, B, scaling, ids, case)


def test_module_forward_takes_the_launch(gpu, calls, fused):
    from nf4_triton_dequantization_amd import Linear4bit, MultiLoraLinear4bit

    g = torch.Generator().manual_seed(6)
    base = Linear4bit.from_float((torch.randn(128, K, generator=g) * 0.05).to(gpu), compute_dtype=TDT,
                                 bias=torch.randn(128, generator=g).to(gpu))
    ads = [((torch.randn(r, K, generator=g) / K ** 0.5).to(TDT), (torch.randn(128, r, generator=g) * 4 / r ** 0.5).to(TDT), sc)
           for r, sc in ((4, 2.0), (20, 0.5), (8, -1.0))]
    m = MultiLoraLinear4bit.from_linear4bit(base, ads)
    assert m.lora_A.device == base.weight.data.device and m.lora_A.dtype == TDT and m.r == 24 and m.scaling.device == m.lora_A.device
    x = _x(gpu, 10, seed=4).reshape(2, 5, K)
    ids = torch.tensor([[0, 1, 2, -1, 1], [2, 2, 3, 0, 1]], device=gpu)
    with torch.no_grad():
        y = m(x, ids)
        assert calls == [(10, 3, 1)] and y.shape == (2, 5, 128)
        _judge(y, x, base, m.lora_A, m.lora_B, m.scaling, ids, "module")
        for s in range(3):                               # the padding adds nothing: the unpadded adapter's oracle holds
            rows = (ids.reshape(-1) == s).nonzero().reshape(-1)
            xr = x.reshape(-1, K)[rows]
            ref, by = lora_oracle(xr, ads[s][0].to(gpu), ads[s][1].to(gpu), ads[s][2], DT, base(xr))
            check(y.reshape(-1, 128)[rows], ref, by, f"module adapter {s}")
            check(m.adapter(s)(xr), ref, by, f"module adapter({s})")
