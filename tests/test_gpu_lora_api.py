"""``nf4_linear_lora_bnb``, ``nf4_linear_lora_bnb_grouped`` and ``LoraLinear4bit`` on the GPU
(``-m gpu``): results against the judge of _lora_cases.py, the base term being the float64 product
with ``dequantize_nf4_bnb``'s weights under the suite's GEMM bound; which route a call takes, seen
through a counting wrapper on the C entry -- the fused launch exactly for the routed range, never
for fp32 adapters, a recorded gradient, r = 12 or M = 129, all of which equal the composite --; and
one graph capture of base plus adapter replayed over a changed x."""
import pytest
import torch
import torch.nn.functional as F

from _gemm_bnb_cases import drawn_weight_bnb
from _lora_cases import check, lora_oracle, tol_t

pytestmark = pytest.mark.gpu

DT, TDT = "bf16", torch.bfloat16
N, K = 128, 256


def _module(gpu, seed=0, bias=False):
    from types import SimpleNamespace

    from nf4_triton_dequantization_amd import QuantState

    packed, a1, code2, a2, offset = drawn_weight_bnb(N, K, seed=seed)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    st2 = QuantState(absmax=t(a2), code=t(code2), blocksize=256, dtype=torch.float32)
    qs = QuantState(absmax=t(a1), shape=torch.Size((N, K)), blocksize=64, quant_type="nf4", dtype=TDT,
                    offset=torch.tensor(offset, dtype=torch.float32, device=gpu), state2=st2)
    b = torch.randn(N, generator=torch.Generator().manual_seed(seed + 40)).to(gpu).to(TDT) if bias else None
    return SimpleNamespace(weight=SimpleNamespace(data=t(packed).view(-1, 1), quant_state=qs), out_features=N,
                           in_features=K, bias=b)


_MODS = {}


def _mods(gpu):
    """Three modules over one weight shape (one with a bias), never changed."""
    if not _MODS:
        _MODS["m"] = [_module(gpu, 0), _module(gpu, 1, bias=True), _module(gpu, 2)]
    return _MODS["m"]


def _adapter(gpu, r, seed, dtype=TDT):
    g = torch.Generator().manual_seed(500 + seed)
    A = (torch.randn(r, K, generator=g) / K ** 0.5).to(dtype).to(gpu)
    B = (torch.randn(N, r, generator=g) * 4 / r ** 0.5).to(dtype).to(gpu)  # a delta of the base's size
    return A, B


def _x(gpu, M, seed=0):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(900 + seed + M)).to(TDT).to(gpu)


def _judge(y, x, mod, A, B, scaling, what):
    from nf4_triton_dequantization_amd import dequantize_nf4_bnb

    W = dequantize_nf4_bnb(mod).double()
    xf = x.double()
    base = xf @ W.T
    bound = tol_t(base, xf.abs() @ W.abs().T, DT)
    if mod.bias is not None:
        base = base + mod.bias.double()
        bound = bound + 2.0 ** -8 * base.abs()          # the 16-bit add of the bias: half an ulp of the result
    ref, by = lora_oracle(x, A.to(TDT), B.to(TDT), scaling, DT, base, bound)
    check(y.reshape(ref.shape), ref, by, what)


def _composite(x, mod, A, B, scaling):
    from nf4_triton_dequantization_amd import nf4_linear_bnb

    y = nf4_linear_bnb(x, mod, mod.bias)
    return y + (F.linear(F.linear(x.to(A.dtype), A), B) * scaling).to(y.dtype)


@pytest.fixture
def calls(monkeypatch):
    """The adapters of every nf4_lora_add call, counted on the C entry itself."""
    from nf4_triton_dequantization_amd import _lib

    L = _lib.lib()
    seen, real = [], L.nf4_lora_add

    def counting(x, M, K_, mats, count, *rest):
        seen.append((int(M), int(count)))
        return real(x, M, K_, mats, count, *rest)

    monkeypatch.setattr(L, "nf4_lora_add", counting)
    return seen


@pytest.fixture
def routed_everywhere(monkeypatch):
    from nf4_triton_dequantization_amd import kernel

    monkeypatch.setattr(kernel, "LORA_ROUTED_MIN_M", 1)
    monkeypatch.setattr(kernel, "LORA_ROUTED_MAX_M", 128)


@pytest.mark.parametrize("M", [1, 8, 33, 128])
@pytest.mark.parametrize("r", [16, 64])
def test_fused_route_against_the_judge(gpu, calls, routed_everywhere, M, r):
    from nf4_triton_dequantization_amd import nf4_linear_lora_bnb

    x = _x(gpu, M)
    for mod in _mods(gpu)[:2]:                           # without and with a bias
        A, B = _adapter(gpu, r, seed=r)
        del calls[:]
        with torch.no_grad():
            y = nf4_linear_lora_bnb(x.reshape(1, M, K), mod, A, B, 0.5, mod.bias)
        assert calls == [(M, 1)] and y.shape == (1, M, N) and y.dtype == TDT
        _judge(y, x, mod, A, B, 0.5, f"M={M} r={r} bias={mod.bias is not None}")


@pytest.mark.parametrize("M", [1, 32, 33])
def test_grouped_is_one_launch_for_all_adapters(gpu, calls, routed_everywhere, M):
    from nf4_triton_dequantization_amd import nf4_linear_bnb_grouped, nf4_linear_lora_bnb_grouped

    mods = _mods(gpu)
    biases = [m.bias for m in mods]
    ads = [(*_adapter(gpu, 16, 1), 2.0), None, (*_adapter(gpu, 64, 2), -0.5)]
    x = _x(gpu, M, seed=1)
    with torch.no_grad():
        base = nf4_linear_bnb_grouped(x, mods, biases)
        ys = nf4_linear_lora_bnb_grouped(x, mods, ads, biases)
    assert calls == [(M, 2)]                             # ONE launch for the two adapters
    assert torch.equal(ys[1], base[1])                   # no adapter: the base's result
    for y, mod, ad in zip(ys, mods, ads):
        if ad is not None:
            _judge(y, x, mod, *ad, f"grouped M={M}")
    # a third adapter in fp32 takes the composite beside the launch of the other two
    del calls[:]
    A32, B32 = _adapter(gpu, 16, 3, torch.float32)
    with torch.no_grad():
        ys2 = nf4_linear_lora_bnb_grouped(x, mods, [ads[0], (A32, B32, 1.0), ads[2]], biases)
        want = base[1] + (F.linear(F.linear(x.float(), A32), B32) * 1.0).to(TDT)
    assert calls == [(M, 2)]
    assert torch.equal(ys2[1], want) and torch.equal(ys2[0], ys[0]) and torch.equal(ys2[2], ys[2])


def test_the_committed_range_routes_as_it_says(gpu, calls):
    """Without any patch of the range: M inside [LORA_ROUTED_MIN_M, LORA_ROUTED_MAX_M] always
    reaches the C entry, M outside it never does."""
    from nf4_triton_dequantization_amd import kernel, nf4_linear_lora_bnb

    lo, hi = kernel.LORA_ROUTED_MIN_M, kernel.LORA_ROUTED_MAX_M
    mod = _mods(gpu)[0]
    A, B = _adapter(gpu, 16, 4)
    for M in (1, 8, 32, 33, 64, 128, 129):
        x = _x(gpu, M, seed=2)
        before = len(calls)
        with torch.no_grad():
            y = nf4_linear_lora_bnb(x, mod, A, B, 0.5)
        assert (len(calls) == before + 1) == (lo <= M <= min(hi, 128)), (M, lo, hi)
        assert len(calls) <= before + 1
        _judge(y, x, mod, A, B, 0.5, f"committed range M={M}")


@pytest.mark.parametrize("case", ["fp32", "requires_grad", "r12", "M129"])
def test_outside_the_rules_takes_the_composite(gpu, calls, routed_everywhere, case):
    from nf4_triton_dequantization_amd import nf4_linear_lora_bnb

    M = 129 if case == "M129" else 8
    mod = _mods(gpu)[1]
    x = _x(gpu, M, seed=3)
    A, B = _adapter(gpu, 12 if case == "r12" else 16, 5, torch.float32 if case == "fp32" else TDT)
    if case == "requires_grad":
        A.requires_grad_()
        B.requires_grad_()
        y = nf4_linear_lora_bnb(x, mod, A, B, 0.5, mod.bias)
        assert y.grad_fn is not None
        y.float().sum().backward()
        assert A.grad is not None and B.grad is not None and bool(B.grad.float().abs().sum() > 0)
        y, A, B = y.detach(), A.detach(), B.detach()
    else:
        with torch.no_grad():
            y = nf4_linear_lora_bnb(x, mod, A, B, 0.5, mod.bias)
    assert calls == [], case
    with torch.no_grad():
        want = _composite(x, mod, A, B, 0.5)
    assert y.dtype == want.dtype and torch.equal(y, want), case
    if case != "fp32":                                   # (fp32 adapters: t and u are not rounded to 16 bits)
        _judge(y, x, mod, A, B, 0.5, case)


def test_module_forward_takes_the_launch(gpu, calls, routed_everywhere):
    from nf4_triton_dequantization_amd import Linear4bit, LoraLinear4bit

    g = torch.Generator().manual_seed(6)
    base = Linear4bit.from_float((torch.randn(N, K, generator=g) * 0.05).to(gpu), compute_dtype=TDT,
                                 bias=torch.randn(N, generator=g).to(gpu))
    m = LoraLinear4bit.from_linear4bit(base, r=16, lora_alpha=32)
    assert m.lora_A.weight.device == base.weight.data.device and m.lora_A.weight.dtype == TDT
    x = _x(gpu, 5, seed=4)
    with torch.no_grad():
        y0 = m(x)
        assert calls == [(5, 1)] and torch.equal(y0, base(x))       # zero B: zero delta, through the launch
        A, B = _adapter(gpu, 16, 7)
        m.load_state_dict({"lora_A.weight": A, "lora_B.weight": B}, strict=False)
        y = m(x)
    assert calls == [(5, 1)] * 2
    _judge(y, x, base, A, B, 2.0, "module")


def test_graph_replay_follows_x(gpu, calls, routed_everywhere):
    from nf4_triton_dequantization_amd import nf4_linear_lora_bnb

    mod = _mods(gpu)[1]
    A, B = _adapter(gpu, 16, 8)
    xs = [_x(gpu, 8, seed=10 + i) for i in range(3)]
    with torch.no_grad():
        eager = [nf4_linear_lora_bnb(x, mod, A, B, 0.5, mod.bias).clone() for x in xs]  # (also the warm-up)
        assert not eager[0].equal(eager[1])
        x = xs[0].clone()
        torch.cuda.synchronize()
        del calls[:]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = nf4_linear_lora_bnb(x, mod, A, B, 0.5, mod.bias)
    assert calls == [(8, 1)]
    for i in (1, 2, 0):
        x.copy_(xs[i])
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert y.equal(eager[i]), f"replay {i} differs from the eager call"
        _judge(y, xs[i], mod, A, B, 0.5, f"replay {i}")
