"""The LLM.int8 input gradient on the project's kernels: F.int8_linear_dgrad (transposing int8 dequantise + k_hgemm)
and MatMul8bitLt.backward.

* Both routes against the fp64 product G @ W, W the 16-bit dequantised weight, at the project's GEMM tolerance
  |got - exp| <= tol * rms(exp) + tol * |exp| (tol = 2e-2 bf16, 1e-2 fp16, tests/test_hgemm_gpu.py); the hgemm route is
  bit-identical from call to call and out= receives the product.
* Routing: shapes / dtypes / strides outside int8_linear_dgrad_supported give the previous expression's bits; a forced
  "hgemm" on them and a bogus route raise.
* The weight workspace holds W^T after a dgrad: a following gemm_4bit(..., reuse_weight=True) must dequantise again.
* Autograd through Linear8bitLt with a frozen weight: thresholds 0 and 6 (planted outlier columns), 2-D and 3-D inputs,
  fp16 and bf16, a transposed-view grad_output; the bias gradient; no double_quant in a threshold-0 step, one
  int8_linear_dgrad; the training forward's bits are the no_grad forward's.  An fp16-weight layer still gets grad_B."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2e-2, torch.float16: 1e-2}


def _bnb():
    import python_src_quants as bnb
    return bnb


def _F():
    import python_src_quants.functional as F
    return F


def _library(G, CB, SCB):
    """MatMul8bitLt.backward's expression before int8_linear_dgrad (autograd._functions._dequantized_weight + matmul)."""
    return torch.matmul(G, CB.to(G.dtype, copy=True).mul_(SCB.unsqueeze(1).mul(1.0 / 127.0)))


_WEIGHTS = {}


def _weight(dev, N, K, seed=0):
    """(CB, SCB) of a random fp16 weight, computed once per shape and left unchanged."""
    key = (N, K, seed)
    if key not in _WEIGHTS:
        g = torch.Generator(device="cpu").manual_seed(77 * seed + N + 3 * K)
        W = (torch.randn(N, K, generator=g) * 0.05).to(torch.float16).to(dev)
        CB, _, SCB, _, _ = _F().double_quant(W)
        _WEIGHTS[key] = (CB, SCB)
    return _WEIGHTS[key]


def _dequantised(CB, SCB, dtype):
    return CB.to(dtype, copy=True).mul_(SCB.unsqueeze(1).mul(1.0 / 127.0))


def _grad(dev, shape, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(9000 + seed)
    return torch.randn(*shape, generator=g).to(dtype).to(dev)


def _assert_close(got, exp, dtype):
    tol = TOL[dtype]
    rms = exp.pow(2).mean().sqrt().item()
    err = (got.double() - exp).abs()
    bound = tol * rms + tol * exp.abs()
    print(f"max err {err.max().item():.3e}  rms(exp) {rms:.3e}  worst err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("route", ["hgemm", "library"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,N,K", [
    (3, 64, 64),         # smallest supported product
    (130, 192, 336),     # K % 64 != 0, ragged tiles
    (257, 320, 1024),    # multi-tile
    (64, 4096, 256),     # long contraction on a small grid: split-K over the workspace
])
def test_int8_linear_dgrad_routes(dev, route, dtype, rows, N, K):
    F = _F()
    CB, SCB = _weight(dev, N, K)
    G = _grad(dev, (rows, N), dtype)
    assert F.int8_linear_dgrad_supported(G, CB, SCB)
    exp = G.double() @ _dequantised(CB, SCB, dtype).double()
    got = F.int8_linear_dgrad(G, CB, SCB, _route=route)
    assert got.shape == (rows, K) and got.dtype == dtype
    _assert_close(got, exp, dtype)
    if route == "hgemm":
        again = F.int8_linear_dgrad(G, CB, SCB, _route=route)
        assert torch.equal(_bits(got), _bits(again))
    else:
        assert torch.equal(_bits(got), _bits(_library(G, CB, SCB)))
    # without _route the call takes the static route's bits
    static = F.int8_linear_dgrad_static_route(rows, N, K, dtype)
    assert static in F.INT8_DGRAD_ROUTES
    if static == route:
        assert torch.equal(_bits(F.int8_linear_dgrad(G, CB, SCB)), _bits(got))


@pytest.mark.parametrize("route", ["hgemm", "library"])
def test_int8_linear_dgrad_out(dev, route):
    """out= receives the product, for a 3-D gradient as well."""
    F = _F()
    CB, SCB = _weight(dev, 192, 336, seed=1)
    G = _grad(dev, (2, 65, 192), torch.bfloat16, seed=1)
    base = F.int8_linear_dgrad(G, CB, SCB, _route=route)
    assert base.shape == (2, 65, 336)
    out = torch.full((130, 336), -7.0, dtype=torch.bfloat16, device=dev)
    res = F.int8_linear_dgrad(G, CB, SCB, out=out, _route=route)
    assert res.data_ptr() == out.data_ptr() and res.shape == (2, 65, 336)
    assert torch.equal(_bits(out), _bits(base.reshape(130, 336)))


def test_int8_linear_dgrad_routing(dev):
    F = _F()
    # N = 72: not a multiple of k_hgemm's k-tile
    CB, SCB = _weight(dev, 72, 64, seed=2)
    G = _grad(dev, (5, 72), torch.bfloat16, seed=2)
    assert not F.int8_linear_dgrad_supported(G, CB, SCB)
    assert torch.equal(_bits(F.int8_linear_dgrad(G, CB, SCB)), _bits(_library(G, CB, SCB)))
    with pytest.raises(ValueError):
        F.int8_linear_dgrad(G, CB, SCB, _route="hgemm")
    # fp32 gradients
    CB, SCB = _weight(dev, 64, 64, seed=3)
    G32 = _grad(dev, (5, 64), torch.float32, seed=3)
    assert not F.int8_linear_dgrad_supported(G32, CB, SCB)
    assert torch.equal(F.int8_linear_dgrad(G32, CB, SCB), _library(G32, CB, SCB))
    with pytest.raises(ValueError):
        F.int8_linear_dgrad(G32, CB, SCB, _route="hgemm")
    # a non-contiguous CB (a transposed view of a [K, N] int8 matrix)
    CBt, _ = _weight(dev, 128, 64, seed=3)
    CBv = CBt.t()
    assert CBv.shape == (64, 128) and not CBv.is_contiguous()
    Gv = _grad(dev, (5, 64), torch.bfloat16, seed=3)
    assert not F.int8_linear_dgrad_supported(Gv, CBv, SCB)
    assert torch.equal(_bits(F.int8_linear_dgrad(Gv, CBv, SCB)), _bits(_library(Gv, CBv, SCB)))
    with pytest.raises(ValueError):
        F.int8_linear_dgrad(Gv, CBv, SCB, _route="hgemm")
    # an unknown route
    G = _grad(dev, (5, 64), torch.bfloat16, seed=3)
    assert F.int8_linear_dgrad_supported(G, CB, SCB)
    with pytest.raises(ValueError):
        F.int8_linear_dgrad(G, CB, SCB, _route="bogus")
    # no rows: the library expression's (empty) result
    G0 = torch.empty((0, 64), dtype=torch.bfloat16, device=dev)
    assert not F.int8_linear_dgrad_supported(G0, CB, SCB)
    assert F.int8_linear_dgrad(G0, CB, SCB).shape == (0, 64)


def test_int8_dgrad_invalidates_the_forward_weight_workspace(dev):
    """gemm_4bit leaves W in the weight workspace and remembers whose it is; int8_linear_dgrad overwrites it with the
    int8 layer's W^T.  A reuse_weight call after it must dequantise again (fails if _DEQ_META is not invalidated)."""
    F = _F()
    N, K = 192, 320
    g = torch.Generator(device="cpu").manual_seed(4)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    q, st = F.quantize_4bit(W, blocksize=64, quant_type="nf4", compress_statistics=True)
    A = _grad(dev, (130, K), torch.bfloat16, seed=4)
    fresh = F.gemm_4bit(A, q, st, _route="hgemm").clone()
    CB, SCB = _weight(dev, N, K, seed=5)
    G = _grad(dev, (130, N), torch.bfloat16, seed=5)
    F.int8_linear_dgrad(G, CB, SCB, _route="hgemm")
    last = F.gemm_4bit(A, q, st, _route="hgemm", reuse_weight=True)
    assert torch.equal(_bits(fresh), _bits(last))


def _layer(dev, threshold, bias):
    bnb = _bnb()
    torch.manual_seed(11)
    layer = bnb.nn.Linear8bitLt(320, 192, bias=bias, has_fp16_weights=False, threshold=threshold)
    return layer.cuda(dev)               # .cuda() quantises the weight rows to CB / SCB


def _input(dev, shape, dtype, threshold, seed):
    x = _grad(dev, shape, dtype, seed=seed).clamp_(-5.0, 5.0)
    if threshold > 0.0:
        x[..., 5] = 6.0                  # planted outlier columns, at and above the threshold
        x[..., 131] = -7.5
    return x


def _counting(monkeypatch, F, name):
    calls = []
    real = getattr(F, name)

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(F, name, counting)
    return calls


@pytest.mark.filterwarnings("ignore:MatMul8bitLt")
@pytest.mark.parametrize("threshold", [0.0, 6.0])
@pytest.mark.parametrize("shape", [(130, 320), (2, 65, 320)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("noncontig", [False, True])
def test_linear8bitlt_frozen_backward_runs_dgrad(dev, monkeypatch, threshold, shape, dtype, noncontig):
    F = _F()
    layer = _layer(dev, threshold, bias=False)
    x = _input(dev, shape, dtype, threshold, seed=6).requires_grad_(True)
    with torch.no_grad():
        y_inference = layer(x.detach())          # 130 rows: above the decode kernel's limit, the GEMM forward
    dq_calls = _counting(monkeypatch, F, "double_quant")
    dgrad_calls = _counting(monkeypatch, F, "int8_linear_dgrad")
    y = layer(x)
    assert torch.equal(_bits(y), _bits(y_inference))
    if noncontig:
        # the gradient reaches MatMul8bitLt.backward as a transposed view (unit stride along the rows)
        g = _grad(dev, (*shape[:-2], 192, shape[-2]), dtype, seed=7).transpose(-1, -2)
        assert not g.is_contiguous()
    else:
        g = _grad(dev, (*shape[:-1], 192), dtype, seed=7)
    assert g.shape == y.shape
    y.backward(g)
    assert len(dgrad_calls) == 1
    # the gradient is never quantised for a frozen weight; the activations only where the COO outliers are needed
    assert len(dq_calls) == (0 if threshold == 0.0 else 1)
    W = _dequantised(layer.state.CB, layer.state.SCB, dtype)
    exp = g.double() @ W.double()
    assert x.grad.shape == x.shape and x.grad.dtype == dtype
    _assert_close(x.grad, exp, dtype)


@pytest.mark.parametrize("threshold", [0.0, 6.0])
def test_linear8bitlt_frozen_backward_bias_grad(dev, threshold):
    """The bias gradient is MatMul8bitLt.backward's grad_output.sum(0, dtype=bias dtype), bit for bit."""
    dtype = torch.float16
    layer = _layer(dev, threshold, bias=True)
    x = _input(dev, (130, 320), dtype, threshold, seed=8).requires_grad_(True)
    g = _grad(dev, (130, 192), dtype, seed=9)
    layer(x).backward(g)
    W = _dequantised(layer.state.CB, layer.state.SCB, dtype)
    _assert_close(x.grad, g.double() @ W.double(), dtype)
    assert layer.bias.grad is not None and layer.bias.grad.shape == (192,)
    assert torch.equal(_bits(layer.bias.grad), _bits(g.sum(0, dtype=dtype)))


def test_frozen_forward_saves_no_column_half(dev):
    """With a frozen weight the forward keeps no column-quantised activations for backward, threshold or not."""
    from python_src_quants.autograd._functions import MatMul8bitLt
    for threshold in (0.0, 6.0):
        layer = _layer(dev, threshold, bias=False)
        x = _input(dev, (130, 320), torch.float16, threshold, seed=10).requires_grad_(True)
        y = layer(x)
        ctx = y.grad_fn
        assert isinstance(ctx, MatMul8bitLt._backward_cls)
        assert ctx.tensors[0] is None and ctx.tensor_states[0] is None
        if threshold > 0.0:
            assert ctx.tensors[1] is not None and sorted(ctx.tensor_states[1].tolist()) == [5, 131]


def test_fp16_weights_still_get_grad_B(dev, monkeypatch):
    """has_fp16_weights=True: the weight gradient is still the column-quantised int8 product (double_quant runs on the
    gradient in backward), within the worst case of two 8-bit column quantisations, and the input gradient arrives."""
    bnb, F = _bnb(), _F()
    T, K, N = 130, 320, 192
    A = _grad(dev, (T, K), torch.float16, seed=12).requires_grad_(True)
    B = (_grad(dev, (N, K), torch.float16, seed=13) * 0.05).requires_grad_(True)
    g = _grad(dev, (T, N), torch.float16, seed=14)
    state = bnb.MatmulLtState()
    state.has_fp16_weights = True
    dq_calls = _counting(monkeypatch, F, "double_quant")
    y = bnb.matmul(A, B, state=state)
    forward_calls = len(dq_calls)
    y.backward(g)
    assert len(dq_calls) == forward_calls + 1
    assert A.grad is not None and A.grad.shape == (T, K)
    assert B.grad is not None and B.grad.shape == (N, K) and B.grad.abs().sum().item() > 0.0
    # each factor is rounded to the nearest of 127 steps of its column's absmax (error <= absmax / 254), T terms
    mg, ma = g.double().abs().amax(0), A.detach().double().abs().amax(0)
    exp = g.double().t() @ A.detach().double()
    bound = T * (2.0 / 254 + 1.0 / 254 ** 2) * mg[:, None] * ma[None, :] + 2.0 ** -10 * exp.abs()
    err = (B.grad.double() - exp).abs()
    print(f"grad_B worst err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
