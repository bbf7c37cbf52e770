"""The 4-bit input gradient on the project's kernels: F.gemm_4bit_dgrad (transposing dequantise + k_hgemm) and
MatMul4Bit.backward.

* Both routes against the fp64 product G @ dequantize_4bit(W), at the project's GEMM tolerance
  |got - exp| <= tol * rms(exp) + tol * |exp| (tol = 2e-2 bf16, 1e-2 fp16, tests/test_hgemm_gpu.py); the hgemm route is
  bit-identical from call to call.
* Routing: shapes / dtypes outside gemm_4bit_dgrad_supported give the previous expression's bits; a bogus route raises.
* The weight workspace holds W^T after a dgrad: a following gemm_4bit(..., reuse_weight=True) must dequantise again.
* Autograd through LinearNF4: 2-D and 3-D inputs, a non-contiguous grad_output, the bias gradient, and the fp32 path
  unchanged."""
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


def _weight(dev, N, K, dtype, nested, quant_type="nf4", seed=0):
    F = _F()
    g = torch.Generator(device="cpu").manual_seed(77 * seed + N + 3 * K)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype).to(dev)
    q, st = F.quantize_4bit(W, blocksize=64, quant_type=quant_type, compress_statistics=nested)
    Wdq = torch.empty((N, K), dtype=dtype, device=dev)
    F.dequantize_4bit(q, st, out=Wdq)
    return q, st, Wdq


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


@pytest.mark.parametrize("route", ["hgemm", "library"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("rows,N,K", [
    (3, 64, 64),         # smallest supported product
    (130, 192, 328),     # K % 64 != 0, ragged tiles
    (257, 320, 1024),    # multi-tile
    (64, 4096, 256),     # long contraction on a small grid: split-K over the workspace
])
def test_gemm_4bit_dgrad_routes(dev, route, dtype, nested, rows, N, K):
    F = _F()
    q, st, Wdq = _weight(dev, N, K, dtype, nested)
    G = _grad(dev, (rows, N), dtype)
    assert F.gemm_4bit_dgrad_supported(G, st)
    exp = G.double() @ Wdq.double()
    got = F.gemm_4bit_dgrad(G, q, st, _route=route)
    assert got.shape == (rows, K) and got.dtype == dtype
    _assert_close(got, exp, dtype)
    if route == "hgemm":
        again = F.gemm_4bit_dgrad(G, q, st, _route=route)
        assert torch.equal(got.view(torch.int16), again.view(torch.int16))
        # the static route of a supported shape is this one
        assert F.gemm_4bit_dgrad_static_route(rows, N, K, dtype) == "hgemm"
        assert torch.equal(F.gemm_4bit_dgrad(G, q, st).view(torch.int16), got.view(torch.int16))


def test_gemm_4bit_dgrad_out_and_resolved_absmax(dev):
    """out= receives the product; absmax= (resolved fp32 statistics) gives the bits of the in-kernel decode."""
    F = _F()
    q, st, _ = _weight(dev, 192, 328, torch.bfloat16, True, seed=1)
    G = _grad(dev, (2, 65, 192), torch.bfloat16, seed=1)
    base = F.gemm_4bit_dgrad(G, q, st, _route="hgemm")
    assert base.shape == (2, 65, 328)
    out = torch.empty((130, 328), dtype=torch.bfloat16, device=dev)
    res = F.gemm_4bit_dgrad(G, q, st, out=out, absmax=F._absmax_fp32(st), _route="hgemm")
    assert res.data_ptr() == out.data_ptr() and res.shape == (2, 65, 328)
    assert torch.equal(out.view(torch.int16), base.reshape(130, 328).view(torch.int16))


def test_gemm_4bit_dgrad_routing(dev):
    F = _F()
    # N = 72: not a multiple of k_hgemm's k-tile
    q, st, _ = _weight(dev, 72, 64, torch.bfloat16, True, seed=2)
    G = _grad(dev, (5, 72), torch.bfloat16, seed=2)
    assert not F.gemm_4bit_dgrad_supported(G, st)
    # MatMul4Bit.backward's previous expression, on the transposed view of the packed weight that Linear4bit passes
    parent = torch.matmul(G, F.dequantize_4bit(q.t(), st).to(G.dtype).t())
    assert parent.shape == (5, 64)
    assert torch.equal(F.gemm_4bit_dgrad(G, q.t(), st).view(torch.int16), parent.view(torch.int16))
    assert torch.equal(F.gemm_4bit_dgrad(G, q, st).view(torch.int16), parent.view(torch.int16))   # either view: G @ W
    with pytest.raises(ValueError):
        F.gemm_4bit_dgrad(G, q, st, _route="hgemm")
    # fp32 gradients
    q, st, _ = _weight(dev, 64, 64, torch.bfloat16, False, seed=3)
    G32 = _grad(dev, (5, 64), torch.float32, seed=3)
    assert not F.gemm_4bit_dgrad_supported(G32, st)
    parent = torch.matmul(G32, F.dequantize_4bit(q.t(), st).to(G32.dtype).t())
    assert torch.equal(F.gemm_4bit_dgrad(G32, q.t(), st), parent)
    # an unknown route
    G = _grad(dev, (5, 64), torch.bfloat16, seed=3)
    with pytest.raises(ValueError):
        F.gemm_4bit_dgrad(G, q, st, _route="bogus")
    # below GEMM_4BIT_DGRAD_MIN_ROWS the static route is the library expression
    assert F.gemm_4bit_dgrad_static_route(F.GEMM_4BIT_DGRAD_MIN_ROWS, 64, 64, torch.bfloat16) == "hgemm"
    assert F.gemm_4bit_dgrad_static_route(F.GEMM_4BIT_DGRAD_MIN_ROWS - 1, 64, 64, torch.bfloat16) == "library"


def test_dgrad_invalidates_the_forward_weight_workspace(dev):
    """gemm_4bit leaves W in the weight workspace and remembers whose it is; gemm_4bit_dgrad overwrites it with W^T.
    A reuse_weight call after it must dequantise again (fails if _DEQ_META is not invalidated)."""
    F = _F()
    N, K = 192, 320
    q, st, _ = _weight(dev, N, K, torch.bfloat16, True, seed=4)
    A = _grad(dev, (130, K), torch.bfloat16, seed=4)
    G = _grad(dev, (130, N), torch.bfloat16, seed=5)
    first = F.gemm_4bit(A, q, st, _route="hgemm").clone()
    F.gemm_4bit_dgrad(G, q, st, _route="hgemm")
    last = F.gemm_4bit(A, q, st, _route="hgemm", reuse_weight=True)
    assert torch.equal(first.view(torch.int16), last.view(torch.int16))


def _layer(dev, dtype, bias):
    bnb = _bnb()
    torch.manual_seed(11)
    return bnb.nn.LinearNF4(320, 192, bias=bias, compute_dtype=dtype).to(dtype).cuda(dev)


def _dequantised(layer, dtype):
    F = _F()
    st = layer.weight.quant_state
    W = torch.empty(tuple(st.shape), dtype=dtype, device=layer.weight.device)
    F.dequantize_4bit(layer.weight.data, st, out=W)
    return W


@pytest.mark.parametrize("shape", [(130, 320), (2, 65, 320)])
@pytest.mark.parametrize("noncontig", [False, True])
def test_linear_nf4_backward_runs_dgrad(dev, monkeypatch, shape, noncontig):
    F = _F()
    dtype = torch.bfloat16
    layer = _layer(dev, dtype, bias=False)
    calls = []
    real = F.gemm_4bit_dgrad

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(F, "gemm_4bit_dgrad", counting)
    x = _grad(dev, shape, dtype, seed=6).requires_grad_(True)
    y = layer(x)
    if noncontig:
        # the gradient reaches MatMul4Bit.backward as a transposed view (unit stride along the rows)
        g = _grad(dev, (*shape[:-2], 192, shape[-2]), dtype, seed=7).transpose(-1, -2)
        assert not g.is_contiguous()
    else:
        g = _grad(dev, (*shape[:-1], 192), dtype, seed=7)
    assert g.shape == y.shape
    y.backward(g)
    assert len(calls) == 1
    exp = g.double() @ _dequantised(layer, dtype).double()
    assert x.grad.shape == x.shape and x.grad.dtype == dtype
    _assert_close(x.grad, exp, dtype)


def test_linear_nf4_backward_bias_grad(dev):
    dtype = torch.bfloat16
    layer = _layer(dev, dtype, bias=True)
    x = _grad(dev, (130, 320), dtype, seed=8).requires_grad_(True)
    g = _grad(dev, (130, 192), dtype, seed=9)
    layer(x).backward(g)
    _assert_close(x.grad, g.double() @ _dequantised(layer, dtype).double(), dtype)
    exp_b = g.double().sum(0)
    assert layer.bias.grad is not None and layer.bias.grad.shape == (192,)
    # one bf16 rounding of a 130-term sum accumulated in the bias dtype: the GEMM tolerance covers it
    _assert_close(layer.bias.grad, exp_b, dtype)


def test_linear_nf4_fp32_backward_keeps_the_old_path(dev, monkeypatch):
    """fp32 activations: MatMul4Bit.backward keeps dequantize_4bit + torch.matmul (as tests/test_nn_gpu.py checks)."""
    bnb, F = _bnb(), _F()
    torch.manual_seed(2)
    layer = bnb.nn.LinearNF4(256, 128, bias=True).cuda(dev)

    def refuse(*a, **kw):
        raise AssertionError("gemm_4bit_dgrad ran for an fp32 gradient")

    monkeypatch.setattr(F, "gemm_4bit_dgrad", refuse)
    x = torch.randn(9, 256, device=dev, requires_grad=True)
    y = layer(x)
    assert y.dtype == torch.float32
    W = F.dequantize_4bit(layer.weight.data, layer.weight.quant_state).float()
    x2 = x.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.linear(x2, W) + layer.bias.float()
    g = torch.randn_like(y)
    y.backward(g)
    ref.backward(g)
    torch.testing.assert_close(x.grad, x2.grad, atol=1e-4, rtol=1e-4)
