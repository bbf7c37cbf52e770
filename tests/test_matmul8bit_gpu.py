"""GPU: autograd.MatMul8bit (mm_cublas / bmm_cublas / matmul_cublas), the vector-wise quantised matmul on F.igemm.

Primary check, bit for bit: the integer product is exact and everything around it is torch, so outputs and both
gradients must equal an emulation written out here -- the same F.vectorwise_quant, the product by torch.matmul in
float64 cast to int32, the same F.vectorwise_mm_dequant -- run on the same device.

Secondary check: the reference's own accuracy contract against torch.matmul (ref:tests_pvc/test_matmulqlt.py:46-50,
69-77, 101-104, 126-133, 158-162) at dims (16, 32, 64, 48) with B set by xavier_uniform_, caps unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 127.0


def _bnb():
    import python_src_quants as bnb
    return bnb


def _F():
    import python_src_quants.functional as F
    return F


def _iprod(a, b):
    return torch.matmul(a.double(), b.double()).to(torch.int32)


def _swap(t):
    return t.transpose(-1, -2)


class Emulated(torch.autograd.Function):
    """MatMul8bit with the int8 GEMM replaced by a float64 torch.matmul (exact at these sizes)."""

    @staticmethod
    def forward(ctx, A, B, quant_type="vector"):
        F = _F()
        qA, SA = F.vectorwise_quant(A, dim=-1, quant_type=quant_type)
        qB, SB = F.vectorwise_quant(B, dim=0 if B.dim() == 2 else 1, quant_type=quant_type)
        ctx.save_for_backward(A, B)
        ctx.quant_type = quant_type
        return F.vectorwise_mm_dequant(_iprod(qA, qB), SA, SB, A.dtype, quant_type)

    @staticmethod
    def backward(ctx, g):
        F = _F()
        A, B = ctx.saved_tensors
        qt = ctx.quant_type
        gA = gB = None
        if B.requires_grad:
            if A.dim() == 3 and B.dim() == 2:
                g2 = g.contiguous().view(-1, g.shape[2])
                A2 = A.contiguous().view(-1, A.shape[2])
                qg, Sg = F.vectorwise_quant(g2, dim=0, quant_type=qt)
                qa, Sa = F.vectorwise_quant(A2, dim=0, quant_type=qt)
                gB = F.vectorwise_mm_dequant(_iprod(qa.t(), qg), Sa.t(), Sg, g.dtype, qt)
            else:
                dims = [0, 1] if A.dim() == 3 else [0]
                qg, Sg = F.vectorwise_quant(g, dim=dims, quant_type=qt)
                qa, Sa = F.vectorwise_quant(A, dim=dims, quant_type=qt)
                gB = F.vectorwise_mm_dequant(_iprod(_swap(qa), qg), _swap(Sa), Sg, g.dtype, qt)
        if A.requires_grad:
            dims = [g.dim() - 1]
            qg, Sg = F.vectorwise_quant(g, dim=dims, quant_type=qt)
            qb, Sb = F.vectorwise_quant(B, dim=dims if B.dim() == 3 else [1], quant_type=qt)
            gA = F.vectorwise_mm_dequant(_iprod(qg, _swap(qb)), Sg, _swap(Sb), g.dtype, qt)
        return gA, gB, None


CASES = ["2d", "2d_tA", "2d_tB", "2d_tAtB", "3x2", "3x2_tB", "bmm"]


def make_case(case, dims, dtype, seed, device):
    """Leaves A, B (requires_grad), the views a, b handed to the matmul, and a target, drawn on the CPU from `seed`
    (so a seed means the same data everywhere) in the reference test's order: A, B, target, then xavier on B."""
    d1, d2, d3, d4 = dims
    torch.manual_seed(seed)
    tA, tB = case in ("2d_tA", "2d_tAtB"), case in ("2d_tB", "2d_tAtB", "3x2_tB")
    if case.startswith("2d"):
        sa, sb, st = ((d3, d2) if tA else (d2, d3)), ((d4, d3) if tB else (d3, d4)), (d2, d4)
    elif case == "bmm":
        sa, sb, st = (d1, d2, d3), (d1, d3, d4), (d1, d2, d4)
    else:
        sa, sb, st = (d1, d2, d3), ((d4, d3) if tB else (d3, d4)), (d1, d2, d4)
    A, B, target = torch.randn(sa), torch.randn(sb), torch.randn(st)
    torch.nn.init.xavier_uniform_(B)
    A = A.to(device=device, dtype=dtype).requires_grad_()
    B = B.to(device=device, dtype=dtype).requires_grad_()
    return A, B, (A.t() if tA else A), (B.t() if tB else B), target.to(device=device, dtype=dtype)


def _grads(out, A, B, g):
    gA, gB = torch.autograd.grad(out, (A, B), g)
    return gA, gB


@pytest.mark.parametrize("dims", [(16, 32, 64, 48), (3, 33, 70, 129)], ids=["ref_dims", "odd_dims"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES)
def test_matmul8bit_equals_emulation_bit_for_bit(dev, case, dtype, dims):
    bnb = _bnb()
    fn = bnb.bmm_cublas if case == "bmm" else (bnb.mm_cublas if case.startswith("2d") else bnb.matmul_cublas)
    A, B, a, b, target = make_case(case, dims, dtype, 1, dev)
    out = fn(a, b)
    emu = Emulated.apply(a, b)
    assert out.dtype == dtype and out.shape == target.shape
    assert torch.equal(out, emu)
    g = target                                     # any fixed upstream gradient
    gA, gB = _grads(out, A, B, g)
    eA, eB = _grads(emu, A, B, g)
    assert gA.shape == A.shape and gB.shape == B.shape
    assert torch.equal(gA, eA)
    assert torch.equal(gB, eB)
    # and the quantisation is not vacuous: the result is near, not equal to, the full-precision product
    full = torch.matmul(a, b)
    assert not torch.equal(out, full)
    assert (out.float() - full.float()).abs().max() <= 0.1 * full.float().abs().max() + 0.05


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", ["2d", "2d_tB", "3x2", "bmm"])
def test_matmul8bit_linear_forward(dev, case, dtype):
    A, B, a, b, _ = make_case(case, (16, 32, 64, 48), dtype, 2, dev)
    with torch.no_grad():
        out = _bnb().matmul_cublas(a, b, None, "linear")
        assert torch.equal(out, Emulated.apply(a, b, "linear"))
        assert out.dtype == dtype


@pytest.mark.parametrize("case", ["2d", "3x2_tB", "bmm"])
def test_matmul8bit_precision_16_is_torch_matmul(dev, case):
    A, B, a, b, target = make_case(case, (16, 32, 64, 48), torch.float16, 3, dev)
    out = _bnb().matmul_cublas(a, b, None, "vector", [16, 16, 16])
    assert torch.equal(out, torch.matmul(a, b))
    if case != "3x2_tB":       # (the reference's fallback grad_B of a 2-D B under a 3-D A keeps the batch dimension)
        gA, gB = _grads(out, A, B, target)
        with torch.no_grad():
            assert torch.equal(gA, torch.matmul(target, _swap(b)))
            assert torch.equal(gB, torch.matmul(_swap(a), target))


# ----------------------------------------------------------------------------- the reference's accuracy contract
# Seeds: the emulation above, run on the CPU at dims (16, 32, 64, 48) over seeds 0..19 (fp32 and fp16), stays inside
# every cap; the 2-D output has 1,536 elements, so its 0.1 % cap is 1.5 elements.  CONTRACT_SEED is the first seed of
# that range at which the CPU emulation has no 2-D element at all outside the wide bound (atol 0.035, rtol 0.2), in
# any 2-D case and either dtype: seed 0 (of the twenty, only seed 4 has such an element, one).  The CPU emulation's
# counts at seed 0, elements outside (atol 0.01, rtol 0.1) as fp16 / fp32 -- outside (0.035, 0.2), outside bmm's
# (0.027, 0.2) and outside every gradient bound the count is 0 in every case:
#   2d 7 / 6, 2d_tA 8 / 10, 2d_tB 5 / 6, 2d_tAtB 8 / 7 of 1,536 (cap 1.75 % = 26.9);
#   3x2 109 / 107, 3x2_tB 139 / 135 of 24,576 (cap 430.1); bmm 0 / 0 of 24,576 (cap 1 % = 245.8).
CONTRACT_SEED = 0


def _outside(x, y, atol, rtol):
    return int((~torch.isclose(x, y, atol=atol, rtol=rtol)).sum().item())


def contract_figures(fn, case, dtype, seed, device):
    """The quantities the reference's test bounds, as counts (and the element totals)."""
    A, B, a, b, target = make_case(case, (16, 32, 64, 48), dtype, seed, device)
    out_torch = torch.matmul(a, b)
    out_bnb = fn(a, b)
    fig = {"n": out_bnb.numel(),
           "out_narrow": _outside(out_bnb, out_torch, 0.01, 0.1),
           "out_wide": _outside(out_bnb, out_torch, 0.035, 0.2),
           "out_bmm": _outside(out_bnb, out_torch, 0.027, 0.2)}
    out_bnb.data.copy_(out_torch)
    torch.nn.functional.mse_loss(out_bnb, target).mean().backward()
    gA1, gB1 = A.grad, B.grad
    A.grad = B.grad = None
    torch.nn.functional.mse_loss(out_torch, target).mean().backward()
    gA2, gB2 = A.grad, B.grad
    fig.update(nB=gB1.numel(), gA=_outside(gA1, gA2, 0.015, 0.1), gB_006=_outside(gB1, gB2, 0.06, 0.3),
               gB_010=_outside(gB1, gB2, 0.10, 0.3), gB_018=_outside(gB1, gB2, 0.18, 0.3))
    return fig


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES)
def test_matmul8bit_reference_contract(dev, case, dtype):
    bnb = _bnb()
    fn = bnb.bmm_cublas if case == "bmm" else (bnb.mm_cublas if case.startswith("2d") else bnb.matmul_cublas)
    fig = contract_figures(fn, case, dtype, CONTRACT_SEED, dev)
    print(case, dtype, fig)
    n = fig["n"]
    if case == "bmm":
        assert fig["out_narrow"] < n * 0.01                 # test_matmulqlt.py:101-104
        assert fig["out_bmm"] == 0
    else:
        assert fig["out_narrow"] < n * 0.0175               # :46-50, :158-162
        assert fig["out_wide"] < n * 0.001
    assert fig["gA"] == 0                                   # :70, :127
    assert fig["gB_006"] < fig["nB"] * 0.1                  # :72-77, :129-133
    assert fig["gB_010"] < fig["nB"] * 0.02
    if case.startswith("2d"):
        assert fig["gB_018"] == 0
