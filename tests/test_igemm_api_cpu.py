"""The igemm family's Python and C surface without a GPU: check_matmul's shape table and errors, the vector-wise
quantisation formulas on CPU tensors against numpy, and the two ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _F():
    import python_src_quants.functional as F
    return F


def _i8(*shape):
    return torch.zeros(shape, dtype=torch.int8)


# (shape A, shape B, transposed_A, transposed_B, expected output shape); m = 3, k = 5, n = 7, batch 2
OK = [
    ((3, 5), (5, 7), False, False, (3, 7)),
    ((5, 3), (5, 7), True, False, (3, 7)),
    ((5, 3), (7, 5), True, True, (3, 7)),
    ((3, 5), (7, 5), False, True, (3, 7)),
    ((2, 3, 5), (5, 7), False, False, (2, 3, 7)),
    ((2, 5, 3), (5, 7), True, False, (2, 3, 7)),
    ((2, 5, 3), (7, 5), True, True, (2, 3, 7)),
    ((2, 3, 5), (7, 5), False, True, (2, 3, 7)),
    ((2, 3, 5), (2, 5, 7), False, False, (2, 3, 7)),
    ((2, 5, 3), (2, 5, 7), True, False, (2, 3, 7)),
    ((2, 5, 3), (2, 7, 5), True, True, (2, 3, 7)),
    ((2, 3, 5), (2, 7, 5), False, True, (2, 3, 7)),
]


@pytest.mark.parametrize("sa,sb,ta,tb,sout", OK)
def test_check_matmul_output_shapes(sa, sb, ta, tb, sout):
    assert tuple(_F().check_matmul(_i8(*sa), _i8(*sb), None, ta, tb)) == sout


@pytest.mark.parametrize("sa,sb,ta,tb,sout", OK)
def test_check_matmul_rejects_the_other_transpose(sa, sb, ta, tb, sout):
    """Each valid case read with transposed_A flipped has inner dimensions 3 and 5: ValueError, with the text."""
    with pytest.raises(ValueError, match="Tensor dimensions incorrect for matrix mulitiplication"):
        _F().check_matmul(_i8(*sa), _i8(*sb), None, not ta, tb)


def test_check_matmul_dtype():
    F = _F()
    with pytest.raises(TypeError, match="Expected torch.int8 input tensors A and B"):
        F.check_matmul(torch.zeros(3, 5), _i8(5, 7), None, False, False)
    with pytest.raises(TypeError):
        F.check_matmul(_i8(3, 5), torch.zeros(5, 7, dtype=torch.int32), None, False, False)
    # another expected type
    assert tuple(F.check_matmul(torch.zeros(3, 5), torch.zeros(5, 7), None, False, False,
                                expected_type=torch.float32)) == (3, 7)


def test_check_matmul_out_given():
    F = _F()
    # a regular product: out's shape is returned
    out = torch.zeros(3, 7, dtype=torch.int32)
    assert tuple(F.check_matmul(_i8(3, 5), _i8(5, 7), out, False, False)) == (3, 7)
    # bsi,bso->io: accepted only with out of shape (i, o)
    A, B = _i8(2, 4, 3), _i8(2, 4, 7)
    assert tuple(F.check_matmul(A, B, torch.zeros(3, 7, dtype=torch.int32), False, False)) == (3, 7)
    with pytest.raises(ValueError):
        F.check_matmul(A, B, None, False, False)
    with pytest.raises(ValueError):
        F.check_matmul(A, B, torch.zeros(7, 3, dtype=torch.int32), False, False)
    with pytest.raises(ValueError):
        F.check_matmul(A, _i8(2, 5, 7), torch.zeros(3, 7, dtype=torch.int32), False, False)


def test_batched_igemm_wants_3d():
    with pytest.raises(ValueError, match="Expected 3-dimensional tensors for bmm"):
        _F().batched_igemm(_i8(3, 5), _i8(5, 7))


def test_igemm_contraction_needs_matching_batch_and_sequence():
    with pytest.raises(ValueError):
        _F().igemm(_i8(2, 4, 3), _i8(2, 5, 7), out=torch.zeros(3, 7, dtype=torch.int32))


@pytest.mark.parametrize("sa,sb,sout", [((3, 5), (5, 7), (7, 3)), ((2, 3, 5), (5, 7), (6, 7)),
                                        ((2, 3, 5), (2, 5, 7), (2, 7, 3)), ((2, 3, 5), (2, 5, 7), (3, 2, 7))])
def test_igemm_refuses_an_out_of_the_wrong_shape(sa, sb, sout):
    """A given `out` whose shape is not the product's raises before anything is launched -- also for 3-D x 3-D,
    where a wrong 3-D `out` must not be taken for the bsi,bso->io contraction."""
    F = _F()
    with pytest.raises(ValueError, match="Expected an output tensor of shape"):
        F.igemm(_i8(*sa), _i8(*sb), out=torch.zeros(sout, dtype=torch.int32))
    if len(sa) == 3 and len(sb) == 3:
        with pytest.raises(ValueError, match="Expected an output tensor of shape"):
            F.batched_igemm(_i8(*sa), _i8(*sb), out=torch.zeros(sout, dtype=torch.int32))


# ----------------------------------------------------------------------------- vector-wise quantisation, on the CPU
def _x(seed, shape=(6, 9)):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * 3)


@pytest.mark.parametrize("quant_type", ["vector", "row"])
@pytest.mark.parametrize("dim", [0, 1, -1])
def test_vectorwise_quant_vector(quant_type, dim):
    x = _x(1)
    xq, mx = _F().vectorwise_quant(x, dim=dim, quant_type=quant_type)
    xn = x.numpy()
    emx = np.abs(xn).max(axis=dim, keepdims=True)
    eq = np.rint(xn * (np.float32(127.0) / emx)).astype(np.int8)      # rint: half to even, as torch.round
    assert xq.dtype == torch.int8 and np.array_equal(xq.numpy(), eq)
    assert np.array_equal(mx.numpy(), emx)


def test_vectorwise_quant_linear():
    x = _x(2)
    xq, mx = _F().vectorwise_quant(x, quant_type="linear")
    xn = x.numpy()
    emx = np.abs(xn).max().astype(np.float32)
    assert mx.dtype == torch.float32 and mx.ndim == 0 and mx.item() == emx
    assert np.array_equal(xq.numpy(), np.rint(xn / emx * np.float32(127)).astype(np.int8))


def test_vectorwise_quant_truncated_vector():
    x = _x(3)
    xn = x.numpy().copy()
    xq, mx = _F().vectorwise_quant(x, dim=1, quant_type="truncated-vector")
    emx = np.abs(xn).max(axis=1, keepdims=True) * np.float32(0.7)
    clamped = np.where(np.abs(xn) > emx, emx * np.sign(xn), xn)
    assert np.array_equal(mx.numpy(), emx)
    assert np.array_equal(x.numpy(), clamped)                       # the input is clamped in place
    assert np.array_equal(xq.numpy(), np.rint(clamped / emx * np.float32(127)).astype(np.int8))
    assert (np.abs(xq.numpy()) == 127).sum() > x.shape[0]            # several values per row sit at the cap


def test_vectorwise_quant_zeropoint_and_unknown():
    F = _F()
    x = _x(4)
    xn = x.numpy()
    q, s = F.vectorwise_quant(x, quant_type="zeropoint")
    qx = np.float32(255.0) / (xn.max() - xn.min())
    zp = np.rint(xn.min() * qx)
    # (torch divides a scalar by a tensor through the reciprocal: the scale may sit one ulp off, a code one step)
    assert np.abs(q.numpy() - (np.rint(qx * xn - zp) + zp)).max() <= 1 and np.isclose(s.item(), qx, rtol=1e-6)
    q, s = F.vectorwise_quant(x, dim=1, quant_type="vector-zeropoint")
    qx = np.float32(255.0) / (xn.max(axis=1, keepdims=True) - xn.min(axis=1, keepdims=True))
    zp = np.rint(xn.min(axis=1, keepdims=True) * qx)
    assert np.abs(q.numpy() - (np.rint(qx * xn - zp) + zp)).max() <= 1 and np.allclose(s.numpy(), qx, rtol=1e-6)
    assert np.array_equal(q.numpy(), np.rint(q.numpy()))
    assert F.vectorwise_quant(x, quant_type="nope") is None
    assert F.vectorwise_dequant(q, s, quant_type="nope") is None
    assert F.vectorwise_mm_dequant(q, s, s, quant_type="nope") is None


def test_vectorwise_dequant_vector():
    F = _F()
    x = _x(5)
    xq, mx = F.vectorwise_quant(x, dim=1, quant_type="vector")
    d = F.vectorwise_dequant(xq, mx)
    e = (xq.numpy().astype(np.float32) / np.float32(127) * mx.numpy()).astype(np.float32)
    assert d.dtype == torch.float32 and np.array_equal(d.numpy(), e)
    assert np.abs(d.numpy() - x.numpy()).max() <= np.abs(x.numpy()).max() / 127 * 0.5 + 1e-6


def _prod(seed, m=6, n=7):
    rng = np.random.default_rng(seed)
    xq = torch.from_numpy(rng.integers(-127 * 127 * 9, 127 * 127 * 9, (m, n)).astype(np.int32))
    s1 = torch.from_numpy(rng.random((m, 1)).astype(np.float32) + 0.5)
    s2 = torch.from_numpy(rng.random((1, n)).astype(np.float32) + 0.5)
    return xq, s1, s2


@pytest.mark.parametrize("quant_type", ["vector", "truncated-vector"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_vectorwise_mm_dequant_vector(quant_type, dtype):
    xq, s1, s2 = _prod(6)
    c = np.float32(127)
    e = xq.numpy().astype(np.float32) * (s1.numpy() / c) * (s2.numpy() / c)
    for S1, S2 in ((s1, s2), (s1[None], s2[None])):                 # 3-D statistics of a 2-D product are squeezed
        o = _F().vectorwise_mm_dequant(xq, S1, S2, dtype, quant_type)
        assert o.dtype == dtype and o.shape == xq.shape
        assert np.array_equal(o.numpy(), torch.from_numpy(e).to(dtype).numpy())


def test_vectorwise_mm_dequant_row():
    xq, s1, s2 = _prod(7)
    c = np.float32(127)
    e = xq.numpy().astype(np.float32) * (s1.numpy() * s2.numpy() / (c * c))
    o = _F().vectorwise_mm_dequant(xq, s1, s2, torch.float32, "row")
    assert np.array_equal(o.numpy(), e)


def test_vectorwise_mm_dequant_linear():
    xq, _, _ = _prod(8)
    s1, s2 = torch.tensor(1.75), torch.tensor(0.625)
    c = np.float32(127)
    e = xq.numpy().astype(np.float32) * (np.float32(1.75) * np.float32(0.625) / (c * c))
    o = _F().vectorwise_mm_dequant(xq, s1, s2, torch.float16, "linear")
    assert o.dtype == torch.float16
    assert np.array_equal(o.numpy(), e.astype(np.float16))


def test_quant_product_dequant_round_trip_cpu():
    """The whole vector-wise chain on the CPU with the integer product done by torch: close to the fp32 product."""
    F = _F()
    A, B = _x(9, (8, 64)), _x(10, (64, 12))
    qA, SA = F.vectorwise_quant(A, dim=-1)
    qB, SB = F.vectorwise_quant(B, dim=0)
    out = F.vectorwise_mm_dequant(torch.matmul(qA.double(), qB.double()).to(torch.int32), SA, SB, torch.float32)
    ref = A @ B
    assert (out - ref).abs().max() <= 0.03 * ref.abs().max()


# ----------------------------------------------------------------------------- exports and ABI
def test_python_exports():
    import python_src_quants as bnb
    from python_src_quants import autograd
    for name in ("MatMul8bit", "mm_cublas", "bmm_cublas", "matmul_cublas"):
        assert name in bnb.__all__ and hasattr(bnb, name) and hasattr(autograd, name)
    for name in ("check_matmul", "igemm", "batched_igemm", "vectorwise_quant", "vectorwise_dequant",
                 "vectorwise_mm_dequant", "igemm_rowmajor"):
        assert callable(getattr(bnb.functional, name))


def test_header_declares_the_reference_signatures():
    text = open(os.path.join(ROOT, "include", "bnb_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("void cigemm(void* context, bool transposeA, bool transposeB, int m, int n, int k, void* A, void* B, "
            "void* C, int lda, int ldb, int ldc);") in flat
    assert ("void cbatched_igemm(void* context, bool transposeA, bool transposeB, int m, int n, int k, void* A, "
            "void* B, void* C, int lda, int ldb, int ldc, long strideA, long strideB, long strideC, "
            "int batchCount);") in flat
