"""The transposing int8 row dequantise (csrc/dequant_int8_t.hip, F.dequantize_int8_t) on the GPU.

* Bit-exact against the expression MatMul8bitLt.backward dequantises with, CB.to(T).mul_(SCB.unsqueeze(1).mul(1/127)),
  .t().contiguous(), for bf16 / fp16 on the smallest shape, a ragged single tile, a ragged multi-tile shape and one of
  whole tiles; with row statistics 0, 1e-6 and 65504 and the weight values -127, 127 and 0.
* out= as a window of a wider buffer (ldo > N): nothing outside the window is written.
* A shape the C entry declines (K = 24) still dequantises through the function, to the same bits.
* The C entry returns 1 and writes nothing for ldo < N, a misaligned out and N % 8 != 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (8, 16),        # the smallest
    (72, 48),       # ragged in both directions, one tile
    (200, 336),     # ragged, 4 x 3 tiles
    (320, 1024),    # whole tiles
]
DTYPES = [torch.bfloat16, torch.float16]
POISON = -7.0


def _F():
    import python_src_quants.functional as F
    return F


def _weight(dev, N, K, seed=0):
    """CB over the whole int8 range of the format (-127..127, with the extremes and 0 planted) and positive row
    statistics, three of them the edge values 0, 1e-6 and 65504."""
    g = torch.Generator(device="cpu").manual_seed(100 * seed + N + 7 * K)
    CB = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    CB[0, 0], CB[0, 1], CB[0, 2] = -127, 127, 0
    CB[N - 1, K - 3], CB[N - 1, K - 2], CB[N - 1, K - 1] = 0, 127, -127
    SCB = (torch.rand(N, generator=g) * 3.0 + 0.01).float()
    SCB[1], SCB[N // 2], SCB[N - 2] = 0.0, 1e-6, 65504.0
    # the extremes also against the edge statistics
    CB[1, :3] = torch.tensor([-127, 127, 0], dtype=torch.int8)
    CB[N // 2, :3] = torch.tensor([-127, 127, 0], dtype=torch.int8)
    CB[N - 2, :3] = torch.tensor([-127, 127, 0], dtype=torch.int8)
    return CB.to(dev), SCB.to(dev)


def _reference(CB, SCB, dtype):
    """autograd._functions._dequantized_weight's expression for a stored CB, transposed."""
    return CB.to(dtype, copy=True).mul_(SCB.unsqueeze(1).mul(1.0 / 127.0)).t().contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_dequantize_int8_t_bit_exact(dev, dtype, N, K):
    F = _F()
    CB, SCB = _weight(dev, N, K)
    exp = _reference(CB, SCB, dtype)
    got = F.dequantize_int8_t(CB, SCB, dtype)
    assert got.shape == (K, N) and got.dtype == dtype and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(exp))
    # the kernel itself took the shape (the function did not fall back to the copy)
    probe = torch.full((K, N), POISON, dtype=dtype, device=dev)
    assert F._dequant_int8_t_launch(CB, SCB, probe) == 0
    assert torch.equal(_bits(probe), _bits(exp))
    # the same expression through the autograd module's helper
    from python_src_quants.autograd._functions import MatmulLtState, _dequantized_weight
    st = MatmulLtState()
    st.CB, st.SCB = CB, SCB
    assert torch.equal(_bits(_dequantized_weight(st, dtype).t()), _bits(got))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K", [(72, 48), (200, 336)])
def test_dequantize_int8_t_out_window(dev, dtype, N, K):
    """out = columns [8, 8 + N) of rows [1, K + 1) of a [K + 2, N + 24] buffer: ldo = N + 24 > N, 16-B aligned."""
    F = _F()
    CB, SCB = _weight(dev, N, K, seed=1)
    buf = torch.full((K + 2, N + 24), POISON, dtype=dtype, device=dev)
    win = buf[1:K + 1, 8:8 + N]
    assert win.data_ptr() % 16 == 0 and win.stride(0) % 8 == 0 and win.stride(0) > N
    assert F._dequant_int8_t_launch(CB, SCB, win) == 0          # the kernel takes the window
    buf.fill_(POISON)
    res = F.dequantize_int8_t(CB, SCB, dtype, out=win)
    assert res.data_ptr() == win.data_ptr()
    assert torch.equal(_bits(buf[1:K + 1, 8:8 + N]), _bits(_reference(CB, SCB, dtype)))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[1:K + 1, 8:8 + N] = False
    assert (buf[outside] == POISON).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_int8_t_declined_shape_falls_back(dev, dtype):
    """K = 24 (K % 16 != 0): the C entry returns 1 and writes nothing; the function returns the same bits."""
    F = _F()
    N, K = 72, 24
    CB, SCB = _weight(dev, N, K, seed=2)
    buf = torch.full((K, N), POISON, dtype=dtype, device=dev)
    assert F._dequant_int8_t_launch(CB, SCB, buf) == 1
    torch.cuda.synchronize()
    assert (buf == POISON).all()
    exp = _reference(CB, SCB, dtype)
    assert torch.equal(_bits(F.dequantize_int8_t(CB, SCB, dtype)), _bits(exp))
    F.dequantize_int8_t(CB, SCB, dtype, out=buf)
    assert torch.equal(_bits(buf), _bits(exp))
    # fp32 is the fallback's as well
    assert torch.equal(F.dequantize_int8_t(CB, SCB, torch.float32), _reference(CB, SCB, torch.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_int8_t_entry_declines(dev, dtype):
    """The C entry called by hand: 1, and a poisoned out untouched, for ldo < N, ldo % 8 != 0, a misaligned out,
    N % 8 != 0 and K % 16 != 0."""
    F = _F()
    CB, SCB = _weight(dev, 64, 64, seed=3)
    out = torch.full((128 * 128,), POISON, dtype=dtype, device=dev)
    fn = F.lib.cdequantize_int8_rows_t_bf16 if dtype == torch.bfloat16 else F.lib.cdequantize_int8_rows_t_fp16
    assert out.data_ptr() % 16 == 0 and CB.data_ptr() % 16 == 0
    for rows, cols, ldo in [(64, 64, 56), (64, 64, 68), (12, 64, 16), (60, 64, 64), (64, 24, 64)]:
        assert fn(CB.data_ptr(), SCB.data_ptr(), out.data_ptr(), rows, cols, ldo) == 1, (rows, cols, ldo)
    assert fn(CB.data_ptr(), SCB.data_ptr(), out.data_ptr() + 2, 64, 64, 64) == 1       # out not 16-B aligned
    assert fn(CB.data_ptr(), SCB.data_ptr(), out.data_ptr() + 8, 64, 64, 64) == 1
    assert fn(CB.data_ptr() + 4, SCB.data_ptr(), out.data_ptr(), 56, 64, 64) == 1       # CB not 16-B aligned
    torch.cuda.synchronize()
    assert (out == POISON).all()
    assert fn(CB.data_ptr(), SCB.data_ptr(), out.data_ptr(), 0, 64, 64) == 0            # nothing to do
    torch.cuda.synchronize()
    assert (out == POISON).all()


def test_dequantize_int8_t_deterministic(dev):
    F = _F()
    CB, SCB = _weight(dev, 200, 336, seed=4)
    a = F.dequantize_int8_t(CB, SCB, torch.bfloat16)
    b = F.dequantize_int8_t(CB, SCB, torch.bfloat16)
    assert torch.equal(_bits(a), _bits(b))
