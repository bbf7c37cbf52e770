"""The transposing 4-bit dequantise (csrc/dequant_t.hip, F.dequantize_4bit_t) on the GPU.

* Bit-exact against dequantize_4bit(...).t().contiguous() for nf4 / fp4, bf16 / fp16, plain and compressed statistics,
  on the smallest shapes that reach each way the kernel can go wrong: one tile, a single block, both dimensions ragged
  with blocks that straddle rows (and a partial second-level block), several tiles, a block that spans many rows.
* out= as a window of a wider buffer (ldo > N): nothing outside the window is written.
* Shapes the C entry declines (return 1, nothing written) still dequantise through the function.
* Two calls give the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (64, 64, 64),      # one tile, one block per row
    (8, 8, 64),        # a single block
    (72, 200, 64),     # both dimensions ragged, blocks straddle rows, 225 blocks: the second-level block is partial
    (264, 576, 64),    # several tiles, ragged in N
    (128, 192, 128),   # blocks straddle rows
    (136, 64, 4096),   # one block spans 64 rows
]


def _F():
    import python_src_quants.functional as F
    return F


def _quantized(dev, N, K, blocksize, quant_type, dtype, nested, seed=0):
    F = _F()
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + N + K)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype).to(dev)
    return F.quantize_4bit(W, blocksize=blocksize, quant_type=quant_type, compress_statistics=nested)


def _reference(q, st, dtype):
    F = _F()
    W = torch.empty(tuple(st.shape), dtype=dtype, device=q.device)
    F.dequantize_4bit(q, st, out=W)
    return W.t().contiguous()


@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("N,K,blocksize", SHAPES)
def test_dequantize_4bit_t_bit_exact(dev, quant_type, dtype, nested, N, K, blocksize):
    F = _F()
    q, st = _quantized(dev, N, K, blocksize, quant_type, dtype, nested)
    assert st.nested == nested
    got = F.dequantize_4bit_t(q, st)
    exp = F.dequantize_4bit(q, st).t().contiguous()
    assert got.shape == (K, N) and got.dtype == dtype and got.is_contiguous()
    assert torch.equal(got.view(torch.int16), exp.view(torch.int16))
    # the kernel itself took the shape (the function did not fall back to the copy)
    probe = torch.empty((K, N), dtype=dtype, device=dev)
    assert F._dequant_4bit_t_launch(q, st, probe) == 0
    assert torch.equal(probe.view(torch.int16), exp.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("N,K", [(72, 200), (264, 576)])
def test_dequantize_4bit_t_out_window(dev, dtype, nested, N, K):
    """out = columns [8, 8 + N) of rows [1, K + 1) of a [K + 2, N + 24] buffer: ldo = N + 24 > N, 16-B aligned."""
    F = _F()
    q, st = _quantized(dev, N, K, 64, "nf4", dtype, nested, seed=1)
    buf = torch.full((K + 2, N + 24), -7.0, dtype=dtype, device=dev)
    win = buf[1:K + 1, 8:8 + N]
    assert win.data_ptr() % 16 == 0 and win.stride(0) % 8 == 0
    assert F._dequant_4bit_t_launch(q, st, win) == 0          # the kernel takes the window
    buf.fill_(-7.0)
    res = F.dequantize_4bit_t(q, st, out=win)
    assert res.data_ptr() == win.data_ptr()
    exp = _reference(q, st, dtype)
    assert torch.equal(buf[1:K + 1, 8:8 + N].view(torch.int16), exp.view(torch.int16))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[1:K + 1, 8:8 + N] = False
    assert (buf[outside] == -7.0).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("N,K,pad", [(64, 100, 0), (12, 64, 0), (64, 64, 4)], ids=["K100", "N12", "ldo_mod8"])
def test_dequantize_4bit_t_declines(dev, dtype, nested, N, K, pad):
    """K % 8, N % 8 or ldo % 8 != 0: the C entry returns 1 and writes nothing; the function still returns the bits."""
    F = _F()
    q, st = _quantized(dev, N, K, 64, "nf4", dtype, nested, seed=2)
    buf = torch.full((K, N + pad), -7.0, dtype=dtype, device=dev)
    win = buf[:, :N]
    assert F._dequant_4bit_t_launch(q, st, win) == 1
    torch.cuda.synchronize()
    assert (buf == -7.0).all()
    exp = _reference(q, st, dtype)
    assert torch.equal(F.dequantize_4bit_t(q, st).view(torch.int16), exp.view(torch.int16))
    F.dequantize_4bit_t(q, st, out=win)
    assert torch.equal(buf[:, :N].contiguous().view(torch.int16), exp.view(torch.int16))
    assert (buf[:, N:] == -7.0).all()


def test_dequantize_4bit_t_plain_entry_declines_directly(dev):
    """The plain C entry called by hand: 1 for K = 100, N = 12, ldo % 8 != 0, ldo < N and an unsupported blocksize."""
    F = _F()
    q, st = _quantized(dev, 64, 64, 64, "nf4", torch.bfloat16, False, seed=3)
    out = torch.full((128 * 128,), -7.0, dtype=torch.bfloat16, device=dev)
    fn = F.lib.cdequantize_blockwise_t_bf16_nf4
    for blocksize, rows, cols, ldo in [(64, 64, 100, 64), (64, 12, 64, 16), (64, 64, 64, 68), (64, 64, 64, 56),
                                       (32, 64, 64, 64), (96, 64, 64, 64)]:
        assert fn(q.data_ptr(), st.absmax.data_ptr(), out.data_ptr(), blocksize, rows, cols, ldo) == 1
    assert fn(q.data_ptr(), st.absmax.data_ptr(), out.data_ptr() + 2, 64, 64, 64, 64) == 1     # out not 16-B aligned
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_dequantize_4bit_t_fp32_and_dtype_of_out(dev):
    """fp32 goes through the untransposed dequantise; out's dtype (not the state's) decides the rounding."""
    F = _F()
    q, st = _quantized(dev, 72, 200, 64, "nf4", torch.bfloat16, True, seed=4)
    for dtype in (torch.float32, torch.float16):
        out = torch.empty((200, 72), dtype=dtype, device=dev)
        F.dequantize_4bit_t(q, st, out=out)
        assert torch.equal(out, _reference(q, st, dtype))


@pytest.mark.parametrize("nested", [False, True])
def test_dequantize_4bit_t_deterministic(dev, nested):
    F = _F()
    q, st = _quantized(dev, 264, 576, 64, "nf4", torch.bfloat16, nested, seed=5)
    a = F.dequantize_4bit_t(q, st)
    b = F.dequantize_4bit_t(q, st)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
