"""GPU: the int8 decode kernel (igemv8.hip) for 1..32 activation rows -- bit-exact against the oracle's igemmlt +
mm_dequant and against the tile-kernel route, coverage and bounds, the fused activation quantisation, and the routes
of igemmlt_dequant and Linear8bitLt under cigemv_set_mode."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import same_bits
from oracle import ref

pytestmark = pytest.mark.gpu


def _F():
    import python_src_quants.functional as F
    return F


@contextlib.contextmanager
def _mode(mode):
    lib = _F().lib
    prev = lib.cigemv_set_mode(mode)
    try:
        yield
    finally:
        lib.cigemv_set_mode(prev)


def _direct(F, A, B, rs, cs, bias, out=None, m=None):
    """cigemv_row_dequant_fp16 on contiguous operands; returns (rc, out)."""
    m = A.shape[0] if m is None else m
    n, k = B.shape
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=A.device)
    rc = F.lib.cigemv_row_dequant_fp16(m, n, k, F.get_ptr(A), F.get_ptr(B), F.get_ptr(out), F.get_ptr(rs),
                                       F.get_ptr(cs), F.get_ptr(bias), k, k, n)
    torch.cuda.synchronize()
    return rc, out


# every row count with at least two (N, K) pairs, every pair with rows 1 and 32
NK = [(1, 16), (17, 64), (100, 1040), (1030, 4096), (256, 11008), (32, 28672)]
ROWS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32]
CASES = sorted({(r, nk) for nk in NK for r in (1, 32)} |
               {(r, NK[(i + j) % len(NK)]) for i, r in enumerate(ROWS) for j in (0, 3)})

_operands = {}


def _weights(n, k):
    """(B, colStats, bias) as numpy, drawn once per (N, K) and shared by the cases; the full int8 range, -128 included."""
    if (n, k) not in _operands:
        rng = np.random.default_rng(1000 * n + k)
        B = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
        B.reshape(-1)[:: 7] = -128
        _operands[(n, k)] = (B, rng.uniform(0.5, 2, n).astype(np.float32), rng.standard_normal(n).astype(np.float16))
    return _operands[(n, k)]


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("rows,nk", CASES)
def test_direct_entry_bit_exact(dev, rows, nk, with_bias):
    F = _F()
    n, k = nk
    B, cs, bias = _weights(n, k)
    rng = np.random.default_rng(rows)
    A = rng.integers(-128, 128, size=(rows, k), dtype=np.int8)
    A[0, :: 5] = -128
    rs = rng.uniform(0.5, 2, rows).astype(np.float32)
    At, Bt = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    rst, cst = torch.from_numpy(rs).to(dev), torch.from_numpy(cs).to(dev)
    bt = torch.from_numpy(bias).to(dev) if with_bias else None
    with _mode(1):
        rc, out = _direct(F, At, Bt, rst, cst, bt)
        assert rc == 0 and F.lib.cget_last_error() == 0
        again = _direct(F, At, Bt, rst, cst, bt)[1]
        via_py = F.igemv_dequant(At, Bt, rst, cst, bias=bt)
    exp = ref.mm_dequant(ref.igemmlt(A, B), rs, cs, bias if with_bias else None)
    assert same_bits(out.cpu().numpy(), exp)
    assert same_bits(again.cpu().numpy(), out.cpu().numpy())          # deterministic
    assert torch.equal(via_py, out)
    with _mode(-1):
        old = F.igemmlt_dequant(At, Bt, rst, cst, bias=bt)
    assert torch.equal(old, out)


@pytest.mark.parametrize("rows,n,k", [(1, 64, 200), (1, 64, 8), (33, 64, 64), (0, 64, 64)])
def test_not_covered_launches_nothing(dev, rows, n, k):
    F = _F()
    rng = np.random.default_rng(k + rows)
    A = torch.from_numpy(rng.integers(-128, 128, size=(rows, k), dtype=np.int8)).to(dev)
    B = torch.from_numpy(rng.integers(-128, 128, size=(n, k), dtype=np.int8)).to(dev)
    rs = torch.from_numpy(rng.uniform(0.5, 2, rows).astype(np.float32)).to(dev)
    cs = torch.from_numpy(rng.uniform(0.5, 2, n).astype(np.float32)).to(dev)
    out = torch.full((max(rows, 1), n), 123.0, dtype=torch.float16, device=dev)
    with _mode(1):
        rc, _ = _direct(F, A, B, rs, cs, None, out=out, m=rows)
        assert rc == (0 if rows == 0 else 2) and F.lib.cget_last_error() == 0
        assert bool((out == 123.0).all())
        got = F.igemv_dequant(A, B, rs, cs)
        fused_in = (torch.randn(rows, k, device=dev) * 3).half()
        got_rows = F.int8_linear_rows(fused_in, B, cs)
    with _mode(-1):
        exp = F.igemmlt_dequant(A, B, rs, cs)
        CA, SCA = F.int8_row_quant(fused_in)
        exp_rows = F.igemmlt_dequant(CA, B, SCA, cs)
    assert got.shape == (rows, n) and torch.equal(got, exp)
    assert got_rows.shape == (rows, n) and torch.equal(got_rows, exp_rows)
    if rows:
        e = ref.mm_dequant(ref.igemmlt(A.cpu().numpy(), B.cpu().numpy()), rs.cpu().numpy(), cs.cpu().numpy(), None)
        assert same_bits(got.cpu().numpy(), e)


def test_bounds_sentinels_intact(dev):
    """B and out are the interior of larger sentinel-filled buffers: the result is right (nothing outside B was
    summed) and nothing around out is written."""
    F = _F()
    rows, n, k, pad = 3, 17, 64, 4096
    rng = np.random.default_rng(5)
    A = rng.integers(-128, 128, size=(rows, k), dtype=np.int8)
    B = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
    rs = rng.uniform(0.5, 2, rows).astype(np.float32)
    cs = rng.uniform(0.5, 2, n).astype(np.float32)
    bigB = torch.full((pad + n * k + pad,), 77, dtype=torch.int8, device=dev)
    bigB[pad:pad + n * k] = torch.from_numpy(B).to(dev).reshape(-1)
    bigO = torch.full((pad + rows * n + pad,), -777.0, dtype=torch.float16, device=dev)
    Bv, Ov = bigB[pad:pad + n * k].view(n, k), bigO[pad:pad + rows * n].view(rows, n)
    assert Bv.data_ptr() % 16 == 0
    with _mode(1):
        rc, _ = _direct(F, torch.from_numpy(A).to(dev), Bv, torch.from_numpy(rs).to(dev), torch.from_numpy(cs).to(dev),
                        None, out=Ov)
    assert rc == 0 and F.lib.cget_last_error() == 0
    assert same_bits(Ov.cpu().numpy(), ref.mm_dequant(ref.igemmlt(A, B), rs, cs, None))
    assert bool((bigO[:pad] == -777.0).all()) and bool((bigO[pad + rows * n:] == -777.0).all())
    assert bool((bigB[:pad] == 77).all()) and bool((bigB[pad + n * k:] == 77).all())


_fused_weight = {}


@pytest.mark.parametrize("k", [64, 4096, 16384, 28672])
@pytest.mark.parametrize("rows", [1, 4, 7, 32])
def test_fused_quantisation_bit_exact(dev, rows, k):
    """int8_linear_rows(A) == igemmlt_dequant(*int8_row_quant(A), ...) with a zero row and an all-NaN row; the row
    statistics are int8_row_quant's (K > 16384: its double_quant fallback), -50000 for the NaN row."""
    F = _F()
    n = 40
    if k not in _fused_weight:
        rng = np.random.default_rng(k)
        _fused_weight[k] = (torch.from_numpy(rng.integers(-128, 128, size=(n, k), dtype=np.int8)).to(dev),
                            torch.from_numpy(rng.uniform(0.5, 2, n).astype(np.float32)).to(dev),
                            torch.from_numpy(rng.standard_normal(n).astype(np.float16)).to(dev))
    CB, SCB, bias = _fused_weight[k]
    torch.manual_seed(rows * 100000 + k)
    A = (torch.randn(rows, k, device=dev) * 3).half()
    A[0] = 0
    if rows > 2:
        A[2] = float("nan")
    stats = torch.full((rows,), 7.0, dtype=torch.float32, device=dev)
    with _mode(1):
        rc = F.lib.cint8_linear_rows_fp16(rows, n, k, F.get_ptr(A), F.get_ptr(CB),
                                          F.get_ptr(torch.empty(rows, n, dtype=torch.float16, device=dev)), None,
                                          F.get_ptr(SCB), F.get_ptr(bias), k, k, n)
        assert rc == 0 and F.lib.cget_last_error() == 0
        got = F.int8_linear_rows(A, CB, SCB, bias=bias, row_stats=stats)
        again = F.int8_linear_rows(A, CB, SCB, bias=bias)
    with _mode(-1):
        CA, SCA = F.int8_row_quant(A)
        exp = F.igemmlt_dequant(CA, CB, SCA, SCB, bias=bias)
        via_fallback = F.int8_linear_rows(A, CB, SCB, bias=bias)
    if k > 16384:       # beyond the one-pass row kernel: int8_row_quant already returned double_quant's row half
        orow, _, rs, _, _ = F.double_quant(A)
        assert torch.equal(orow, CA) and same_bits(rs.cpu().numpy(), SCA.cpu().numpy())
    assert same_bits(got.cpu().numpy(), exp.cpu().numpy())
    assert same_bits(again.cpu().numpy(), got.cpu().numpy())
    assert same_bits(via_fallback.cpu().numpy(), exp.cpu().numpy())
    assert same_bits(stats.cpu().numpy(), SCA.cpu().numpy())
    assert stats[0].item() == 0.0
    if rows > 2:
        assert stats[2].item() == -50000.0
    # and against the oracle, from the quantised activations
    e = ref.mm_dequant(ref.igemmlt(CA.cpu().numpy(), CB.cpu().numpy()), SCA.cpu().numpy(), SCB.cpu().numpy(),
                       bias.cpu().numpy())
    assert same_bits(got.cpu().numpy(), e)


@pytest.mark.parametrize("rows,n,k", [(1, 300, 512), (5, 256, 1024), (32, 1030, 4096)])
def test_route_equality_igemmlt_dequant(dev, rows, n, k):
    """igemmlt_dequant itself under mode -1 and mode 1, also through the workspace-less C entry."""
    F = _F()
    rng = np.random.default_rng(rows + n)
    A = torch.from_numpy(rng.integers(-128, 128, size=(rows, k), dtype=np.int8)).to(dev)
    B = torch.from_numpy(rng.integers(-128, 128, size=(n, k), dtype=np.int8)).to(dev)
    rs = torch.from_numpy(rng.uniform(0.5, 2, rows).astype(np.float32)).to(dev)
    cs = torch.from_numpy(rng.uniform(0.5, 2, n).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rng.standard_normal(n).astype(np.float16)).to(dev)
    outs = {}
    for mode in (-1, 1, 0):
        with _mode(mode):
            outs[mode] = F.igemmlt_dequant(A, B, rs, cs, bias=bias)
            o2 = torch.empty_like(outs[mode])
            assert F.lib.cigemmlt_row_dequant_fp16(rows, n, k, F.get_ptr(A), F.get_ptr(B), F.get_ptr(o2), F.get_ptr(rs),
                                                   F.get_ptr(cs), F.get_ptr(bias), k, k, n) == 0
            assert torch.equal(o2, outs[mode])
    assert torch.equal(outs[-1], outs[1]) and torch.equal(outs[-1], outs[0])
    # a forced tile kernel or split-K factor keeps the route it names, whatever the mode: still the same bits
    with _mode(1):
        F.lib.cigemm_set_tile(128)
        try:
            assert torch.equal(F.igemmlt_dequant(A, B, rs, cs, bias=bias), outs[-1])
        finally:
            F.lib.cigemm_set_tile(0)
        F.lib.cigemm_set_splitk(2)
        try:
            assert torch.equal(F.igemmlt_dequant(A, B, rs, cs, bias=bias), outs[-1])
        finally:
            F.lib.cigemm_set_splitk(-1)


def _layer(dev, threshold):
    from python_src_quants.nn import Linear8bitLt
    torch.manual_seed(11)
    lin = Linear8bitLt(512, 384, bias=True, has_fp16_weights=False, threshold=threshold)
    return lin.cuda(dev).eval()              # .cuda() quantises the weight rows to CB / SCB


@pytest.mark.parametrize("shape", [(1, 1, 512), (2, 3, 512)])
def test_linear8bitlt_identical_under_both_modes(dev, shape):
    lin = _layer(dev, 0.0)
    torch.manual_seed(shape[1])
    x = torch.randn(*shape, device=dev).half()
    outs = {}
    with torch.no_grad():
        for mode in (-1, 1, 0):
            with _mode(mode):
                outs[mode] = lin(x)
    assert outs[1].shape == shape[:2] + (384,)
    assert torch.equal(outs[-1], outs[1]) and torch.equal(outs[-1], outs[0])
    # the one-launch step is what mode 1 ran: its result from the layer's own state
    st = lin.state
    with _mode(1):
        direct = _F().int8_linear_rows(x.reshape(-1, 512), st.CB, st.SCB, bias=lin.bias)
    assert torch.equal(direct.view(outs[1].shape), outs[1])


def test_linear8bitlt_outlier_path_ignores_the_mode(dev):
    """threshold 6 with an outlier planted: the fp16 outlier product must stay, so the fused entry is not taken."""
    lin = _layer(dev, 6.0)
    torch.manual_seed(3)
    x = torch.randn(2, 3, 512, device=dev).half()
    x[0, 1, 17] = 40.0
    outs = {}
    with torch.no_grad():
        for mode in (-1, 1):
            with _mode(mode):
                outs[mode] = lin(x)
        with _mode(1):
            no_outlier = _F().int8_linear_rows(x.reshape(-1, 512), lin.state.CB, lin.state.SCB, bias=lin.bias)
    assert torch.equal(outs[-1], outs[1])
    assert not torch.equal(no_outlier.view(outs[1].shape), outs[1])
