"""GPU: the LLM.int8 decode forward with a threshold in one launch (csrc/igemv8_outlier.hip,
cint8_linear_rows_outlier_fp16, F.int8_linear_rows(threshold=...), Linear8bitLt(fused_outlier_decode=True)) against the
float64 restatement and derived tolerance of tests/int8_outlier_helpers.py.  Every tolerance check prints its worst
|out - exact| / tol before it asserts."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import same_bits
from int8_outlier_helpers import entry_only_reference, outlier_reference

pytestmark = pytest.mark.gpu

THR = 6.0
BELOW_THR = float(np.nextafter(np.float16(THR), np.float16(0)))          # the next fp16 below the threshold


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


def _direct(F, A, B, cs, bias, thr, out=None, m=None, stats=None, count=None):
    """cint8_linear_rows_outlier_fp16 on contiguous operands; returns (rc, out)."""
    m = A.shape[0] if m is None else m
    n, k = B.shape
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=A.device)
    rc = F.lib.cint8_linear_rows_outlier_fp16(m, n, k, F.get_ptr(A), F.get_ptr(B), F.get_ptr(out), F.get_ptr(stats),
                                              F.get_ptr(count), F.get_ptr(cs), F.get_ptr(bias), thr, k, k, n)
    torch.cuda.synchronize()
    return rc, out


# rows, N, K, outlier columns planted beyond the fixed patterns (17 x 16 x 2048: 70 in all, more than a 64-entry list)
SHAPES = [(1, 17, 64, 0), (3, 40, 1040, 0), (16, 33, 4096, 0), (17, 16, 2048, None), (32, 100, 4096, 0),
          (32, 32, 28672, 0)]
COL_EQ, COL_BELOW = 33, 34                                   # a value equal to the threshold / the next fp16 below

_cases = {}


def _wave_share_columns(k):
    """One column inside every wave's K share (the kernel's split: eighths of whole 256-column steps)."""
    nsteps = (k + 255) // 256
    cols = []
    for w in range(8):
        s0, s1 = w * nsteps // 8, (w + 1) * nsteps // 8
        if s1 > s0:
            cols.append(min(s0 * 256 + 37, k - 1))
    return cols


def _weights(rng, n, k):
    """(B, colStats, bias): the full int8 range, -128 included; colStats uniform in (0.5, 2); an fp16 bias."""
    B = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
    B.reshape(-1)[:: 7] = -128
    return B, rng.uniform(0.5, 2, n).astype(np.float32), rng.standard_normal(n).astype(np.float16)


def _planted(rows, n, k, extra):
    """Operands with planted outliers, drawn once per shape and shared (with their reference) by the cases:
    column 0 and K - 1, two outliers in one 16-byte chunk (columns 18 and 21), one in every wave's K share, signs
    alternating, magnitudes 8..60, each in ONE row while the other rows hold ordinary values there, a value equal to
    the threshold (outlier) and the next fp16 below it (not), and a zero row when there are three rows or more."""
    key = (rows, n, k)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(100 * k + rows)
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)      # sigma 1, nothing near the threshold
    zero_row = 1 if rows >= 3 else None
    live_rows = [r for r in range(rows) if r != zero_row]
    cols = sorted({0, k - 1, 18, 21, *_wave_share_columns(k)})
    if extra is None:                                        # 70 outlier columns in all, COL_EQ among them
        free = np.setdiff1d(np.arange(k), cols + [COL_EQ, COL_BELOW])
        cols = sorted(cols + list(rng.choice(free, 69 - len(cols), replace=False)))
    for i, c in enumerate(cols):
        mag = 8.0 + (i * 13) % 53                            # 8 .. 60
        A[live_rows[i % len(live_rows)], c] = mag if i % 2 == 0 else -mag
    A[live_rows[-1], COL_EQ] = THR
    A[live_rows[0], COL_BELOW] = BELOW_THR
    if zero_row is not None:
        A[zero_row] = 0
    B, cs, bias = _weights(rng, n, k)
    refs = {wb: outlier_reference(A, B, cs, bias if wb else None, THR) for wb in (False, True)}
    assert len(refs[True]["S"]) == len(cols) + 1 and COL_BELOW not in refs[True]["S"]
    assert float(np.abs(refs[True]["exact"]).max()) < 65504
    _cases[key] = (A, B, cs, bias, refs, zero_row)
    return _cases[key]


def _check(tag, got, r):
    """|got - exact| <= tol everywhere; prints the worst ratio first."""
    err = np.abs(got.astype(np.float64) - r["exact"])
    ratio = float((err / r["tol"]).max())
    print(f"[outlier] {tag}: |S| = {len(r['S'])}, worst |out - exact| / tol = {ratio:.3f}")
    assert np.all(err <= r["tol"]), (tag, ratio)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("rows,n,k,extra", SHAPES)
def test_planted_outliers(dev, rows, n, k, extra, with_bias):
    F = _F()
    A, B, cs, bias, refs, zero_row = _planted(rows, n, k, extra)
    r = refs[with_bias]
    At, Bt, cst = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(cs).to(dev)
    bt = torch.from_numpy(bias).to(dev) if with_bias else None
    stats = torch.full((rows,), 7.0, dtype=torch.float32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    with _mode(1):
        rc, out = _direct(F, At, Bt, cst, bt, THR, stats=stats, count=count)
        assert rc == 0 and F.lib.cget_last_error() == 0
        again = _direct(F, At, Bt, cst, bt, THR)[1]
        via_py = F.int8_linear_rows(At, Bt, cst, bias=bt, threshold=THR)
    got = out.cpu().numpy()
    _check(f"{rows} x {n} x {k} bias={with_bias}", got, r)
    expected_stats = F.get_colrow_absmax(At, threshold=THR)[0]
    assert same_bits(stats.cpu().numpy(), expected_stats.cpu().numpy())
    assert same_bits(stats.cpu().numpy(), r["row_stats"])
    assert count.item() == len(r["S"])
    assert same_bits(again.cpu().numpy(), got)                                # deterministic
    assert torch.equal(via_py, out)
    if zero_row is not None:
        assert stats[zero_row].item() == 0.0
    if rows > 1:
        # the whole column leaves the int8 product, not only the entry above the threshold
        assert not same_bits(got, entry_only_reference(A, B, cs, bias if with_bias else None, THR))


def test_nan_row(dev):
    """An all-NaN row: its statistic is -50000 and it marks no column; the other rows stay within the tolerance."""
    F = _F()
    rows, n, k = 3, 40, 1040
    A, B, cs, bias, _, _ = _planted(rows, n, k, 0)
    A = A.copy()
    A[2] = np.float16("nan")
    r = outlier_reference(A, B, cs, bias, THR)
    stats = torch.empty(rows, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    with _mode(1):
        rc, out = _direct(F, torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(cs).to(dev),
                          torch.from_numpy(bias).to(dev), THR, stats=stats, count=count)
    assert rc == 0 and F.lib.cget_last_error() == 0
    assert stats[2].item() == -50000.0 and same_bits(stats.cpu().numpy(), r["row_stats"])
    assert count.item() == len(r["S"])
    got = out.cpu().numpy()
    live = [0, 1]
    assert np.all(np.abs(got[live].astype(np.float64) - r["exact"][live]) <= r["tol"][live])


@pytest.mark.parametrize("rows,n,k", [(1, 17, 64), (5, 40, 1040), (32, 33, 4096)])
def test_no_outlier_is_the_threshold_zero_kernel(dev, rows, n, k):
    F = _F()
    rng = np.random.default_rng(k + rows)
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)
    A[0, 3] = BELOW_THR
    if rows > 1:
        A[1] = 0                                              # signed zeros in the result
    B, cs, bias = _weights(rng, n, k)
    At, Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (A, B, cs, bias))
    s0 = torch.empty(rows, dtype=torch.float32, device=dev)
    s1 = torch.empty(rows, dtype=torch.float32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    with _mode(1):
        for b in (None, bt):
            plain = F.int8_linear_rows(At, Bt, cst, bias=b, row_stats=s0)
            rc, out = _direct(F, At, Bt, cst, b, THR, stats=s1, count=count)
            assert rc == 0 and F.lib.cget_last_error() == 0
            assert same_bits(out.cpu().numpy(), plain.cpu().numpy())
            assert same_bits(s1.cpu().numpy(), s0.cpu().numpy())
            assert count.item() == 0
            assert torch.equal(F.int8_linear_rows(At, Bt, cst, bias=b, threshold=THR), plain)


def test_every_column_an_outlier(dev):
    F = _F()
    rows, n, k, thr = 4, 24, 1040, 1e-6
    rng = np.random.default_rng(9)
    A = rng.standard_normal((rows, k)).astype(np.float16)
    A[A == 0] = np.float16(0.5)
    B, cs, bias = _weights(rng, n, k)
    r = outlier_reference(A, B, cs, bias, thr)
    assert len(r["S"]) == k
    stats = torch.full((rows,), 7.0, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    with _mode(1):
        rc, out = _direct(F, torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(cs).to(dev),
                          torch.from_numpy(bias).to(dev), thr, stats=stats, count=count)
    assert rc == 0 and F.lib.cget_last_error() == 0
    _check("every column", out.cpu().numpy(), r)
    assert bool((stats == 0).all()) and count.item() == k


def test_bounds_sentinels_intact(dev):
    """B and out are the interior of larger sentinel-filled buffers, with outliers in column 0 and K - 1: the result is
    right (nothing outside B was summed) and nothing around out is written."""
    F = _F()
    rows, n, k, pad = 3, 17, 64, 4096
    A, B, cs, _, refs, _ = _planted(rows, n, k, 0)
    bigB = torch.full((pad + n * k + pad,), 77, dtype=torch.int8, device=dev)
    bigB[pad:pad + n * k] = torch.from_numpy(B).to(dev).reshape(-1)
    bigO = torch.full((pad + rows * n + pad,), -777.0, dtype=torch.float16, device=dev)
    Bv, Ov = bigB[pad:pad + n * k].view(n, k), bigO[pad:pad + rows * n].view(rows, n)
    assert Bv.data_ptr() % 16 == 0
    with _mode(1):
        rc, _ = _direct(F, torch.from_numpy(A).to(dev), Bv, torch.from_numpy(cs).to(dev), None, THR, out=Ov)
    assert rc == 0 and F.lib.cget_last_error() == 0
    _check("sentinels", Ov.cpu().numpy(), refs[False])
    assert bool((bigO[:pad] == -777.0).all()) and bool((bigO[pad + rows * n:] == -777.0).all())
    assert bool((bigB[:pad] == 77).all()) and bool((bigB[pad + n * k:] == 77).all())


@pytest.mark.parametrize("rows,n,k,thr", [(1, 64, 200, THR), (1, 64, 8, THR), (33, 64, 64, THR), (2, 8, 65552, THR),
                                          (2, 64, 64, 0.0), (2, 64, 64, float("nan"))])
def test_not_covered_launches_nothing_and_falls_back(dev, rows, n, k, thr):
    F = _F()
    rng = np.random.default_rng(k + rows)
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)
    A[0, 5], A[rows - 1, k - 1], A[0, 2] = 40.0, -9.0, THR
    B, cs, bias = _weights(rng, n, k)
    At, Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (A, B, cs, bias))
    out = torch.full((rows, n), 123.0, dtype=torch.float16, device=dev)
    stats = torch.full((rows,), 7.0, dtype=torch.float32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    with _mode(1):
        rc, _ = _direct(F, At, Bt, cst, bt, thr, out=out, stats=stats, count=count)
        assert rc == 2 and F.lib.cget_last_error() == 0
        assert bool((out == 123.0).all()) and bool((stats == 7.0).all()) and count.item() == -1
        if thr == THR:
            got = F.int8_linear_rows(At, Bt, cst, bias=bt, threshold=THR, row_stats=stats)
    if thr == THR:
        r = outlier_reference(A, B, cs, bias, THR)
        err = np.abs(got.cpu().numpy().astype(np.float64) - r["exact"])
        print(f"[outlier] fallback {rows} x {n} x {k}: worst |out - exact| / unfused_tol = "
              f"{float((err / r['unfused_tol']).max()):.3f}")
        assert got.shape == (rows, n) and np.all(err <= r["unfused_tol"])
        assert same_bits(stats.cpu().numpy(), r["row_stats"])


def _layer(dev, fused):
    from python_src_quants.nn import Linear8bitLt
    torch.manual_seed(11)
    lin = Linear8bitLt(512, 384, bias=True, has_fp16_weights=False, threshold=THR, fused_outlier_decode=fused)
    # .cuda() quantises the weight rows to CB / SCB; an inference layer: no parameter wants a gradient (a trainable
    # bias is an input that needs one, and keeps MatMul8bitLt on its training-capable path)
    return lin.cuda(dev).eval().requires_grad_(False)


def test_linear8bitlt_fused_outlier_decode(dev):
    F = _F()
    on, off = _layer(dev, True), _layer(dev, False)
    assert on.state.fused_outlier_decode is True and off.state.fused_outlier_decode is False
    torch.manual_seed(3)
    x = torch.randn(2, 3, 512, device=dev).clamp_(-5, 5).half()
    x[0, 1, 17] = 40.0
    outs = {}
    with torch.no_grad():
        for mode in (-1, 1):
            with _mode(mode):
                outs["on", mode], outs["off", mode] = on(x), off(x)
        with _mode(1):
            direct = F.int8_linear_rows(x.reshape(-1, 512), on.state.CB, on.state.SCB, bias=on.bias, threshold=THR)
    assert torch.equal(on.state.CB, off.state.CB)                             # the same weight in both layers
    assert torch.equal(outs["on", 1], direct.view(2, 3, 384))
    r = outlier_reference(x.reshape(-1, 512).cpu().numpy(), on.state.CB.cpu().numpy(), on.state.SCB.cpu().numpy(),
                          on.bias.detach().cpu().numpy(), THR)
    assert list(r["S"]) == [17]
    _check("layer", outs["on", 1].reshape(-1, 384).cpu().numpy(), r)
    assert torch.equal(outs["on", -1], outs["off", -1])                       # switched off: the unfused layer
    assert torch.equal(outs["off", -1], outs["off", 1])                       # a default layer ignores the mode
    xg = x.clone().requires_grad_(True)
    with _mode(1):
        assert torch.equal(on(xg), off(xg))                                   # a gradient is wanted: the unfused layer
