"""GPU: the LLM.int8 prefill forward with a threshold and no host round trip (csrc/int8_outlier_prefill.hip,
cint8_outlier_quant_fp16 / cint8_outlier_side_fp16, F.int8_linear_outliers, Linear8bitLt(fused_outlier_prefill=True))
against the restatement and derived tolerance of tests/int8_outlier_prefill_helpers.py.  Every tolerance check prints its
worst |out - exact| / tol before it asserts."""
import numpy as np
import pytest
import torch

from helpers import same_bits
from int8_outlier_prefill_helpers import prefill_reference, workspace_layout

pytestmark = pytest.mark.gpu

THR = 6.0
BELOW_THR = float(np.nextafter(np.float16(THR), np.float16(0)))          # the next fp16 below the threshold
COL_EQ, COL_BELOW = 33, 34                                   # a value equal to the threshold / the next fp16 below

# rows, N, K, planted outlier columns in all (None: the fixed patterns only)
SHAPES = [(33, 17, 64, None),          # the first row count past the decode kernel
          (1, 40, 1040, None),         # K no multiple of 32: the mask has a tail word
          (70, 100, 4096, 70),         # ragged row and column tiles; 70 columns: more than one list chunk
          (257, 384, 512, None),       # more than one row block (and the 16-B read-modify-write)
          (2, 8, 65552, None)]         # beyond the decode kernel's K limit

_cases = {}


def _F():
    import python_src_quants.functional as F
    return F


def _weights(rng, n, k):
    """(B, colStats, bias): the full int8 range, -128 included; colStats uniform in (0.5, 2); an fp16 bias."""
    B = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
    B.reshape(-1)[:: 7] = -128
    return B, rng.uniform(0.5, 2, n).astype(np.float32), rng.standard_normal(n).astype(np.float16)


def _activations(rng, rows, k, cols, zero_row):
    """sigma-1 activations clipped to +-5 (nothing near the threshold) with one outlier per column of `cols`: signs
    alternating, magnitudes 8..60, each in ONE row while the other rows hold ordinary values there; the last column of
    `cols` in the last row."""
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)
    live = [r for r in range(rows) if r != zero_row]
    for i, c in enumerate(cols):
        mag = 8.0 + (i * 13) % 53                            # 8 .. 60
        r = live[-1] if i == len(cols) - 1 else live[i % len(live)]
        A[r, c] = mag if i % 2 == 0 else -mag
    if zero_row is not None:
        A[zero_row] = 0
    return A


def _planted(rows, n, k, total):
    """Operands with planted outliers, drawn once per shape and shared (with their reference) by the cases: columns 0
    and K - 1 (the latter only in the last row), two in one 16-byte chunk (18 and 21), two more in one 32-bit mask word
    (40 and 59), a value equal to the threshold (outlier) and the next fp16 below it (not), a zero row when there are
    three rows or more."""
    key = (rows, n, k)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(100 * k + rows)
    zero_row = 1 if rows >= 3 else None
    cols = [0, 18, 21, 40, 59, k - 1]
    if total is not None:                                    # `total` outlier columns in all, COL_EQ among them
        free = np.setdiff1d(np.arange(k), cols + [COL_EQ, COL_BELOW])
        cols = sorted(cols + list(rng.choice(free, total - 1 - len(cols), replace=False)))
    A = _activations(rng, rows, k, cols, zero_row)
    live = [r for r in range(rows) if r != zero_row]
    A[live[-1], COL_EQ] = THR
    A[live[0], COL_BELOW] = BELOW_THR
    B, cs, bias = _weights(rng, n, k)
    refs = {wb: prefill_reference(A, B, cs, bias if wb else None, THR) for wb in (False, True)}
    assert len(refs[True]["S"]) == len(cols) + 1 and COL_BELOW not in refs[True]["S"] and COL_EQ in refs[True]["S"]
    _cases[key] = (A, B, cs, bias, refs, zero_row)
    return _cases[key]


def _check(tag, got, r, tol="tol", exact="exact"):
    """|got - exact| <= tol everywhere; prints the worst ratio first."""
    err = np.abs(got.astype(np.float64) - r[exact])
    ratio = float((err / r[tol]).max())
    print(f"[outlier prefill] {tag}: |S| = {len(r['S'])}, worst |out - {exact}| / {tol} = {ratio:.3f}")
    assert np.all(err <= r[tol]), (tag, ratio)


def _quant(F, At, thr=THR, ws=None):
    """cint8_outlier_quant_fp16 on a contiguous A; returns (rc, CA, rowStats, ws)."""
    m, k = At.shape
    nbytes, _, _ = workspace_layout(k)
    assert F.lib.cint8_outlier_workspace_bytes(k) == nbytes
    if ws is None:
        ws = torch.full((nbytes // 4,), 0x5a5a5a5a, dtype=torch.int32, device=At.device)   # a stale mask and list
    CA = torch.full((m, k), 99, dtype=torch.int8, device=At.device)
    stats = torch.full((m,), 7.0, dtype=torch.float32, device=At.device)
    rc = F.lib.cint8_outlier_quant_fp16(m, k, F.get_ptr(At), thr, F.get_ptr(CA), F.get_ptr(stats), F.get_ptr(ws),
                                        ws.numel() * 4)
    torch.cuda.synchronize()
    return rc, CA, stats, ws


@pytest.mark.parametrize("rows,n,k,total", SHAPES)
def test_quant_alone_is_bit_exact(dev, rows, n, k, total):
    F = _F()
    A, _, _, _, refs, zero_row = _planted(rows, n, k, total)
    r = refs[False]
    rc, CA, stats, ws = _quant(F, torch.from_numpy(A).to(dev))
    assert rc == 0 and F.lib.cget_last_error() == 0
    _, i_count, i_idx = workspace_layout(k)
    w = ws.cpu().numpy()
    assert int(w[i_count]) == len(r["S"])
    assert np.array_equal(w[i_idx:i_idx + len(r["S"])], r["S"].astype(np.int32))
    assert same_bits(stats.cpu().numpy(), r["row_stats"])
    assert same_bits(stats.cpu().numpy(), F.get_colrow_absmax(torch.from_numpy(A).to(dev), threshold=THR)[0].cpu().numpy())
    assert np.array_equal(CA.cpu().numpy(), r["CA"])
    if zero_row is not None:
        assert stats[zero_row].item() == 0.0 and not CA[zero_row].any()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("rows,n,k,total", SHAPES)
def test_planted_outliers(dev, rows, n, k, total, with_bias):
    F = _F()
    A, B, cs, bias, refs, _ = _planted(rows, n, k, total)
    r = refs[with_bias]
    At, Bt, cst = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(cs).to(dev)
    bt = torch.from_numpy(bias).to(dev) if with_bias else None
    stats = torch.full((rows,), 7.0, dtype=torch.float32, device=dev)
    out = F.int8_linear_outliers(At, Bt, cst, bias=bt, threshold=THR, row_stats=stats)
    again = F.int8_linear_outliers(At, Bt, cst, bias=bt, threshold=THR)
    assert F.lib.cget_last_error() == 0 and out.shape == (rows, n)
    got = out.cpu().numpy()
    _check(f"{rows} x {n} x {k} bias={with_bias}", got, r)
    assert same_bits(stats.cpu().numpy(), r["row_stats"])
    assert same_bits(again.cpu().numpy(), got)                                # the same call twice: equal bits
    # first's bits are the restatement's, so a zero side product would leave them; the planted columns must not
    assert not same_bits(got, r["first16"])
    # any rank: flattened over the leading dimensions
    if rows % 2 == 0:
        assert torch.equal(F.int8_linear_outliers(At.view(2, rows // 2, k), Bt, cst, bias=bt, threshold=THR), out)


def test_every_column_an_outlier(dev):
    F = _F()
    rows, n, k = 33, 17, 64
    rng = np.random.default_rng(9)
    A = _activations(rng, rows, k, list(range(k)), None)
    B, cs, bias = _weights(rng, n, k)
    r = prefill_reference(A, B, cs, bias, THR)
    assert len(r["S"]) == k
    At, Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (A, B, cs, bias))
    rc, CA, stats, ws = _quant(F, At)
    assert rc == 0 and not CA.any() and same_bits(stats.cpu().numpy(), r["row_stats"])
    assert ws[0].item() == k
    _check("every column", F.int8_linear_outliers(At, Bt, cst, bias=bt, threshold=THR).cpu().numpy(), r)


def _clean(rng, rows, k):
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)
    A[0, 3] = BELOW_THR
    if rows > 1:
        A[1] = 0                                              # signed zeros in the result
    return A


@pytest.mark.parametrize("rows,n,k", [(33, 17, 64), (1, 40, 1040), (70, 100, 4096), (257, 384, 512)])
def test_no_outlier_is_the_threshold_zero_layer(dev, rows, n, k):
    F = _F()
    rng = np.random.default_rng(k + rows)
    A = _clean(rng, rows, k)
    B, cs, bias = _weights(rng, n, k)
    At, Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (A, B, cs, bias))
    for b in (None, bt):
        CA0, s0 = F.int8_row_quant(At)
        plain = F.igemmlt_dequant(CA0, Bt, s0, cst, bias=b)
        s1 = torch.empty(rows, dtype=torch.float32, device=dev)
        out = F.int8_linear_outliers(At, Bt, cst, bias=b, threshold=THR, row_stats=s1)
        assert same_bits(out.cpu().numpy(), plain.cpu().numpy())
        assert same_bits(s1.cpu().numpy(), s0.cpu().numpy())
    rc, CA, _, ws = _quant(F, At)
    assert rc == 0 and ws[0].item() == 0 and torch.equal(CA, CA0)


def test_two_calls_share_the_workspace(dev):
    """The same workspace, first with outlier columns, then without: each call matches its own reference, so the mask of
    the first does not reach the second."""
    F = _F()
    rows, n, k = 70, 100, 4096
    A, B, cs, bias, refs, _ = _planted(rows, n, k, 70)
    A2 = _clean(np.random.default_rng(5), rows, k)
    At, A2t, Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (A, A2, B, cs, bias))
    first = F.int8_linear_outliers(At, Bt, cst, bias=bt, threshold=THR)
    second = F.int8_linear_outliers(A2t, Bt, cst, bias=bt, threshold=THR)
    third = F.int8_linear_outliers(At, Bt, cst, bias=bt, threshold=THR)
    _check("shared workspace, first", first.cpu().numpy(), refs[True])
    CA0, s0 = F.int8_row_quant(A2t)
    assert torch.equal(second, F.igemmlt_dequant(CA0, Bt, s0, cst, bias=bt))
    assert torch.equal(third, first)
    # the C entry on one explicit buffer: the second list is empty and CA is the threshold-0 quantisation
    rc, _, _, ws = _quant(F, At)
    assert rc == 0 and ws[0].item() == len(refs[True]["S"])
    rc, CA, _, ws = _quant(F, A2t, ws=ws)
    assert rc == 0 and ws[0].item() == 0 and torch.equal(CA, CA0)


def test_graph_replay_follows_the_device_data(dev):
    """Captured once into a linear graph, replayed after A is overwritten in place with other outlier columns (another
    count as well): right only if no size or branch came from the host."""
    F = _F()
    rows, n, k = 70, 100, 4096
    A, B, cs, bias, refs, _ = _planted(rows, n, k, 70)
    rng = np.random.default_rng(77)
    A2 = _activations(rng, rows, k, [5, 100, 101, 2047, 4000], 3)
    r2 = prefill_reference(A2, B, cs, bias, THR)
    assert list(r2["S"]) == [5, 100, 101, 2047, 4000]
    Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (B, cs, bias))
    A_static = torch.from_numpy(A).to(dev)
    out = torch.zeros((rows, n), dtype=torch.float16, device=dev)
    stats = torch.zeros(rows, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        F.int8_linear_outliers(A_static, Bt, cst, bias=bt, threshold=THR, out=out, row_stats=stats)   # workspaces exist
        with torch.cuda.graph(g, stream=s):
            F.int8_linear_outliers(A_static, Bt, cst, bias=bt, threshold=THR, out=out, row_stats=stats)
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check("graph, captured data", out.cpu().numpy(), refs[True])
    A_static.copy_(torch.from_numpy(A2).to(dev))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    _check("graph, new data", out.cpu().numpy(), r2)
    assert same_bits(stats.cpu().numpy(), r2["row_stats"])


def test_not_covered_launches_nothing_and_falls_back(dev):
    F = _F()
    rows, n, k = 5, 24, 12
    rng = np.random.default_rng(12)
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)
    A[0, 5], A[rows - 1, k - 1], A[0, 2] = 40.0, -9.0, THR
    B, cs, bias = _weights(rng, n, k)
    At, Bt, cst, bt = (torch.from_numpy(x).to(dev) for x in (A, B, cs, bias))
    assert not F.int8_linear_outliers_supported(rows, n, k)
    ws = torch.full((64,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    rc, CA, stats, ws = _quant(F, At, ws=ws)
    out = torch.full((rows, n), 123.0, dtype=torch.float16, device=dev)
    rc2 = F.lib.cint8_outlier_side_fp16(rows, n, k, F.get_ptr(At), F.get_ptr(Bt), F.get_ptr(cst), F.get_ptr(out), n,
                                        F.get_ptr(ws))
    torch.cuda.synchronize()
    assert rc == 2 and rc2 == 2 and F.lib.cget_last_error() == 0
    assert bool((out == 123.0).all()) and bool((CA == 99).all()) and bool((stats == 7.0).all())
    assert bool((ws == 0x5a5a5a5a).all())
    got = F.int8_linear_outliers(At, Bt, cst, bias=bt, threshold=THR, row_stats=stats)
    r = prefill_reference(A, B, cs, bias, THR)
    assert got.shape == (rows, n)
    _check("fallback 5 x 24 x 12", got.cpu().numpy(), r, tol="unfused_tol", exact="unfused_exact")
    assert same_bits(stats.cpu().numpy(), r["row_stats"])


def _layer(dev, **flags):
    from python_src_quants.nn import Linear8bitLt
    torch.manual_seed(11)
    lin = Linear8bitLt(512, 384, bias=True, has_fp16_weights=False, threshold=THR, **flags)
    # .cuda() quantises the weight rows to CB / SCB; an inference layer: no parameter wants a gradient
    return lin.cuda(dev).eval().requires_grad_(False)


def test_linear8bitlt_fused_outlier_prefill(dev):
    F = _F()
    on, off = _layer(dev, fused_outlier_prefill=True), _layer(dev)
    both = _layer(dev, fused_outlier_prefill=True, fused_outlier_decode=True)
    assert on.state.fused_outlier_prefill is True and off.state.fused_outlier_prefill is False
    torch.manual_seed(3)
    x = torch.randn(2, 40, 512, device=dev).clamp_(-5, 5).half()
    x[0, 1, 17], x[1, 39, 511], x[1, 2, 300] = 40.0, -9.0, THR
    with torch.no_grad():
        before = off(x)
        y_on = on(x)
        after = off(x)
        direct = F.int8_linear_outliers(x, on.state.CB, on.state.SCB, bias=on.bias, threshold=THR)
    assert torch.equal(on.state.CB, off.state.CB)                             # the same weight in the layers
    assert y_on.shape == (2, 40, 384) and torch.equal(y_on, direct.view(2, 40, 384))
    assert on.state.idx is None and on.state.subB is None                     # backward's only: not produced
    r = prefill_reference(x.reshape(-1, 512).cpu().numpy(), on.state.CB.cpu().numpy(), on.state.SCB.cpu().numpy(),
                          on.bias.detach().cpu().numpy(), THR)
    assert list(r["S"]) == [17, 300, 511]
    _check("layer", y_on.reshape(-1, 384).cpu().numpy(), r)
    _check("layer", y_on.reshape(-1, 384).cpu().numpy(), r, tol="unfused_tol", exact="unfused_exact")
    _check("default layer", before.reshape(-1, 384).cpu().numpy(), r, tol="unfused_tol", exact="unfused_exact")
    assert torch.equal(before, after)                                         # a default layer: unchanged bits
    xg = x.clone().requires_grad_(True)
    assert torch.equal(on(xg), off(xg))                                       # a gradient is wanted: the unfused layer
    # both flags: 1..32 rows stay on the one-launch decode kernel
    x3 = x[0, :3].contiguous()
    lib = F.lib
    prev = lib.cigemv_set_mode(1)
    try:
        with torch.no_grad():
            y3 = both(x3)
            rows3 = F.int8_linear_rows(x3, both.state.CB, both.state.SCB, bias=both.bias, threshold=THR)
    finally:
        lib.cigemv_set_mode(prev)
    assert torch.equal(y3, rows3)
