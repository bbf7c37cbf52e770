"""GPU: the plain int8 matmul family -- functional.igemm / batched_igemm and the cigemm / cbatched_igemm ABI -- on the
K-contiguous / K-strided int8 MFMA kernel (csrc/igemm_strided.hip).  Every result is compared for exact equality
with the integer product computed by torch in float64 (exact: |sum| <= 1000 * 2^14 < 2^53)."""
import ctypes as ct

import pytest
import torch

pytestmark = pytest.mark.gpu


def _F():
    import python_src_quants.functional as F
    return F


def _rand_i8(dev, *shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 7919 * len(shape) + sum(shape))
    t = torch.randint(-128, 128, shape, generator=g, dtype=torch.int8)
    flat = t.view(-1)
    flat[:: max(1, flat.numel() // 5)] = -128          # -128 is always present: no symmetric-range shortcut
    return t.to(dev)


def _exact(a, b):
    return torch.matmul(a.double(), b.double()).to(torch.int64)


def _same(out, expect):
    assert out.dtype == torch.int32 and tuple(out.shape) == tuple(expect.shape)
    return torch.equal(out.to(torch.int64), expect)


FORMS = ["NN", "NT", "TN", "TT"]       # is A / B handed over as the .t() view of a contiguous tensor?


def _operands(dev, m, n, k, form, seed=0):
    """A [m, k] and B [k, n] as views: 'T' = the transpose of a contiguous [cols, rows] tensor."""
    A = _rand_i8(dev, k, m, seed=seed).t() if form[0] == "T" else _rand_i8(dev, m, k, seed=seed)
    B = _rand_i8(dev, n, k, seed=seed + 1).t() if form[1] == "T" else _rand_i8(dev, k, n, seed=seed + 1)
    return A, B


SHAPES = [(1, 1, 1), (17, 5, 3), (64, 40, 96), (128, 128, 128), (129, 130, 131), (256, 129, 128), (77, 300, 1000)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_igemm_2d_views(dev, m, n, k, form):
    A, B = _operands(dev, m, n, k, form)
    assert _same(_F().igemm(A, B), _exact(A, B))


@pytest.mark.parametrize("form", ["NN", "TN", "TT", "NT"])
def test_igemm_larger_k_strided(dev, form):
    """Enough tiles (8 x 6 of 128 x 128, 4 k-tiles) to exercise the XCD-aware tile mapping and the aligned 16-B load +
    register transpose path of each K-strided instance: NN (B K-strided, MatMul8bit's forward), TT (A K-strided) and
    TN (both).  NT, both K-contiguous, rides along on the existing route."""
    A, B = _operands(dev, 1024, 768, 512, form, seed=3)
    assert _same(_F().igemm(A, B), _exact(A, B))


@pytest.mark.parametrize("form", FORMS)
def test_igemm_larger_unaligned_ld(dev, form):
    """Leading dimensions 776 and 520 (8 mod 16) over 8 x 7 tiles and 5 k-tiles: every operand row starts off a 16-B
    boundary, so full units take the two-aligned-loads-and-shift path and the last tile column / k-tile the bytewise one."""
    A, B = _operands(dev, 1024, 776, 520, form, seed=30)
    assert _same(_F().igemm(A, B), _exact(A, B))


def test_igemm_agrees_with_igemm_rowmajor(dev):
    F = _F()
    A, Bt = _rand_i8(dev, 300, 256, seed=4), _rand_i8(dev, 520, 256, seed=5)
    out = F.igemm(A, Bt.t())
    assert torch.equal(out, F.igemm_rowmajor(A, Bt))
    assert _same(out, _exact(A, Bt.t()))


def test_igemm_transposed_flags(dev):
    """transposed_A / transposed_B name the operand whose last two dims are swapped."""
    F = _F()
    A, B = _rand_i8(dev, 96, 33, seed=6), _rand_i8(dev, 50, 96, seed=7)        # A^T [33, 96] @ B^T [96, 50]
    assert _same(F.igemm(A, B, transposed_A=True, transposed_B=True), _exact(A.t(), B.t()))


def test_igemm_zero_rows(dev):
    out = _F().igemm(torch.empty((0, 16), dtype=torch.int8, device=dev), _rand_i8(dev, 16, 8))
    assert out.shape == (0, 8) and out.dtype == torch.int32


def test_igemm_out_given(dev):
    F = _F()
    A, B = _operands(dev, 70, 45, 130, "NN", seed=8)
    out = torch.full((70, 45), 7, dtype=torch.int32, device=dev)
    assert F.igemm(A, B, out=out) is out and _same(out, _exact(A, B))
    wide = torch.full((70, 64), 7, dtype=torch.int32, device=dev)            # a non-contiguous out
    F.igemm(A, B, out=wide[:, :45])
    assert _same(wide[:, :45], _exact(A, B)) and bool((wide[:, 45:] == 7).all())


@pytest.mark.parametrize("b_transposed", [False, True])
def test_igemm_3d_x_2d(dev, b_transposed):
    A = _rand_i8(dev, 2, 7, 70, seed=9)
    B = _rand_i8(dev, 33, 70, seed=10).t() if b_transposed else _rand_i8(dev, 70, 33, seed=10)
    assert _same(_F().igemm(A, B), _exact(A, B))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", [1, 3, 5])
def test_batched_igemm_permuted_views(dev, batch, form):
    F = _F()
    A = (_rand_i8(dev, batch, 70, 33, seed=11).permute(0, 2, 1) if form[0] == "T"
         else _rand_i8(dev, batch, 33, 70, seed=11))
    B = (_rand_i8(dev, batch, 65, 70, seed=12).permute(0, 2, 1) if form[1] == "T"
         else _rand_i8(dev, batch, 70, 65, seed=12))
    expect = _exact(A, B)
    assert _same(F.igemm(A, B), expect)
    assert _same(F.batched_igemm(A, B), expect)


def test_batched_igemm_non_contiguous_batch_slice(dev):
    """X[::2] has a batch stride no layout rule describes: made contiguous first, still exact."""
    A = _rand_i8(dev, 6, 33, 70, seed=13)[::2]
    B = _rand_i8(dev, 6, 70, 65, seed=14)[::2]
    assert not A.is_contiguous()
    assert _same(_F().igemm(A, B), _exact(A, B))


def test_igemm_bsi_bso_to_io(dev):
    A, B = _rand_i8(dev, 3, 40, 72, seed=15), _rand_i8(dev, 3, 40, 136, seed=16)
    out = torch.full((72, 136), -1, dtype=torch.int32, device=dev)
    res = _F().igemm(A, B, out=out)
    assert res is out
    assert _same(out, torch.einsum("bsi,bso->io", A.double(), B.double()).to(torch.int64))


def test_igemm_stream_capture(dev):
    """One NN igemm captured in a single-branch graph and replayed twice gives the eager result: no workspace, no
    allocation, launched on the capturing stream."""
    F = _F()
    A, B = _operands(dev, 200, 136, 300, "NN", seed=17)
    eager = F.igemm(A, B)
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        F.igemm(A, B, out=out)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        F.igemm(A, B, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager)


# ----------------------------------------------------------------------------- the C ABI, directly
SENTINEL = -559038737      # 0xDEADBEEF as int32
GUARD = 64


def _embed(dev, mat, transposed, pad, offset, seed):
    """Store `mat` [rows, cols] (or its transpose) in a larger noise-filled byte buffer with ld = extent + pad,
    starting `offset` bytes in.  Returns (buffer, device address of the first element, ld)."""
    stored = mat.t() if transposed else mat
    r, c = stored.shape
    ld = c + pad
    buf = _rand_i8(dev, offset + r * ld + 32, seed=seed)
    buf[offset: offset + r * ld].view(r, ld)[:, :c] = stored
    return buf, buf.data_ptr() + offset, ld


@pytest.mark.parametrize("pad,offset", [(16, 0), (16, 1), (3, 0), (3, 1)])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m,n,k", [(17, 5, 3), (128, 128, 128), (129, 130, 131)])
def test_cigemm_abi_padded_unaligned(dev, m, n, k, form, pad, offset):
    """Row-major out[m, n] = X[m, k] @ Y[k, n] is the column-major product of cigemm with A = Y, B = X and the sizes
    swapped.  The operands sit in larger buffers (ld > extent, base off by one byte); the output has ldc = n + 5 and
    guard regions, all prefilled with a sentinel that must survive outside out[0..m)[0..n)."""
    F = _F()
    from python_src_quants.cextension import lib
    X, Y = _rand_i8(dev, m, k, seed=20), _rand_i8(dev, k, n, seed=21)
    tX, tY = form[0] == "T", form[1] == "T"
    xbuf, xptr, ldx = _embed(dev, X, tX, pad, offset, 22)
    ybuf, yptr, ldy = _embed(dev, Y, tY, pad, offset, 23)
    ldc = n + 5
    obuf = torch.full((GUARD + m * ldc + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    prev = F.pre_call(dev)
    lib.cigemm(None, ct.c_bool(tY), ct.c_bool(tX), ct.c_int32(n), ct.c_int32(m), ct.c_int32(k), ct.c_void_p(yptr),
               ct.c_void_p(xptr), ct.c_void_p(obuf.data_ptr() + 4 * GUARD), ct.c_int32(ldy), ct.c_int32(ldx),
               ct.c_int32(ldc))
    F.post_call(prev)
    torch.cuda.synchronize(dev)
    body = obuf[GUARD: GUARD + m * ldc].view(m, ldc)
    assert torch.equal(body[:, :n].to(torch.int64), _exact(X, Y))
    assert bool((body[:, n:] == SENTINEL).all()), "ldc padding written"
    assert bool((obuf[:GUARD] == SENTINEL).all()) and bool((obuf[GUARD + m * ldc:] == SENTINEL).all()), "guard written"


@pytest.mark.parametrize("form", FORMS)
def test_cbatched_igemm_abi_strides(dev, form):
    """Batch strides larger than one matrix, unaligned bases, ldc = n + 5."""
    F = _F()
    from python_src_quants.cextension import lib
    nb, m, n, k = 3, 33, 65, 70
    X, Y = _rand_i8(dev, nb, m, k, seed=24), _rand_i8(dev, nb, k, n, seed=25)
    tX, tY = form[0] == "T", form[1] == "T"

    def embed(T, transposed, seed):
        stored = T.permute(0, 2, 1) if transposed else T
        _, r, c = stored.shape
        ld = c + 3
        stride = r * ld + 11
        buf = _rand_i8(dev, 1 + nb * stride + 32, seed=seed)
        for b in range(nb):
            buf[1 + b * stride: 1 + b * stride + r * ld].view(r, ld)[:, :c] = stored[b]
        return buf, buf.data_ptr() + 1, ld, stride

    xbuf, xptr, ldx, sx = embed(X, tX, 26)
    ybuf, yptr, ldy, sy = embed(Y, tY, 27)
    ldc = n + 5
    sc = m * ldc + 9
    obuf = torch.full((GUARD + nb * sc + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    prev = F.pre_call(dev)
    lib.cbatched_igemm(None, ct.c_bool(tY), ct.c_bool(tX), ct.c_int32(n), ct.c_int32(m), ct.c_int32(k),
                       ct.c_void_p(yptr), ct.c_void_p(xptr), ct.c_void_p(obuf.data_ptr() + 4 * GUARD), ct.c_int32(ldy),
                       ct.c_int32(ldx), ct.c_int32(ldc), ct.c_long(sy), ct.c_long(sx), ct.c_long(sc), ct.c_int32(nb))
    F.post_call(prev)
    torch.cuda.synchronize(dev)
    expect = _exact(X, Y)
    written = torch.zeros_like(obuf, dtype=torch.bool)
    for b in range(nb):
        body = obuf[GUARD + b * sc: GUARD + b * sc + m * ldc].view(m, ldc)
        assert torch.equal(body[:, :n].to(torch.int64), expect[b])
        written[GUARD + b * sc: GUARD + b * sc + m * ldc].view(m, ldc)[:, :n] = True
    assert bool((obuf[~written] == SENTINEL).all()), "wrote outside Out[b][0..m)[0..n)"


def test_cigemm_nonpositive_sizes_and_bad_ld(dev):
    F = _F()
    from python_src_quants.cextension import lib
    X, Y = _rand_i8(dev, 4, 8, seed=28), _rand_i8(dev, 8, 4, seed=29)
    out = torch.full((16,), SENTINEL, dtype=torch.int32, device=dev)
    prev = F.pre_call(dev)
    for m, n, k in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (-1, 4, 8)):
        lib.cigemm(None, ct.c_bool(False), ct.c_bool(False), ct.c_int32(n), ct.c_int32(m), ct.c_int32(k),
                   F.get_ptr(Y), F.get_ptr(X), F.get_ptr(out), ct.c_int32(4), ct.c_int32(8), ct.c_int32(4))
    F.post_call(prev)
    torch.cuda.synchronize(dev)
    assert bool((out == SENTINEL).all())
    # ld below the extent: refused through cget_last_error, nothing launched
    lib.cigemm(None, ct.c_bool(False), ct.c_bool(False), ct.c_int32(4), ct.c_int32(4), ct.c_int32(8), F.get_ptr(Y),
               F.get_ptr(X), F.get_ptr(out), ct.c_int32(4), ct.c_int32(7), ct.c_int32(4))
    assert lib.cget_last_error() != 0
    torch.cuda.synchronize(dev)
    assert bool((out == SENTINEL).all())
