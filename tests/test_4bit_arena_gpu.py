"""Every kernel of the 4-bit product family (probe4bit_helpers.CASES) once with poison around its operands.

One dense call per case, Gaussian operands as in the tolerance tests.  Every operand lies inside a larger buffer at a
256-byte-aligned offset (no alignment contract changes, nothing is copied: the pointers are asserted), with at least a
256-row tile of poison before and after it: NaN around activations, absmax, code, code2, absmax2 and offset, 0xFF around
the packed weight and the nested codes.  The cached split-K workspace and the weight workspace are filled with NaN
before the call, and out= is a window in a buffer of sentinels.  The result must have the bits of the same call on
plain, freshly allocated operands and no NaN; every sentinel outside out[0:rows, 0:N] and every byte of every input
buffer must survive.  An over-read at a ragged tail that is multiplied by zero, or a split-K partial read before it is
written, shows here as a NaN; with the allocator's finite neighbours it shows nowhere.

All memory touched is allocated by the test."""
import ctypes as ct

import numpy as np
import pytest
import torch

import probe4bit_helpers as ph
from oracle import ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = 7.0
TILE_ROWS = 256
QUANT_TYPES = ["nf4", "fp4"]
KINDS16 = ["bf16", "fp16"]


def _F():
    import python_src_quants.functional as F
    return F


def _gaussian(dev, shape, kind, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(ph.torch_dtype(kind))


class Arena:
    """The operands of one call inside poisoned buffers; snapshot() before the call, assert_unchanged() after it."""

    def __init__(self):
        self.buffers = []

    def put(self, t, pad_elems, poison):
        buf, view = ph.in_arena(t.contiguous(), pad_elems, poison)
        self.buffers.append(buf)
        return view

    def state(self, F, st, K):
        """A QuantState like `st` whose every tensor lies in a poisoned buffer."""
        per_tile = TILE_ROWS * max(1, K // st.blocksize)
        code = self.put(st.code, TILE_ROWS, NAN)
        if not st.nested:
            return F.QuantState(absmax=self.put(st.absmax, per_tile, NAN), shape=st.shape, dtype=st.dtype,
                                blocksize=st.blocksize, code=code, quant_type=st.quant_type)
        s2 = st.state2
        state2 = F.QuantState(absmax=self.put(s2.absmax, TILE_ROWS, NAN), code=self.put(s2.code, TILE_ROWS, NAN),
                              blocksize=s2.blocksize, dtype=s2.dtype)
        offset = self.put(st.offset.reshape(1), TILE_ROWS, NAN).view(())
        return F.QuantState(absmax=self.put(st.absmax, per_tile, 0xFF), shape=st.shape, dtype=st.dtype,
                            blocksize=st.blocksize, code=code, quant_type=st.quant_type, offset=offset, state2=state2)

    def out(self, rows, N, dtype, dev):
        """A [rows, N] window with TILE_ROWS rows of sentinels before and after it."""
        self.outbuf = torch.full(((2 * TILE_ROWS + rows) * N,), SENTINEL, dtype=dtype, device=dev)
        self.lo, self.hi = TILE_ROWS * N, (TILE_ROWS + rows) * N
        view = self.outbuf[self.lo:self.hi].view(rows, N)
        assert view.data_ptr() == self.outbuf.data_ptr() + self.lo * self.outbuf.element_size()
        return view

    def snapshot(self):
        self.before = [ph.bits(b).clone() for b in self.buffers]

    def assert_unchanged(self):
        for b, was in zip(self.buffers, self.before):
            assert torch.equal(ph.bits(b), was), "an input buffer was written"
        assert bool((self.outbuf[:self.lo] == SENTINEL).all()) and bool((self.outbuf[self.hi:] == SENTINEL).all()), \
            "a sentinel outside out[0:rows, 0:N] was overwritten"


def _poison_workspaces(F, dev, dtype, rows, N, K):
    L = ph.lib()
    nbytes = max(int(L.cgemm_4bit_workspace_bytes(ct.c_int32(N), ct.c_int32(rows), ct.c_int32(K))),
                 int(L.chgemm_tn_workspace_bytes(ct.c_int32(rows), ct.c_int32(N), ct.c_int32(K))),
                 int(L.chgemm_tn_workspace_bytes(ct.c_int32(rows), ct.c_int32(K), ct.c_int32(N))))
    ws = F._gemm_workspace(dev, nbytes)
    if ws is not None:
        ws.fill_(NAN)
    if dtype != torch.float32:
        F._dequant_workspace(dev, dtype, N * K).fill_(NAN)
    return ws


def test_arena_layout(dev):
    """The helper itself: the operand is a 256-byte-aligned window of the buffer with its own values, everything before
    and after it (a 256-row tile at least) is poison, and a read one element too far on either side meets it."""
    operands = ((torch.arange(1, 301 * 8 + 1, device=dev, dtype=torch.float32).view(301, 8), TILE_ROWS * 8, NAN),
                (torch.arange(77, device=dev, dtype=torch.uint8).view(77, 1), TILE_ROWS * 4, 0xFF),
                (torch.ones(3, 16, device=dev, dtype=torch.bfloat16), TILE_ROWS * 16, NAN))
    for t, pad, poison in operands:
        buf, view = ph.in_arena(t, pad, poison)
        n = t.numel()
        off = (view.data_ptr() - buf.data_ptr()) // t.element_size()
        assert view.data_ptr() % 256 == 0 and off >= pad and buf.numel() - off - n >= pad
        assert torch.equal(view, t) and view.is_contiguous()
        around = torch.cat([buf[:off], buf[off + n:]])
        if t.is_floating_point():
            assert bool(torch.isnan(around).all()) and not bool(torch.isnan(buf[off:off + n].sum()))
            assert bool(torch.isnan(buf[off:off + n + 1].sum())) and bool(torch.isnan(buf[off - 1:off + n].sum()))
        else:
            assert bool((around == poison).all())


def _assert_same_bits_no_nan(got, want, what):
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the result"
    assert torch.equal(ph.bits(got), ph.bits(want)), f"{what}: differs from the call on plain operands"


def _product_in_arena(F, dev, case, kind, quant_type):
    N, rows, K = case.N, case.rows, case.K
    dtype = ph.torch_dtype(kind)
    W = _gaussian(dev, (N, K), kind, seed=N + K, scale=0.02)
    X = _gaussian(dev, (rows, K), kind, seed=rows * 3 + K)
    q, st = F.quantize_4bit(W, blocksize=case.blocksize, quant_type=quant_type, compress_statistics=case.nested)

    def call(X_, q_, st_, out):
        if case.api == "gemv":
            return F.gemv_4bit(X_, q_.t(), out=out, state=st_)
        return F.gemm_4bit(X_, q_, st_, out=out, _route=case.route)

    with ph.knobs(case.knobs):
        want = call(X, q, st, torch.empty(rows, N, dtype=dtype, device=dev)).clone()
        ar = Arena()
        Xa = ar.put(X, TILE_ROWS * K, NAN)
        qa = ar.put(q, TILE_ROWS * K // 2, 0xFF)
        sta = ar.state(F, st, K)
        out = ar.out(rows, N, dtype, dev)
        ws = _poison_workspaces(F, dev, dtype, rows, N, K)
        ar.snapshot()
        ptrs = (Xa.data_ptr(), qa.data_ptr(), out.data_ptr())
        got = call(Xa, qa, sta, out)
        assert got.data_ptr() == out.data_ptr() and ptrs == (Xa.data_ptr(), qa.data_ptr(), out.data_ptr())
        if ws is not None:
            assert F._gemm_workspace(dev, 4) is ws            # the call found the poisoned workspace, not a new one
    _assert_same_bits_no_nan(out, want, f"{case.kernel} [{case.id}, {kind}, {quant_type}]")
    ar.assert_unchanged()


@pytest.mark.parametrize("kernel,cases", [pytest.param(k, g, id=k) for k, g in ph.by_kernel(ph.CASES)])
def test_product_in_a_poisoned_arena(dev, kernel, cases):
    """Every table entry of the kernel, every activation type it takes, NF4 and FP4: one dense call each."""
    F = _F()
    fails = ph.Failures()
    for case in cases:
        for kind in case.kinds:
            for quant_type in QUANT_TYPES:
                with fails.check(f"{case.id}-{kind}-{quant_type}"):
                    _product_in_arena(F, dev, case, kind, quant_type)
    fails.assert_none()


@pytest.mark.parametrize("shape", [(192, 208), (300, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dequantize_in_a_poisoned_arena(dev, shape):
    """dequantize_4bit (plain and nested statistics) and dequantize_4bit_t, bf16 and fp16, NF4 and FP4: the bits of the
    call on plain operands, and of the CPU oracle's dequantise (one fp32 product, one rounding) on the decoded
    statistics."""
    F = _F()
    N, K = shape
    fails = ph.Failures()
    for kind in KINDS16:
        dtype = ph.torch_dtype(kind)
        W = _gaussian(dev, (N, K), kind, seed=N * 5 + K, scale=0.02)
        for quant_type in QUANT_TYPES:
            for nested in (False, True):
                q, st = F.quantize_4bit(W, blocksize=64, quant_type=quant_type, compress_statistics=nested)
                want, want_t = F.dequantize_4bit(q, st).clone(), F.dequantize_4bit_t(q, st).clone()
                label = f"{kind}-{quant_type}-{'nested' if nested else 'plain'}"
                with fails.check(label + "-oracle"):
                    oracle = ref.dequantize_blockwise(q.cpu().numpy().reshape(-1), F._absmax_fp32(st).cpu().numpy(), 64,
                                                      N * K, quant_type, kind)
                    assert torch.equal(ph.bits(want).cpu(), torch.from_numpy(oracle.view(np.int16)).view(N, K))
                for transposed in (False, True):
                    name = f"dequantize_4bit{'_t' if transposed else ''}"
                    with fails.check(f"{label}-{name}"):
                        ar = Arena()
                        qa = ar.put(q, TILE_ROWS * K // 2, 0xFF)
                        sta = ar.state(F, st, K)
                        out = ar.out(K, N, dtype, dev) if transposed else ar.out(N, K, dtype, dev)
                        ar.snapshot()
                        fn = F.dequantize_4bit_t if transposed else F.dequantize_4bit
                        got = fn(qa, sta, out=out)
                        assert got.data_ptr() == out.data_ptr()
                        _assert_same_bits_no_nan(out, want_t if transposed else want, name)
                        ar.assert_unchanged()
    fails.assert_none()


@pytest.mark.parametrize("route", ["hgemm", "library"])
@pytest.mark.parametrize("nested", [False, True], ids=["plain", "nested"])
def test_gemm_4bit_dgrad_in_a_poisoned_arena(dev, nested, route):
    """3 and 130 gradient rows, bf16 and fp16, NF4 and FP4, on the dequantize_4bit_t + k_hgemm route and on the
    dequantize_4bit + library GEMM route."""
    F = _F()
    N, K = 192, 208
    fails = ph.Failures()
    for kind in KINDS16:
        dtype = ph.torch_dtype(kind)
        W = _gaussian(dev, (N, K), kind, seed=9, scale=0.02)
        for quant_type, rows in ((qt, r) for qt in QUANT_TYPES for r in (3, 130)):
            q, st = F.quantize_4bit(W, blocksize=64, quant_type=quant_type, compress_statistics=nested)
            with fails.check(f"{kind}-{quant_type}-rows{rows}"):
                G = _gaussian(dev, (rows, N), kind, seed=rows)
                want = F.gemm_4bit_dgrad(G, q, st, _route=route).clone()
                ar = Arena()
                Ga = ar.put(G, TILE_ROWS * N, NAN)
                qa = ar.put(q, TILE_ROWS * K // 2, 0xFF)
                sta = ar.state(F, st, K)
                out = ar.out(rows, K, dtype, dev)
                _poison_workspaces(F, dev, dtype, rows, N, K)
                ar.snapshot()
                got = F.gemm_4bit_dgrad(Ga, qa, sta, out=out, _route=route)
                assert got.data_ptr() == out.data_ptr()
                _assert_same_bits_no_nan(out, want, "gemm_4bit_dgrad")
                ar.assert_unchanged()
    fails.assert_none()


def test_int8_linear_dgrad_in_a_poisoned_arena(dev):
    """3 and 130 gradient rows, bf16 and fp16, on the dequantize_int8_t + k_hgemm route."""
    F = _F()
    N, K = 192, 208
    g = torch.Generator(device="cpu").manual_seed(21)
    CB = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8).to(dev)
    SCB = (torch.rand(N, generator=g) * 3 + 0.1).to(dev)
    fails = ph.Failures()
    for kind in KINDS16:
        dtype = ph.torch_dtype(kind)
        for rows in (3, 130):
            with fails.check(f"{kind}-rows{rows}"):
                G = _gaussian(dev, (rows, N), kind, seed=rows + 1)
                want = F.int8_linear_dgrad(G, CB, SCB, _route="hgemm").clone()
                ar = Arena()
                Ga = ar.put(G, TILE_ROWS * N, NAN)
                CBa = ar.put(CB, TILE_ROWS * K, -1)               # 0xFF bytes
                SCBa = ar.put(SCB, TILE_ROWS, NAN)
                out = ar.out(rows, K, dtype, dev)
                _poison_workspaces(F, dev, dtype, rows, N, K)
                ar.snapshot()
                got = F.int8_linear_dgrad(Ga, CBa, SCBa, out=out, _route="hgemm")
                assert got.data_ptr() == out.data_ptr()
                _assert_same_bits_no_nan(out, want, "int8_linear_dgrad")
                ar.assert_unchanged()
    fails.assert_none()
