"""Exact one-hot probes of every kernel of the 4-bit product family (probe4bit_helpers.CASES: the kernel, the knobs that
force it -- checked on the CPU by test_4bit_probe_routes_cpu.py -- and the shape).

Weights are built directly: seeded uniform 4-bit codes, plain absmax 2^e_b with e_b = ((5 b + 3) % 7) - 3, so that
neighbouring statistics blocks and the blocks one weight row apart differ by a factor of >= 2.  Row m of call c holds
one nonzero +-2^j at k = (37 m + c) % K; calls c = 0 .. K - 1 probe every (row, k) pair once.  Every output is then
x_m * round_T(code[q[n, k_m]]) * 2^e_block(n, k_m) on every route, as values (a zero of either sign is zero, no NaN
anywhere): no tolerance.  The expectation is a gather from one [N, K] tensor built on the CPU; mismatches are counted on
the device, one synchronisation per case; a failing case runs again to name the first (c, m, n, k).

Contract pins: the same sweep with absmax 0.0537 (1 + b % 5) separates the arithmetic contracts (dequantise first and
round to T / T(code) products scaled by the fp32 absmax); each case names its class from its kernel file's header.
Nested statistics: each route that decodes them in the kernel equals, bit for bit, itself on the decoded fp32 absmax.
Then the dequantises, the two input gradients and chgemm_tn_* by hand on the same sweeps."""
import functools

import numpy as np
import pytest
import torch

import probe4bit_helpers as ph
from test_hgemm_gpu import _hgemm, _hgemm_ws

pytestmark = pytest.mark.gpu
F32 = np.float32
QUANT_TYPES = ["nf4", "fp4"]


def _F():
    import python_src_quants.functional as F
    return F


def _variants(cases):
    """(case, kind, quant type): every activation type of every case, NF4 and FP4."""
    return [(c, kind, qt) for c in cases for kind in c.kinds for qt in QUANT_TYPES]


PLAIN = [c for c in ph.CASES if not c.nested]
NESTED = [c for c in ph.CASES if c.nested]


def _by_kernel(cases):
    return [pytest.param(kernel, group, id=kernel) for kernel, group in ph.by_kernel(cases)]


@functools.lru_cache(maxsize=8)
def _codes(N, K):
    return ph.probe_codes(N, K, seed=N * 7919 + K)


@functools.lru_cache(maxsize=4)
def _expectation_t(dev, N, K, blocksize, quant_type, kind, contract, stats):
    """([K, N] fp32 expectation on the device, absmax) for the probe weight of this shape."""
    q, _ = _codes(N, K)
    absmax = (ph.pow2_absmax if stats == "pow2" else ph.pin_absmax)(ph.nblocks(N, K, blocksize))
    W = ph.expected_weight(q, absmax, blocksize, quant_type, kind, contract)
    return torch.from_numpy(np.ascontiguousarray(W.T)).to(dev), absmax


def _weight(F, dev, case, quant_type, kind, absmax):
    _, packed = _codes(case.N, case.K)
    q, st = ph.make_weight(F, dev, case.N, case.K, case.blocksize, quant_type, kind, packed, absmax)
    assert st.code.cpu().numpy().tobytes() == ph.table_of(quant_type).tobytes()
    return q, st


def _probe(dev, case, kind, quant_type, stats):
    F = _F()
    Et, absmax = _expectation_t(dev, case.N, case.K, case.blocksize, quant_type, kind, case.contract, stats)
    q, st = _weight(F, dev, case, quant_type, kind, absmax)
    with ph.knobs(case.knobs):
        ph.assert_sweep_exact(ph.runner(F, case, q, st), Et, ph.Sweep(dev, case.rows, case.K, kind),
                              f"{case.kernel} [{case.id}, {kind}, {quant_type}, {stats} absmax]")


@pytest.mark.parametrize("case", PLAIN, ids=ph.case_id)
def test_one_hot_probe_is_exact(dev, case):
    """One table entry: every activation type it takes, NF4 and FP4."""
    fails = ph.Failures()
    for kind in case.kinds:
        for quant_type in QUANT_TYPES:
            with fails.check(f"{kind}-{quant_type}"):
                _probe(dev, case, kind, quant_type, "pow2")
    fails.assert_none()


@pytest.mark.parametrize("kernel,cases", _by_kernel(PLAIN))
def test_contract_pin(dev, kernel, cases):
    """The same sweep with non-power-of-two statistics: every plain entry of the kernel computes what its kernel file's
    header says (case.contract)."""
    fails = ph.Failures()
    for case, kind, quant_type in _variants(cases):
        with fails.check(f"{case.id}-{kind}-{quant_type}"):
            _probe(dev, case, kind, quant_type, "pin")
    fails.assert_none()


def _nested_equals_decoded(dev, case, kind, quant_type):
    F = _F()
    _, packed = _codes(case.N, case.K)
    q, st = ph.make_nested_weight(F, dev, case.N, case.K, case.blocksize, quant_type, kind, packed,
                                  seed=case.N + case.K)
    assert st.nested and F._nested_stats_in_kernel_ok(st)
    absmax = F._absmax_fp32(st)
    assert bool(torch.isfinite(absmax).all()) and float(absmax.min()) > 0
    with ph.knobs(case.knobs):
        n = ph.sweep_bit_differences(ph.runner(F, case, q, st), ph.runner(F, case, q, st, absmax=absmax),
                                     ph.Sweep(dev, case.rows, case.K, kind))
    assert n == 0, f"{case.kernel} [{case.id}]: {n} outputs differ between nested and decoded statistics"


@pytest.mark.parametrize("kernel,cases", _by_kernel(NESTED))
def test_nested_statistics_equal_their_decoded_form(dev, kernel, cases):
    """Arbitrary nested statistics (those of a quantised Gaussian tensor): every nested entry of the kernel, decoding
    them in the kernel, equals, bit for bit over the whole sweep, the same route on absmax = F._absmax_fp32(state)."""
    fails = ph.Failures()
    for case, kind, quant_type in _variants(cases):
        with fails.check(f"{case.id}-{kind}-{quant_type}"):
            _nested_equals_decoded(dev, case, kind, quant_type)
    fails.assert_none()


# ------------------------------------------------------------------------------------ dequantise and input gradients
DG_SHAPES = [(64, 64), (64, 208), (192, 64), (192, 208)]      # (N, K); K = 208: blocks straddle weight rows
_SHAPE_ID = dict(ids=lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else None)
KINDS16 = ["bf16", "fp16"]


def _dg_weight(F, dev, N, K, quant_type, kind, stats):
    q, packed = ph.probe_codes(N, K, seed=N * 31 + K)
    absmax = (ph.pow2_absmax if stats == "pow2" else ph.pin_absmax)(ph.nblocks(N, K, 64))
    W = ph.expected_weight(q, absmax, 64, quant_type, kind, ph.DEQUANT_FIRST)
    qd, st = ph.make_weight(F, dev, N, K, 64, quant_type, kind, packed, absmax)
    if quant_type == "fp4":
        # bit for bit: the reference's FP4 decode is a magnitude tree and a sign bit (oracle.ref.dequant_fp4_value), so
        # code 8 dequantises to -0.0 where the code table holds +0.0 -- the same value, the zero's other sign
        W = np.where(q == 8, F32(-0.0), W)
    return qd, st, torch.from_numpy(W).to(dev)


@pytest.mark.parametrize("shape", DG_SHAPES, **_SHAPE_ID)
def test_dequantize_and_its_transpose_are_the_expectation_tensor(dev, shape):
    """bf16 and fp16, NF4 and FP4, power-of-two and pin statistics: bit for bit."""
    F = _F()
    N, K = shape
    fails = ph.Failures()
    for kind in KINDS16:
        for quant_type in QUANT_TYPES:
            for stats in ("pow2", "pin"):
                with fails.check(f"{kind}-{quant_type}-{stats}"):
                    q, st, W = _dg_weight(F, dev, N, K, quant_type, kind, stats)
                    want = W.to(ph.torch_dtype(kind))
                    assert torch.equal(want.float(), W)       # the expectation is a tensor of T values
                    got, got_t = F.dequantize_4bit(q, st), F.dequantize_4bit_t(q, st)
                    assert got.shape == (N, K) and got_t.shape == (K, N)
                    assert torch.equal(ph.bits(got), ph.bits(want)), "dequantize_4bit"
                    assert torch.equal(ph.bits(got_t), ph.bits(want.t().contiguous())), "dequantize_4bit_t"
    fails.assert_none()


@pytest.mark.parametrize("route", ["hgemm", "library"])
@pytest.mark.parametrize("shape", DG_SHAPES, **_SHAPE_ID)
def test_gemm_4bit_dgrad_returns_scaled_weight_rows(dev, shape, route):
    """One-hot gradient rows (3 and 130 of them), swept over N: out[m, :] == g_m * W[n_m, :]."""
    F = _F()
    N, K = shape
    fails = ph.Failures()
    for kind in KINDS16:
        for quant_type in QUANT_TYPES:
            q, st, W = _dg_weight(F, dev, N, K, quant_type, kind, "pow2")
            for rows in (3, 130):
                what = f"gemm_4bit_dgrad[{route}] {N}x{K} rows {rows} {kind} {quant_type}"
                with fails.check(what):
                    ph.assert_sweep_exact(lambda G: F.gemm_4bit_dgrad(G, q, st, _route=route), W,
                                          ph.Sweep(dev, rows, N, kind), what)
    fails.assert_none()


@pytest.mark.parametrize("shape", DG_SHAPES, **_SHAPE_ID)
def test_int8_linear_dgrad_returns_scaled_weight_rows(dev, shape):
    """SCB = 127 * 2^e_n and a seeded random CB: out[m, :] == g_m * round_T(CB * (SCB / 127))[n_m, :], on both routes,
    at 3 and 130 gradient rows."""
    F = _F()
    N, K = shape
    CB = np.random.default_rng(N * 13 + K).integers(-127, 128, size=(N, K), dtype=np.int8)
    scale = ph.pow2_absmax(N)
    SCB = (F32(127.0) * scale).astype(F32)
    s = (SCB * F32(1.0 / 127.0)).astype(F32)                  # the scale as the dequantise forms it
    assert np.array_equal(s, scale)                           # ... which is SCB / 127 exactly here
    CBd, SCBd = torch.from_numpy(CB).to(dev), torch.from_numpy(SCB).to(dev)
    fails = ph.Failures()
    for kind in KINDS16:
        W = torch.from_numpy(ph.round_T((CB.astype(F32) * s[:, None]).astype(F32), kind)).to(dev)
        for route in ("hgemm", "library"):
            for rows in (3, 130):
                what = f"int8_linear_dgrad[{route}] {N}x{K} rows {rows} {kind}"
                with fails.check(what):
                    ph.assert_sweep_exact(lambda G: F.int8_linear_dgrad(G, CBd, SCBd, _route=route), W,
                                          ph.Sweep(dev, rows, N, kind), what)
    fails.assert_none()


# ------------------------------------------------------------------------------------ chgemm_tn_* by hand
def _random_T(dev, n, k, ld, kind, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, ld, generator=g).to(dev).to(ph.torch_dtype(kind))[:, :k]


@pytest.mark.parametrize("mnk,lda,ldw,ws", [((300, 300, 1024), None, None, True), ((300, 300, 1024), None, None, False),
                                            ((3, 5, 128), None, None, False), ((70, 300, 256), 320, 384, False)],
                         ids=["300x300x1024-ws", "300x300x1024", "3x5x128", "70x300x256-strided"])
def test_hgemm_by_hand_one_hot(dev, mnk, lda, ldw, ws):
    """k_hgemm alone (with its split-K workspace, without one, and on row slices of wider buffers), bf16 and fp16:
    seeded random W, one-hot rows: C[m, n] == x_m * W[n, k_m], torch.equal."""
    F = _F()
    m, n, k = mnk
    fails = ph.Failures()
    for kind in KINDS16:
        W = _random_T(dev, n, k, ldw or k, kind, seed=m + n + k)
        sweep = ph.Sweep(dev, m, k, kind, round_product=True)     # randn values: a product may be subnormal in fp16
        if lda:
            sweep.X = torch.zeros(m, lda, device=dev, dtype=ph.torch_dtype(kind))[:, :k]

        def run(X):
            rc, Y = _hgemm_ws(F, X, W) if ws else _hgemm(F, X, W, lda=lda, ldw=ldw)
            assert rc == 0
            return Y

        with fails.check(kind):
            if ws:
                assert ph.hgemm_plan(m, n, k)["splits"] > 1 and W.is_contiguous()
            ph.assert_sweep_exact(run, W.t().float().contiguous(), sweep, f"chgemm_tn {mnk} {kind}")
            kk, v = sweep.put(5)                                  # and once more, spelled with torch.equal
            assert torch.equal(run(sweep.X), (W.t()[kk].float() * v[:, None]).to(W.dtype))
    fails.assert_none()
