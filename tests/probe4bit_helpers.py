"""Shared by the exact probes of the 4-bit product family (test_4bit_probe_routes_cpu.py, test_4bit_exact_probe_gpu.py,
test_4bit_arena_gpu.py): one table of (kernel, knobs that force it, shape), weights built directly from 4-bit codes
and chosen statistics, the three expected-value functions (one per arithmetic contract of the kernel files' header
comments) and the one-hot sweep that checks a route on the device without a tolerance.

Why one-hot rows: with a single nonzero activation +-2^j in a row, every output is x * w[n, k] for exactly one weight
element, so an output names the weight element (and the statistics block) it came from, and with power-of-two
statistics all three contracts give the same value: Y[m, n] == x_m * round_T(code[q[n, k_m]]) * 2^e_block(n, k_m).
Row m of call c probes k = (37 m + c) % K, so calls c = 0 .. K - 1 probe every (row, k) pair once.

Not a conftest: the tests import it."""
import contextlib
import ctypes as ct
from collections import namedtuple

import numpy as np

from oracle import ref
# FtKernel (csrc/gemm_common.hpp) and the fields of cgemm_4bit_plan, as test_fewtoken_plan_cpu.py names them
from test_fewtoken_plan_cpu import FIELDS as PLAN_FIELDS
from test_fewtoken_plan_cpu import (BAD_ARGS, FEWTOK, GEMV_TOK, NONE, SKINNY, T64, T64R,  # noqa: F401
                                    TILE128, TILE256, WK)

F32 = np.float32

# arithmetic contracts (header comments of the kernel files)
DEQUANT_FIRST = "dequant_first"   # gemm4bit{,_256,_wk,_skinny}.hip, hgemm route: T(fp32(code * absmax)) on the MFMA
GEMV = "gemv"                     # gemv4bit{,_tok}.hip dot / bal / wide: (sum x * T(code)) * absmax in fp32
TCODE_MFMA = "tcode_mfma"         # gemm4bit_{fewtok,t64}.hip: T(code) * x on the MFMA, block sum * fp32 absmax


def lib():
    import python_src_quants as bnb
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    return bnb.lib


# ------------------------------------------------------------------------------------------------ knobs
# setter -> default; cgemm_4bit_set_* / cgemv_4bit_set_*
KNOB_DEFAULTS = {"cgemm_4bit_set_tile": 0, "cgemm_4bit_set_fewtoken_kernel": 0, "cgemm_4bit_set_skinny_config": -1,
                 "cgemm_4bit_set_fewtok_mode": 0, "cgemm_4bit_set_t64_mode": 0, "cgemm_4bit_set_t64_regfed": 1,
                 "cgemm_4bit_set_t64_splits": 0, "cgemv_4bit_set_kernel": 0, "cgemv_4bit_set_wide_rows": 0}


@contextlib.contextmanager
def knobs(settings):
    """Set {setter name: value} for one block; every setter goes back to its default in the finally."""
    L = lib()
    try:
        for name, v in settings.items():
            assert name in KNOB_DEFAULTS, name
            getattr(L, name)(ct.c_int(v))
        yield
    finally:
        for name in settings:
            getattr(L, name)(ct.c_int(KNOB_DEFAULTS[name]))


def gemm_plan(N, rows, K, blocksize=64, nested=False, blocksize2=256):
    out = (ct.c_int * 16)()
    lib().cgemm_4bit_plan(ct.c_int(N), ct.c_int(rows), ct.c_int(K), ct.c_int(blocksize),
                          ct.c_int(blocksize2 if nested else 0), ct.c_int(1 if nested else 0), out)
    return dict(zip(PLAN_FIELDS, out))


def hgemm_plan(m, n, k):
    out = (ct.c_int * 4)()
    lib().chgemm_tn_plan(ct.c_int(m), ct.c_int(n), ct.c_int(k), out)
    return {"wi": out[0], "wj": out[1], "splits": out[2], "kchunk": out[3]}


# ------------------------------------------------------------------------------------------------ the table
# api: "gemm" = F.gemm_4bit(_route=route), "gemv" = F.gemv_4bit (one row).  plan: what cgemm_4bit_plan (route "fused")
# or chgemm_tn_plan (route "hgemm") must report under `knobs`; "split": True asserts splits > 1, False splits == 1.
# kinds: activation dtypes.  The one-row GEMVs have no plan query: their knob is a hard selection in gemv4bit.hip
# (launch_gemv_dot / gemv_wide_preferred / gemv_4bit), restated per case in `why`.
Case = namedtuple("Case", "id kernel api knobs N rows K blocksize nested contract route plan kinds why")
_16 = ("bf16", "fp16")
_FT = {"cgemm_4bit_set_fewtok_mode": 2}
_NOFT = {"cgemm_4bit_set_fewtok_mode": 1}
_WK = {"cgemm_4bit_set_fewtoken_kernel": 2}
_SK = {"cgemm_4bit_set_fewtoken_kernel": 1}


def _both(id, kernel, api, kn, N, rows, K, bs, contract, route, plan, kinds=_16, why="", nested=(False, True)):
    return [Case(f"{id}-{'nested' if ns else 'plain'}", kernel, api, kn, N, rows, K, bs, ns, contract, route, plan,
                 kinds, why) for ns in nested]


def _cases():
    c = []
    # k_gemv_4bit_tok: 2 and 4 rows; it declines fewer weight rows than CUs (256), so N = 300
    for rows in (2, 4):
        c += _both(f"gemv_tok-r{rows}", "k_gemv_4bit_tok", "gemm", _NOFT, 300, rows, 1024, 64, GEMV, "fused",
                   {"kernel": GEMV_TOK, "mt": 2 if rows == 2 else 4})
    # ... and 1100 weight rows: 512 workgroups of 3 / 2 rows (N / G and one more in the first N % G)
    for rows in (2, 4):
        c += _both(f"gemv_tok-r{rows}-n1100", "k_gemv_4bit_tok", "gemm", _NOFT, 1100, rows, 1024, 64, GEMV, "fused",
                   {"kernel": GEMV_TOK, "mt": 2 if rows == 2 else 4, "grid": 512, "waves": 3, "rg": 1})
    for bs in (128, 256):
        c += _both(f"gemv_tok-r2-bs{bs}", "k_gemv_4bit_tok", "gemm", _NOFT, 300, 2, 1024, bs, GEMV, "fused",
                   {"kernel": GEMV_TOK, "mt": 2})
    # k_gemm_4bit_fewtok: each MT instance (5 -> MT 1 with the 8-token form, 17 / 32 -> MT 2); K / 256 four-block groups
    # over 8 waves: K = 1024 leaves waves without a group, 2048 one each, 4096 two each
    for rows, K, plan in ((5, 1024, {"mt": 1, "x8": 1}), (17, 1024, {"mt": 2}), (32, 1024, {"mt": 2}),
                          (5, 2048, {"mt": 1, "x8": 1}), (17, 4096, {"mt": 2})):
        c += _both(f"fewtok-r{rows}-k{K}", "k_gemm_4bit_fewtok", "gemm", _FT, 200, rows, K, 64, TCODE_MFMA, "fused",
                   dict(plan, kernel=FEWTOK, s4=1, waves=8))
    c += _both("fewtok-r5-n1", "k_gemm_4bit_fewtok", "gemm", _FT, 1, 5, 1024, 64, TCODE_MFMA, "fused",
               {"kernel": FEWTOK, "mt": 1, "grid": 1})
    for bs in (128, 256):
        c += _both(f"fewtok-r5-bs{bs}", "k_gemm_4bit_fewtok", "gemm", _FT, 200, 5, 1024, bs, TCODE_MFMA, "fused",
                   {"kernel": FEWTOK, "mt": 1, "s4": 0})
    # k_gemm_4bit_wk (whole K, waves split it) and k_gemm_4bit_skinny (workgroups split it)
    for K in (1024, 2048):
        c += _both(f"wk-r8-k{K}", "k_gemm_4bit_wk", "gemm", _WK, 200, 8, K, 64, DEQUANT_FIRST, "fused",
                   {"kernel": WK, "mt": 1})
    for bs in (128, 256):
        c += _both(f"wk-r8-bs{bs}", "k_gemm_4bit_wk", "gemm", _WK, 200, 8, 1024, bs, DEQUANT_FIRST, "fused",
                   {"kernel": WK})
    c += _both("skinny-r8", "k_gemm_4bit_skinny", "gemm", _SK, 200, 8, 2048, 64, DEQUANT_FIRST, "fused",
               {"kernel": SKINNY, "mt": 1, "split": True})
    c += _both("skinny-r48", "k_gemm_4bit_skinny", "gemm", _SK, 200, 48, 1024, 64, DEQUANT_FIRST, "fused",
               {"kernel": SKINNY, "mt": 4, "split": True})
    c += _both("skinny-r48-cfg2", "k_gemm_4bit_skinny", "gemm", dict(_SK, cgemm_4bit_set_skinny_config=2), 200, 48,
               1024, 64, DEQUANT_FIRST, "fused", {"kernel": SKINNY, "mt": 4, "cfg": 2, "waves": 8, "split": True})
    for bs in (128, 256):
        c += _both(f"skinny-r8-bs{bs}", "k_gemm_4bit_skinny", "gemm", _SK, 200, 8, 2048, bs, DEQUANT_FIRST, "fused",
                   {"kernel": SKINNY, "split": True})
    # k_gemm_4bit_t64 (split over the workspace, and unsplit) and the register-fed k_gemm_4bit_t64r; blocksize 64 only
    for rows in (33, 64):
        c += _both(f"t64-r{rows}-split", "k_gemm_4bit_t64", "gemm", _NOFT, 200, rows, 1024, 64, TCODE_MFMA, "fused",
                   {"kernel": T64, "split": True, "waves": 8 if rows == 33 else 4})
        c += _both(f"t64-r{rows}-whole", "k_gemm_4bit_t64", "gemm", dict(_NOFT, cgemm_4bit_set_t64_splits=1), 200, rows,
                   1024, 64, TCODE_MFMA, "fused", {"kernel": T64, "split": False})
        c += _both(f"t64r-r{rows}", "k_gemm_4bit_t64r", "gemm", dict(_NOFT, cgemm_4bit_set_t64_regfed=2), 200, rows,
                   1024, 64, TCODE_MFMA, "fused", {"kernel": T64R})
    # the tile kernels take plain statistics only
    c += _both("tile128-r70", "k_gemm_4bit", "gemm", {"cgemm_4bit_set_tile": 128}, 300, 70, 1024, 64, DEQUANT_FIRST,
               "fused", {"kernel": TILE128}, nested=(False,))
    for bs in (128, 256):
        c += _both(f"tile128-r70-bs{bs}", "k_gemm_4bit", "gemm", {"cgemm_4bit_set_tile": 128}, 300, 70, 1024, bs,
                   DEQUANT_FIRST, "fused", {"kernel": TILE128}, nested=(False,))
    c += _both("tile256-r300-split", "k_gemm_4bit_256", "gemm", {"cgemm_4bit_set_tile": 256}, 300, 300, 1024, 64,
               DEQUANT_FIRST, "fused", {"kernel": TILE256, "split": True}, nested=(False,))
    c += _both("tile256-r300-whole", "k_gemm_4bit_256", "gemm", {"cgemm_4bit_set_tile": 256}, 300, 300, 256, 64,
               DEQUANT_FIRST, "fused", {"kernel": TILE256, "split": False}, nested=(False,))
    for bs in (128, 256):
        c += _both(f"tile256-r300-bs{bs}", "k_gemm_4bit_256", "gemm", {"cgemm_4bit_set_tile": 256}, 300, 300, 1024, bs,
                   DEQUANT_FIRST, "fused", {"kernel": TILE256, "split": True}, nested=(False,))
    # dequantise + k_hgemm at 300 rows.  At N = 300 the plan returns the 128 x 128 tile only (split-K from K = 1024,
    # whole K at 512); the other tile shapes need N >= 10884 at 300 rows, probed at K = 64 (64 calls) to stay small.
    for K, sp in ((1024, True), (2048, True), (512, False)):
        c += _both(f"hgemm-r300-k{K}", "k_hgemm", "gemm", {}, 300, 300, K, 64, DEQUANT_FIRST, "hgemm",
                   {"wi": 4, "wj": 4, "split": sp})
    for N, wi, wj in ((10884, 8, 4), (16388, 4, 8), (21764, 8, 8)):
        c += _both(f"hgemm-r300-tile{wi}x{wj}", "k_hgemm", "gemm", {}, N, 300, 64, 64, DEQUANT_FIRST, "hgemm",
                   {"wi": wi, "wj": wj, "split": False}, nested=(False,))
    for bs in (128, 256):
        c += _both(f"hgemm-r300-bs{bs}", "k_hgemm", "gemm", {}, 300, 300, 1024, bs, DEQUANT_FIRST, "hgemm",
                   {"wi": 4, "wj": 4, "split": True})
    # the one-row GEMVs.  N is ragged against each kernel's own row group (gemv4bit.hip): k_gemv_4bit_dot at K = 1024
    # runs <T, 8, 1>, 8 rows per wave and 32 per workgroup; k_gemv_4bit<float, 4> 4 rows per wave; the generic kernel 4
    # rows per workgroup: N = 203.  k_gemv_4bit_bal spreads N rows over G = min(2 CUs, N) workgroups, N / G rows each
    # and one more in the first N % G: N = 203 (one row, one wave each), 1100 (G = 512: 3 and 2 rows, one row per wave)
    # and 6501 (13 and 12 rows: two rows per wave, the last wave one).  k_gemv_4bit_wide: N / CUs rows per workgroup.
    gv = "cgemv_4bit_set_kernel"
    c += _both("gemv-dot", "k_gemv_4bit_dot", "gemv", {gv: 1}, 203, 1, 1024, 64, GEMV, None, None,
               why="set_kernel(1): launch_gemv_dot skips the wide and the balanced kernel")
    c += _both("gemv-bal", "k_gemv_4bit_bal", "gemv", {gv: 3}, 203, 1, 1024, 64, GEMV, None, None,
               why="set_kernel(3): no wide kernel; launch_gemv_bal fits (one row per wave, U = 1)")
    c += _both("gemv-bal-n1100", "k_gemv_4bit_bal", "gemv", {gv: 3}, 1100, 1, 1024, 64, GEMV, None, None,
               why="set_kernel(3); 512 workgroups of 3 / 2 rows, one row per wave")
    c += _both("gemv-bal-n6501", "k_gemv_4bit_bal", "gemv", {gv: 3}, 6501, 1, 1024, 64, GEMV, None, None,
               why="set_kernel(3); 512 workgroups of 13 / 12 rows, two rows per wave (R = 2)")
    c += _both("gemv-wide", "k_gemv_4bit_wide", "gemv", {gv: 2}, 601, 1, 2048, 64, GEMV, None, None,
               why="set_kernel(2): gemv_wide_preferred; 601 rows / 256 CUs -> two rows per workgroup, the last has one")
    c += _both("gemv-wide-1row", "k_gemv_4bit_wide", "gemv", {gv: 2, "cgemv_4bit_set_wide_rows": 1}, 601, 1, 2048, 64,
               GEMV, None, None, why="set_wide_rows(1): the wide kernel with one row per workgroup")
    c += _both("gemv-auto", "k_gemv_4bit_wide", "gemv", {}, 203, 1, 1024, 64, GEMV, None, None,
               why="no knob: fewer rows than CUs -> the wide kernel")
    for bs in (128, 256):
        c += _both(f"gemv-dot-bs{bs}", "k_gemv_4bit_dot", "gemv", {gv: 1}, 203, 1, 1024, bs, GEMV, None, None)
        c += _both(f"gemv-bal-bs{bs}", "k_gemv_4bit_bal", "gemv", {gv: 3}, 1100, 1, 1024, bs, GEMV, None, None)
        c += _both(f"gemv-wide-bs{bs}", "k_gemv_4bit_wide", "gemv", {gv: 2}, 601, 1, 2048, bs, GEMV, None, None)
    # fp32 activations run k_gemv_4bit<float> (fp32 codes: round_T is the identity)
    c += _both("gemv-fp32", "k_gemv_4bit", "gemv", {}, 203, 1, 1024, 64, GEMV, None, None, kinds=("fp32",),
               nested=(False,), why="sizeof(T) == 4: the table/dot kernels are 16-bit only")
    # K = 200: K % 32 != 0 -> k_gemv_4bit_generic; blocks straddle weight rows (absmax by the flat element index) and
    # its codes stay fp32: x * (code * absmax), the dequantise-first value
    c += _both("gemv-generic", "k_gemv_4bit_generic", "gemv", {}, 203, 1, 200, 64, DEQUANT_FIRST, None, None,
               kinds=("bf16", "fp16", "fp32"), nested=(False,), why="K % 32 != 0: not `fast` in gemv_4bit")
    for bs in (128, 256):
        c += _both(f"gemv-fp32-bs{bs}", "k_gemv_4bit", "gemv", {}, 203, 1, 1024, bs, GEMV, None, None, kinds=("fp32",),
                   nested=(False,))
        c += _both(f"gemv-generic-bs{bs}", "k_gemv_4bit_generic", "gemv", {}, 203, 1, 200, bs, DEQUANT_FIRST, None,
                   None, kinds=("bf16", "fp16", "fp32"), nested=(False,))
    return c


CASES = _cases()
FAMILY = ("k_gemv_4bit_dot", "k_gemv_4bit_bal", "k_gemv_4bit_wide", "k_gemv_4bit_generic", "k_gemv_4bit_tok",
          "k_gemm_4bit_fewtok", "k_gemm_4bit_t64", "k_gemm_4bit_t64r", "k_gemm_4bit_wk", "k_gemm_4bit_skinny",
          "k_gemm_4bit", "k_gemm_4bit_256", "k_hgemm")


def case_id(case):
    return case.id


def check_case_plan(case):
    """Assert that `case` selects its kernel under its knobs (CPU: the plan queries need no device)."""
    if case.plan is None:
        return
    want = dict(case.plan)
    split = want.pop("split", None)
    with knobs(case.knobs):
        if case.route == "hgemm":
            p = hgemm_plan(case.rows, case.N, case.K)
        else:
            p = gemm_plan(case.N, case.rows, case.K, case.blocksize, case.nested)
    got = {k: p[k] for k in want}
    assert got == want, (case.id, got, want, p)
    if split is not None:
        assert (p["splits"] > 1) == split, (case.id, p)
        if case.route != "hgemm" and case.plan["kernel"] != T64R:
            assert bool(p["reduce"]) == split, (case.id, p)


# ------------------------------------------------------------------------------------------------ weights
def table_of(quant_type):
    return ref.nf4_table() if quant_type == "nf4" else ref.fp4_table()


def probe_codes(N, K, seed):
    """Seeded uniform 4-bit codes [N, K] and their packed bytes (high nibble = even element)."""
    q = np.random.default_rng(seed).integers(0, 16, size=N * K, dtype=np.uint8)
    packed = ((q[0::2] << 4) | q[1::2]).astype(np.uint8)
    return q.reshape(N, K), packed


def pow2_absmax(nblocks):
    """2^e_b, e_b = ((5 b + 3) % 7) - 3: neighbouring blocks differ by a factor of >= 2, and so do blocks one weight
    row apart wherever the blocks per row are no multiple of 7."""
    b = np.arange(nblocks, dtype=np.int64)
    return np.exp2((((5 * b + 3) % 7) - 3).astype(F32)).astype(F32)


def pin_absmax(nblocks):
    """Non-power-of-two statistics for the contract pins."""
    b = np.arange(nblocks, dtype=np.int64)
    return (F32(0.0537) * (1 + b % 5).astype(F32)).astype(F32)


def nblocks(N, K, blocksize):
    return (N * K + blocksize - 1) // blocksize


def absmax_per_element(absmax, N, K, blocksize):
    """absmax of element (n, k): indexed by the flat element index (blocks may straddle weight rows)."""
    return np.repeat(np.asarray(absmax, dtype=F32), blocksize)[:N * K].reshape(N, K)


# ------------------------------------------------------------------------------------------------ expectations
def round_T(v, kind):
    return ref.round_to(np.asarray(v, dtype=F32), kind)


def expect_dequant_first(x, code, absmax, kind):
    """The weight dequantised in fp32 and rounded once to T, the product rounded to T."""
    w = round_T(np.asarray(code, F32) * np.asarray(absmax, F32), kind)
    return round_T(np.asarray(x, F32) * w, kind)


def expect_gemv(x, code, absmax, kind):
    """(sum x * T(code)) * absmax in fp32 (fp32 activations: fp32 codes), rounded to T at the store."""
    c = round_T(code, kind)
    s = (np.asarray(x, F32) * c).astype(F32)
    return round_T(s * np.asarray(absmax, F32), kind)


def expect_tcode_mfma(x, code, absmax, kind):
    """T(code) * x on the MFMA (exact fp32 product), the block sum scaled by the fp32 absmax with one fma onto the
    other blocks' sum (zero on a one-hot row), rounded to T at the store."""
    s = (round_T(code, kind) * np.asarray(x, F32)).astype(F32)
    return round_T((s.astype(np.float64) * np.asarray(absmax, F32).astype(np.float64) + 0.0).astype(F32), kind)


EXPECT = {DEQUANT_FIRST: expect_dequant_first, GEMV: expect_gemv, TCODE_MFMA: expect_tcode_mfma}


def expected_weight(q, absmax, blocksize, quant_type, kind, contract):
    """[N, K] fp32: what a unit activation at k yields at output n under `contract`.  The probes' activations are powers
    of two, which commute with every rounding above (no subnormal or overflow in the probes' ranges;
    test_4bit_probe_routes_cpu.py checks that on every value used), so Y[m, n] == x_m * this[n, k_m]."""
    N, K = q.shape
    am = absmax_per_element(absmax, N, K, blocksize)
    return EXPECT[contract](F32(1.0), table_of(quant_type)[q], am, kind)


# ------------------------------------------------------------------------------------------------ activations
PROBE_VALUES = np.array([s * 2.0 ** j for s in (1.0, -1.0) for j in (-1, 0, 1, 2)], dtype=F32)


def probe_k(m, c, K):
    return (37 * m + c) % K


def probe_value(m, c):
    """+-2^j, j = ((m + c) % 4) - 1, negative when (m + c) // 4 is odd."""
    return PROBE_VALUES[(m + c) % 8]


# ------------------------------------------------------------------------------------------------ device side
def torch_dtype(kind):
    import torch
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[kind]


def make_weight(F, dev, N, K, blocksize, quant_type, kind, packed, absmax):
    """code and QuantState from quantize_4bit of a zero tensor of that shape; packed bytes and absmax overwritten."""
    import torch
    qz, st = F.quantize_4bit(torch.zeros(N, K, device=dev, dtype=torch_dtype(kind)), blocksize=blocksize,
                             quant_type=quant_type)
    qz.copy_(torch.from_numpy(packed).to(dev).view_as(qz))
    st.absmax.copy_(torch.from_numpy(np.asarray(absmax, dtype=F32)).to(dev))
    return qz, st


def make_nested_weight(F, dev, N, K, blocksize, quant_type, kind, packed, seed):
    """Arbitrary nested statistics: those of a quantised Gaussian tensor; the packed bytes overwritten."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = torch.randn(N, K, generator=g).to(dev).to(torch_dtype(kind))
    qz, st = F.quantize_4bit(W, blocksize=blocksize, quant_type=quant_type, compress_statistics=True)
    qz.copy_(torch.from_numpy(packed).to(dev).view_as(qz))
    return qz, st


def plain_state(F, st, absmax):
    return F.QuantState(absmax=absmax, shape=st.shape, dtype=st.dtype, blocksize=st.blocksize, code=st.code,
                        quant_type=st.quant_type)


def runner(F, case, q, st, absmax=None):
    """X [rows, K] -> Y [rows, N] on the case's route (the caller holds the knobs)."""
    if case.api == "gemv":
        state = st if absmax is None else plain_state(F, st, absmax)
        return lambda X: F.gemv_4bit(X, q.t(), state=state)
    return lambda X: F.gemm_4bit(X, q, st, absmax=absmax, _route=case.route)


class Sweep:
    """The one-hot activations of calls c = 0 .. width - 1 for `rows` rows of width `width`, built on the device: row m
    of call c holds probe_value(m, c) at probe_k(m, c, width).  round_product: compare with the exact product rounded to
    the activations' type -- for operands whose product need not be a value of that type (a subnormal fp16 product in
    the hand-driven k_hgemm sweeps); in the 4-bit probes every product is one (test_4bit_probe_routes_cpu.py)."""

    def __init__(self, dev, rows, width, kind, round_product=False):
        import torch
        self.rows, self.width, self.round_product = rows, width, round_product
        self.m = torch.arange(rows, device=dev)
        c = torch.arange(width, device=dev)[:, None]
        self.k = (37 * self.m[None, :] + c) % width                           # [calls, rows]
        self.v = torch.from_numpy(PROBE_VALUES).to(dev)[(self.m[None, :] + c) % 8]
        self.vT = self.v.to(torch_dtype(kind))
        self.X = torch.zeros(rows, width, device=dev, dtype=torch_dtype(kind))

    def put(self, c):
        """Write call c's nonzeros into X; returns (k index per row, fp32 value per row)."""
        k = self.k[c]
        self.X[self.m, k] = self.vT[c]
        return k, self.v[c]

    def clear(self, k):
        self.X[self.m, k] = 0


def sweep_mismatches(run, Et, sweep, first=False):
    """Run every call of the sweep through `run` and compare with Et[k_m] * x_m (Et: [width, out] fp32, the expectation
    transposed) as values: zeros of either sign are equal, a NaN is a mismatch.  Returns the mismatch count after one
    synchronisation -- or, with first=True, the first mismatch as (c, m, n, k, got, want), checked per call."""
    import torch
    bad = torch.zeros((), dtype=torch.int64, device=Et.device)
    for c in range(sweep.width):
        k, v = sweep.put(c)
        Y = run(sweep.X).reshape(sweep.rows, -1).float()
        E = Et[k] * v[:, None]
        if sweep.round_product:
            E = E.to(sweep.X.dtype).float()
        ne = Y != E
        if first:
            if bool(ne.any()):
                m, n = [int(i) for i in ne.nonzero()[0]]
                return (c, m, n, int(k[m]), float(Y[m, n]), float(E[m, n]))
        else:
            bad += ne.sum()
        sweep.clear(k)
    return None if first else int(bad)


def assert_sweep_exact(run, Et, sweep, what):
    n = sweep_mismatches(run, Et, sweep)
    if n:
        sweep.X.zero_()
        c, m, nn, k, got, want = sweep_mismatches(run, Et, sweep, first=True)
        raise AssertionError(f"{what}: {n} outputs differ; first at (c, m, n, k) = ({c}, {m}, {nn}, {k}): "
                             f"got {got!r}, expected {want!r}")


def sweep_bit_differences(run_a, run_b, sweep):
    """Count of outputs whose bits differ between two routes over the whole sweep (one synchronisation)."""
    import torch
    bad = torch.zeros((), dtype=torch.int64, device=sweep.X.device)
    for c in range(sweep.width):
        k, _ = sweep.put(c)
        Ya, Yb = run_a(sweep.X), run_b(sweep.X)
        bad += (bits(Ya) != bits(Yb)).sum()
        sweep.clear(k)
    return int(bad)


def bits(t):
    import torch
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ------------------------------------------------------------------------------------------------ poisoned arenas
ARENA_ALIGN = 256


def in_arena(t, pad_elems, poison):
    """A copy of contiguous `t` inside a larger buffer of its dtype, at a 256-byte-aligned offset with at least
    pad_elems elements of `poison` (a float, or a byte value for uint8 / int8) before and after it.  Returns
    (buffer, view)."""
    import torch
    esz = t.element_size()
    unit = ARENA_ALIGN // esz
    pad = (max(pad_elems, 1) + unit - 1) // unit * unit
    n = t.numel()
    buf = torch.full((2 * pad + (n + unit - 1) // unit * unit,), poison, dtype=t.dtype, device=t.device)
    view = buf[pad:pad + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + pad * esz and view.data_ptr() % ARENA_ALIGN == 0
    return buf, view


# ------------------------------------------------------------------------------------------------ grouped checks
def by_kernel(cases):
    """[(kernel, [its cases])] in table order: one test item per kernel where a case each would be too many items."""
    groups = {}
    for c in cases:
        groups.setdefault(c.kernel, []).append(c)
    return list(groups.items())


class Failures:
    """Several labelled checks in one test item: every failed assertion is kept and all are reported at the end, so
    one failing variant does not hide the next.  Only AssertionError is held back; any other error ends the test."""

    def __init__(self):
        self.messages = []

    @contextlib.contextmanager
    def check(self, label):
        try:
            yield
        except AssertionError as e:
            self.messages.append(f"[{label}] {e}")

    def assert_none(self):
        assert not self.messages, f"{len(self.messages)} failed:\n" + "\n".join(self.messages)
