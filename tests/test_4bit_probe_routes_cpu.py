"""The route table of the exact 4-bit probes (probe4bit_helpers.CASES), checked without a GPU: cgemm_4bit_plan and
chgemm_tn_plan must name each case's kernel under the case's knobs (as test_fewtoken_plan_cpu.py does for the default
plan; without a device the CU count is the MI355X's 256), so a later routing change cannot silently take a kernel out
of the probes.  Plus the helper's own arithmetic: the three expected-value functions against the fp64 oracle on
one-hot inputs, and that the expectation really depends on which statistics block an element belongs to."""
import numpy as np
import pytest

import probe4bit_helpers as ph
from oracle import ref

F32 = np.float32


@pytest.mark.parametrize("case", ph.CASES, ids=ph.case_id)
def test_case_selects_its_kernel(case):
    ph.check_case_plan(case)


def test_knobs_go_back_to_their_defaults():
    """After a knobs() block (also one left by an exception) the default plan is back."""
    before = ph.gemm_plan(200, 8, 1024)
    with pytest.raises(RuntimeError):
        with ph.knobs({"cgemm_4bit_set_fewtoken_kernel": 1, "cgemm_4bit_set_skinny_config": 2}):
            assert ph.gemm_plan(200, 8, 1024)["kernel"] == ph.SKINNY
            raise RuntimeError("leave by exception")
    assert ph.gemm_plan(200, 8, 1024) == before
    with ph.knobs({"cgemm_4bit_set_tile": 128, "cgemm_4bit_set_t64_splits": 1, "cgemm_4bit_set_t64_regfed": 2}):
        assert ph.gemm_plan(200, 8, 1024)["kernel"] == ph.TILE128
    assert ph.gemm_plan(200, 8, 1024) == before and ph.gemm_plan(200, 33, 1024)["kernel"] == ph.T64


def test_knob_defaults_are_the_library_defaults():
    """KNOB_DEFAULTS restates the C side's defaults: the plans of every table shape as the library starts, and again
    after each plan knob was set to another value and put back by knobs(), are the same."""
    shapes = sorted({(c.N, c.rows, c.K, c.blocksize, c.nested) for c in ph.CASES if c.api == "gemm"})
    before = [ph.gemm_plan(*s) for s in shapes]
    assert {p["kernel"] for p in before} >= {ph.GEMV_TOK, ph.T64, ph.SKINNY, ph.TILE256, ph.NONE}
    other = {"cgemm_4bit_set_tile": 128, "cgemm_4bit_set_fewtoken_kernel": 1, "cgemm_4bit_set_skinny_config": 2,
             "cgemm_4bit_set_fewtok_mode": 2, "cgemm_4bit_set_t64_mode": 1, "cgemm_4bit_set_t64_regfed": 2,
             "cgemm_4bit_set_t64_splits": 1}
    assert set(other) == {k for k in ph.KNOB_DEFAULTS if k.startswith("cgemm_")}
    for name, value in other.items():
        with ph.knobs({name: value}):
            assert [ph.gemm_plan(*s) for s in shapes] != before, name     # the knob is seen by these shapes
        assert [ph.gemm_plan(*s) for s in shapes] == before, name


def test_table_covers_the_family_and_the_shapes_that_matter():
    by_kernel = {}
    for c in ph.CASES:
        by_kernel.setdefault(c.kernel, []).append(c)
    assert set(ph.FAMILY) <= set(by_kernel)
    ids = [c.id for c in ph.CASES]
    assert len(ids) == len(set(ids))

    def rows(k):
        return {c.rows for c in by_kernel[k]}

    assert rows("k_gemv_4bit_tok") >= {2, 4} and rows("k_gemm_4bit_fewtok") >= {5, 17, 32}
    assert rows("k_gemm_4bit_wk") == {8} and rows("k_gemm_4bit_skinny") >= {8, 48}
    assert rows("k_gemm_4bit_t64") == {33, 64} and rows("k_gemm_4bit_t64r") == {33, 64}
    assert rows("k_gemm_4bit") == {70} and rows("k_gemm_4bit_256") == {300} and rows("k_hgemm") == {300}
    assert any(c.N == 1 for c in by_kernel["k_gemm_4bit_fewtok"])
    # ragged against the row group / tile; 16-bit in both formats for every kernel; blocksizes 128 and 256 where taken
    for k, cs in by_kernel.items():
        if not k.startswith("k_gemv_4bit"):              # (the GEMVs: test_gemv_cases_are_ragged_against_...)
            tile = {"k_gemm_4bit": 128, "k_gemm_4bit_256": 256, "k_hgemm": 128}.get(k, 16)
            assert any(c.N % tile for c in cs), k
        assert any(set(c.kinds) >= {"bf16", "fp16"} for c in cs) or k == "k_gemv_4bit", k
        if k not in ("k_gemm_4bit_t64", "k_gemm_4bit_t64r"):
            assert {c.blocksize for c in cs} >= {64, 128, 256}, k
    # every split-K form really splits, and the in-kernel nested decode is probed wherever a kernel has one
    for k in ("k_gemm_4bit_256", "k_gemm_4bit_skinny", "k_gemm_4bit_t64", "k_hgemm"):
        assert any(c.plan.get("split") for c in by_kernel[k]), k
    for k in ph.FAMILY:
        if k not in ("k_gemm_4bit", "k_gemm_4bit_256", "k_gemv_4bit_generic"):
            assert any(c.nested for c in by_kernel[k]), k
    assert all(c.K % 256 == 0 for c in by_kernel["k_gemm_4bit_t64"])
    assert {c.K for c in by_kernel["k_gemv_4bit_generic"]} == {200}
    assert {(c.plan["wi"], c.plan["wj"]) for c in by_kernel["k_hgemm"]} == {(4, 4), (8, 4), (4, 8), (8, 8)}


def test_gemv_cases_are_ragged_against_their_row_groups():
    """Each GEMV kernel's own row group, restated from its launch code (gemv4bit.hip launch_gemv_dot, launch_gemv_bal,
    launch_gemv_wide, gemv_4bit; gemv4bit_tok.hip gemv_tok_plan; 256 CUs): the tail guards `min(row0 + r, M - 1)` /
    `if (row0 + r < M)` and the uneven N / G, N % G row split only run where N is no multiple of the group."""
    cus = 256
    by_kernel = dict(ph.by_kernel(ph.CASES))
    for c in by_kernel["k_gemv_4bit_dot"]:                # <T, R, U> by K / 32 chunks: R rows per wave, 4 waves
        nch = c.K // 32
        R = 8 if nch <= 64 else 4 if nch <= 128 else 2 if nch <= 256 else 1
        assert R == 8 and c.N % R and c.N % (4 * R), c.id
    for k in ("k_gemv_4bit", "k_gemv_4bit_generic"):      # 4 rows per wave of 4 waves / 4 rows per workgroup
        assert all(c.N % 4 and c.N % 16 for c in by_kernel[k]), k
    bal = []
    for c in by_kernel["k_gemv_4bit_bal"]:                # G workgroups of N / G rows, one more in the first N % G
        G = min(2 * cus, c.N)
        rows = -(-c.N // G)
        R = -(-rows // (8 if c.nested else 12))           # rows per wave (U = 1 at K = 1024, two workgroups per CU)
        assert c.K == 1024 and R <= 4, c.id
        bal.append((c.nested, c.blocksize, rows, R, -(-rows // R), c.N % G))
    for nested in (False, True):
        mine = [b for b in bal if b[0] == nested]
        assert any(rows == 1 for _, _, rows, _, _, _ in mine)                        # one row, one wave
        assert any(R == 1 and nw > 1 and rem for _, _, _, R, nw, rem in mine)        # several waves, uneven split
        assert any(R == 2 and rows % R and rem for _, _, rows, R, _, rem in mine)    # two rows per wave, odd tail
        assert all(rem for _, bs, _, _, _, rem in mine if bs != 64)
    wide = [(max(1, min(4, c.N // cus)), c) for c in by_kernel["k_gemv_4bit_wide"]]
    assert any(R == 2 and c.N % R and not c.knobs.get("cgemv_4bit_set_wide_rows") for R, c in wide)
    assert any(R == 1 for R, c in wide) and any(c.knobs.get("cgemv_4bit_set_wide_rows") == 1 for _, c in wide)
    tok = []
    for c in by_kernel["k_gemv_4bit_tok"]:                # the plan reports G (grid), R (rg) and the waves
        with ph.knobs(c.knobs):
            p = ph.gemm_plan(c.N, c.rows, c.K, c.blocksize, c.nested)
        tok.append((c.rows, c.nested, p["grid"] < c.N and c.N % p["grid"] != 0 and p["waves"] > 1))
    for rows in (2, 4):
        for nested in (False, True):
            assert any(r == rows and n == nested and ragged for r, n, ragged in tok), (rows, nested)


def test_t64_declines_other_blocksizes():
    """Why the table has no blocksize 128 / 256 case for k_gemm_4bit_t64{,r}: the plan does not give them the kernel."""
    for bs in (128, 256):
        with ph.knobs({"cgemm_4bit_set_fewtok_mode": 1}):
            assert ph.gemm_plan(200, 33, 1024, bs)["kernel"] not in (ph.T64, ph.T64R)
        with ph.knobs({"cgemm_4bit_set_fewtok_mode": 1, "cgemm_4bit_set_t64_regfed": 2}):
            assert ph.gemm_plan(200, 33, 1024, bs)["kernel"] not in (ph.T64, ph.T64R)


def _all_inputs(kind, quant_type, absmax_values):
    """Every (x, code, absmax) triple the probes can form: 8 activation values x 16 codes x the statistics used."""
    x, code, am = np.meshgrid(ph.PROBE_VALUES, ph.table_of(quant_type), np.asarray(absmax_values, dtype=F32),
                              indexing="ij")
    return x.ravel(), code.ravel(), am.ravel()


@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp32"])
def test_contracts_agree_on_power_of_two_statistics(kind, quant_type):
    """With absmax = 2^e, e in [-3, 3], all three contracts give x * round_T(code) * 2^e: exactly, finite, and with no
    subnormal result except zero."""
    x, code, am = _all_inputs(kind, quant_type, ph.pow2_absmax(7))
    assert set(np.log2(ph.pow2_absmax(7))) == set(range(-3, 4))
    want = (x.astype(np.float64) * ph.round_T(code, kind).astype(np.float64) * am.astype(np.float64))
    tiny = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14, "fp32": 2.0 ** -126}[kind]
    assert np.all((want == 0) | (np.abs(want) >= tiny)) and np.all(np.isfinite(want))
    for fn in ph.EXPECT.values():
        got = fn(x, code, am, kind)
        assert np.array_equal(got.astype(np.float64), want), fn.__name__


@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_contract_pins_are_not_vacuous_and_scale_by_the_probe_values(kind, quant_type):
    """With the pins' statistics 0.0537 (1 + b % 5): the dequantise-first and T(code) classes differ on some codes (so
    a route is pinned to its class), and every class commutes with the power-of-two activations
    (expected_weight's premise: f(x, code, absmax) == x * f(1, code, absmax))."""
    x, code, am = _all_inputs(kind, quant_type, ph.pin_absmax(5))
    out = {name: fn(x, code, am, kind) for name, fn in ph.EXPECT.items()}
    assert np.any(out[ph.DEQUANT_FIRST] != out[ph.TCODE_MFMA]) and np.any(out[ph.DEQUANT_FIRST] != out[ph.GEMV])
    one = np.ones_like(x)
    for name, fn in ph.EXPECT.items():
        assert np.array_equal(out[name], x * fn(one, code, am, kind)), name
        assert np.all(np.isfinite(out[name]))
    table = ph.table_of(quant_type)
    differ = sum(1 for cv in table if np.any(ph.expect_dequant_first(one[:5], cv, ph.pin_absmax(5), kind)
                                             != ph.expect_tcode_mfma(one[:5], cv, ph.pin_absmax(5), kind)))
    assert differ >= 2, differ


@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("stats", ["pow2", "pin"])
def test_expectations_against_the_fp64_oracle_on_one_hot_rows(kind, quant_type, stats):
    """oracle.ref.gemm_4bit_dequant_ref (the fp64 product of the once-rounded weight) rounded once to T, on the probes'
    one-hot rows: equal exactly for the dequantise-first class (both statistics), and for all classes with power-of-two
    statistics.  K = 200 at blocksize 64: blocks straddle weight rows."""
    N, K, bs, rows = 24, 200, 64, 9
    q, packed = ph.probe_codes(N, K, seed=11)
    absmax = (ph.pow2_absmax if stats == "pow2" else ph.pin_absmax)(ph.nblocks(N, K, bs))
    table = ph.table_of(quant_type)
    for c in (0, 1, 63, 64, 199):
        X = np.zeros((rows, K), dtype=F32)
        ks = [ph.probe_k(m, c, K) for m in range(rows)]
        for m in range(rows):
            X[m, ks[m]] = ph.probe_value(m, c)
        oracle = ph.round_T(ref.gemm_4bit_dequant_ref(X, packed, absmax, N, K, bs, table, kind).astype(F32), kind)
        for name in ph.EXPECT:
            W = ph.expected_weight(q, absmax, bs, quant_type, kind, name)
            mine = np.stack([X[m, ks[m]] * W[:, ks[m]] for m in range(rows)])
            if name == ph.DEQUANT_FIRST or stats == "pow2":
                assert np.array_equal(mine, oracle), (name, c)


def test_probe_rows_cover_every_k_once():
    for rows, K in ((5, 1024), (300, 1024), (1, 200), (64, 2048)):
        for m in (0, rows - 1):
            assert sorted(ph.probe_k(m, c, K) for c in range(K)) == list(range(K))
    assert {float(ph.probe_value(m, 0)) for m in range(8)} == {0.5, 1.0, 2.0, 4.0, -0.5, -1.0, -2.0, -4.0}


@pytest.mark.parametrize("blocksize,K", [(64, 1024), (64, 2048), (64, 4096), (128, 1024), (256, 1024), (64, 200),
                                         (64, 64), (64, 208), (64, 512), (64, 256)])
def test_a_moved_statistics_block_changes_every_probed_position(blocksize, K):
    """The probes can see a statistics-index error: neighbouring blocks, and the blocks one weight row apart, differ by
    a factor of >= 2, and with every block given the statistic of the next block (or of the block one weight row on)
    the expectation changes at every position whose code is not the zero code."""
    N = 12
    nb = ph.nblocks(N, K, blocksize)
    am = ph.pow2_absmax(nb)
    per_row = max(1, K // blocksize)
    for shift in (1, per_row):
        moved = ph.pow2_absmax(nb + shift)[shift:]
        ratio = np.maximum(am, moved) / np.minimum(am, moved)
        assert np.all(ratio >= 2.0), (shift, K, blocksize)
        q, _ = ph.probe_codes(N, K, seed=5)
        for kind in ("bf16", "fp16"):
            a = ph.expected_weight(q, am, blocksize, "nf4", kind, ph.DEQUANT_FIRST)
            b = ph.expected_weight(q, moved, blocksize, "nf4", kind, ph.DEQUANT_FIRST)
            assert np.array_equal(a != b, q != 7)          # NF4 code 7 is 0.0: the only value no scale can change


def test_device_sweep_is_the_scalar_definition():
    """Sweep (the tables the GPU tests index) against probe_k / probe_value, and the mismatch count / first-mismatch
    report of sweep_mismatches, on CPU tensors with a plain product standing in for the kernel."""
    import torch
    rows, K = 7, 200
    sweep = ph.Sweep(torch.device("cpu"), rows, K, "bf16")
    for c in (0, 3, K - 1):
        k, v = sweep.put(c)
        assert [int(x) for x in k] == [ph.probe_k(m, c, K) for m in range(rows)]
        assert [float(x) for x in v] == [float(ph.probe_value(m, c)) for m in range(rows)]
        assert int((sweep.X != 0).sum()) == rows and all(float(sweep.X[m, k[m]]) == float(v[m]) for m in range(rows))
        sweep.clear(k)
        assert int((sweep.X != 0).sum()) == 0
    W = torch.randn(5, K, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    Et = W.t().float().contiguous()
    assert ph.sweep_mismatches(lambda X: X @ W.t(), Et, sweep) == 0
    W2 = W.clone()
    W2[3, 77] += 1.0                                          # one wrong element: seen by every row, once each
    assert ph.sweep_mismatches(lambda X: X @ W2.t(), Et, sweep) == rows
    W2[3, 77] = float("nan")                                  # a NaN weight reaches output 3 of every row in every call
    assert ph.sweep_mismatches(lambda X: X @ W2.t(), Et, sweep) == rows * K
    c, m, n, k, got, want = ph.sweep_mismatches(lambda X: X @ W.roll(1, 1).t(), Et, sweep, first=True)
    assert (c, m, n, k) == (0, 0, 0, 0) and got != want


def test_grouped_checks_report_every_failure():
    """Failures (several variants in one test item): every failed assertion is reported, another error is not held."""
    fails = ph.Failures()
    with fails.check("a"):
        assert 1 == 2, "first"
    with fails.check("b"):
        pass
    with fails.check("c"):
        assert False, "third"
    with pytest.raises(AssertionError) as e:
        fails.assert_none()
    assert "2 failed" in str(e.value) and "[a] first" in str(e.value) and "[c] third" in str(e.value)
    ph.Failures().assert_none()
    with pytest.raises(RuntimeError):
        with ph.Failures().check("d"):
            raise RuntimeError("not a failed check")
    assert [k for k, _ in ph.by_kernel(ph.CASES)] == list(dict.fromkeys(c.kernel for c in ph.CASES))
    assert sum(len(g) for _, g in ph.by_kernel(ph.CASES)) == len(ph.CASES)
