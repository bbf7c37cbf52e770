"""Quantile code books without a GPU: the C-ABI and Python surface exists, the numpy restatement of the estimate
(tests/quantile_helpers.py) behaves as DESIGN.md §4e says, create_fp8_map reproduces the recorded reference maps, and
estimate_quantiles keeps the reference's refusals."""
import os
import re

import numpy as np
import pytest
import torch

import quantile_helpers as qh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cestimate_quantiles_fp32", "cestimate_quantiles_fp16", "cestimate_quantiles_bf16",
           "chistogram_scatter_add_2d")
FP8_CASES = [(True, 4, 3, 8), (True, 5, 2, 8), (False, 5, 3, 8), (True, 3, 2, 6), (True, 2, 1, 4)]


def _F():
    import python_src_quants.functional as F
    return F


def test_header_declares_the_quantile_symbols():
    txt = open(os.path.join(ROOT, "include", "bnb_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", txt))
    assert set(SYMBOLS) <= declared, sorted(set(SYMBOLS) - declared)
    import python_src_quants as bnb
    for sym in SYMBOLS:
        assert hasattr(bnb.lib._lib, sym), sym
    for name in ("estimate_quantiles", "create_quantile_map", "create_fp8_map", "histogram_scatter_add_2d"):
        assert callable(getattr(bnb.functional, name)), name


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("valid", [256, 257, 1000, 4095, 4096])
@pytest.mark.parametrize("offset", [0.0, 1 / 512, 1 / 510, 0.02])
def test_indices_are_monotone_and_collide_only_where_expected(valid, offset):
    idx = qh.quantile_indices(valid, offset)
    assert idx.shape == (256,) and idx[0] >= 0 and idx[-1] <= valid - 1
    assert np.all(np.diff(idx) >= 0)
    distinct = {(256, 0.02): 246, (257, 0.02): 247, (256, 1 / 510): 255, (257, 1 / 510): 255}.get((valid, offset), 256)
    assert np.unique(idx).size == distinct


def test_indices_reach_both_ends_at_offset_zero():
    for valid in (256, 1000, 4096):
        idx = qh.quantile_indices(valid, 0.0)
        assert idx[0] == 0 and idx[-1] == valid - 1
    assert np.array_equal(qh.quantile_indices(256, 0.0), np.arange(256))


def test_restatement_permutation_returns_the_indices():
    rng = np.random.default_rng(0)
    x = rng.permutation(4096).astype(np.float32)
    for offset in (1 / 512, 0.02, 0.0):
        code = qh.estimate_quantiles(x, offset)
        assert code.dtype == np.float32
        assert np.array_equal(code, qh.quantile_indices(4096, offset).astype(np.float32))


def test_restatement_mean_over_blocks_and_ignored_tail():
    rng = np.random.default_rng(1)
    blocks = 3
    x = np.concatenate([rng.permutation(4096) + 4096 * b for b in range(blocks)] + [np.full(7, 1e30)]).astype(np.float32)
    code = qh.estimate_quantiles(x, 1 / 512)
    assert np.array_equal(code, (qh.quantile_indices(4096, 1 / 512) + 4096 * (blocks - 1) / 2).astype(np.float32))


def test_restatement_signed_zeros_and_total_order():
    x = np.tile(np.array([0.0, -0.0], np.float32), 128)
    code = qh.estimate_quantiles(x, 1 / 512)
    assert np.all(code == 0) and not np.any(np.signbit(code))       # the sum starts from +0.0
    nan_neg = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    special = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf, nan_neg], np.float32)
    got = qh.total_order_sort(special).view(np.uint32)
    want = np.array([nan_neg, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], np.float32).view(np.uint32)
    assert np.array_equal(got, want)


def test_restatement_colliding_indices_all_get_the_value():
    # valid = 256 at offset 0.02: 246 distinct indices; the reference's LDS race would leave 10 entries at zero
    x = (np.random.default_rng(2).permutation(256) + 1).astype(np.float32)
    code = qh.estimate_quantiles(x, 0.02)
    assert np.array_equal(code, (qh.quantile_indices(256, 0.02) + 1).astype(np.float32)) and np.all(code > 0)


# ---------------------------------------------------------------- create_fp8_map
@pytest.mark.parametrize("args", FP8_CASES, ids=lambda a: "s%d_e%d_p%d_b%d" % (int(a[0]), a[1], a[2], a[3]))
def test_create_fp8_map_equals_the_recorded_reference_map(args):
    recorded = np.load(os.path.join(ROOT, "tests", "golden", "fp8_maps_v1.npz"), allow_pickle=False)
    want = recorded["s%d_e%d_p%d_b%d" % (int(args[0]), args[1], args[2], args[3])]
    got = _F().create_fp8_map(*args)
    assert got.dtype == torch.float32 and got.shape == (256,)
    got = got.numpy()
    assert want.dtype == np.float32 and got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert np.all(np.diff(got) >= 0) and got.max() == 1.0


def test_create_fp8_map_checks_the_bit_budget():
    with pytest.raises(AssertionError):
        _F().create_fp8_map(True, 4, 4, 8)


# ---------------------------------------------------------------- refusals
def test_estimate_quantiles_refusals():
    F = _F()
    with pytest.raises(NotImplementedError, match="at least 256"):
        F.estimate_quantiles(torch.zeros(255))
    with pytest.raises(NotImplementedError, match="num_quantiles=257"):
        F.estimate_quantiles(torch.zeros(256), num_quantiles=257)
    for dtype in (torch.int32, torch.float64):
        with pytest.raises(NotImplementedError, match="data type"):
            F.estimate_quantiles(torch.zeros(256, dtype=dtype))
    with pytest.raises(TypeError, match="GPU"):                      # the refusal of every GPU op for a host tensor
        F.estimate_quantiles(torch.zeros(256))
    for bad in (torch.zeros(255), torch.zeros(256, dtype=torch.float16), torch.zeros(512)[::2]):
        with pytest.raises(ValueError, match="out must be"):
            F.estimate_quantiles(torch.zeros(256), out=bad)


def test_histogram_scatter_add_2d_refusals():
    F = _F()
    h, i, s = torch.zeros(4, 4), torch.zeros(3, dtype=torch.int32), torch.zeros(3)
    with pytest.raises(AssertionError):
        F.histogram_scatter_add_2d(torch.zeros(16), i, i, s)
    with pytest.raises(AssertionError):
        F.histogram_scatter_add_2d(h, i.long(), i, s)
    with pytest.raises(AssertionError):
        F.histogram_scatter_add_2d(h, i, i, s.double())
    with pytest.raises(AssertionError):
        F.histogram_scatter_add_2d(h, i, i[:2], s)
    with pytest.raises(TypeError, match="GPU"):
        F.histogram_scatter_add_2d(h, i, i, s)
