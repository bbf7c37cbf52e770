"""GPU: estimate_quantiles (the 4096-key workgroup sort of csrc/quantiles.hip), create_quantile_map and
histogram_scatter_add_2d.

The estimate is defined bit for bit (totalOrder inside a block, fp32 index expression, slot-ordered
fp64 sum rounded once), so every comparison with the numpy restatement in tests/quantile_helpers.py is an equality of
bit patterns.  `out` is pre-filled with NaN in every case: the call overwrites it, it does not accumulate.
"""
import numpy as np
import pytest
import torch

import quantile_helpers as qh
from helpers import to_torch
from oracle import ref

pytestmark = pytest.mark.gpu

BLOCK, SLOTS = qh.BLOCK, qh.SLOTS
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
POS_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _F():
    import python_src_quants.functional as F
    return F


def _estimate(tA, offset, **kw):
    out = torch.full((256,), float("nan"), device=tA.device)
    got = _F().estimate_quantiles(tA, out=out, offset=offset, **kw)
    return got.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(got, want, what=""):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first t={bad[:4]} got {got[bad[:4]]} want {want[bad[:4]]}"


_NORMAL = {}


def _normal(n):
    """The first n of one seeded fp32 normal sample (generated once)."""
    if "x" not in _NORMAL:
        _NORMAL["x"] = np.random.default_rng(5).standard_normal(3 * BLOCK + 5).astype(np.float32)
    return _NORMAL["x"][:n]


@pytest.mark.parametrize("n", [256, 257, 1000, 4095, 4096, 4097, 8191, 8192, 3 * 4096 + 5])
def test_sizes_fp32(dev, n):
    x = _normal(n)
    tA = to_torch(x, "fp32", dev)
    for offset in (1 / 512, 0.02, 0.0):            # one upload per size
        _check(_estimate(tA, offset), qh.estimate_quantiles(x, offset), f"n={n} offset={offset}")


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("kind", ["fp32", "fp16"])
def test_position_probe(dev, kind, blocks):
    """Block b is a permutation of 4096 b + (0..4095): entry t is idx[t] + 4096 (blocks - 1) / 2 exactly.  fp16 holds
    (perm - 2048) / 2 with one block's range per block (exact in fp16), so the expectation shifts and halves."""
    rng = np.random.default_rng(10 + blocks)
    idx = qh.quantile_indices(BLOCK, 1 / 512).astype(np.float64)
    if kind == "fp32":
        vals = np.concatenate([rng.permutation(BLOCK) + BLOCK * b for b in range(blocks)]).astype(np.float64)
        want = (idx + BLOCK * (blocks - 1) / 2).astype(np.float32)
    else:
        vals = np.concatenate([(rng.permutation(BLOCK) - 2048) / 2 for b in range(blocks)])
        want = ((idx - 2048) / 2).astype(np.float32)
    x = vals.astype(np.float32 if kind == "fp32" else np.float16)
    assert np.array_equal(x.astype(np.float64), vals)                # the storage type holds the probe exactly
    got = _estimate(to_torch(x, kind, dev), 1 / 512)
    _check(got, want, f"{kind} blocks={blocks}")
    _check(got, qh.estimate_quantiles(ref.as_f32(x, kind), 1 / 512), "restatement")


def test_bf16(dev):
    n = 2 * BLOCK
    x = ref.cast_out(np.random.default_rng(6).standard_normal(n).astype(np.float32), "bf16")
    _check(_estimate(to_torch(x, "bf16", dev), 1 / 512), qh.estimate_quantiles(ref.as_f32(x, "bf16"), 1 / 512))


def test_fp16_random_and_unaligned(dev):
    n = 2 * BLOCK + 3
    x = np.random.default_rng(7).standard_normal(n + 1).astype(np.float16)
    t = to_torch(x, "fp16", dev)
    _check(_estimate(t[:n], 0.02), qh.estimate_quantiles(ref.as_f32(x[:n], "fp16"), 0.02), "aligned")
    assert t[1:].data_ptr() % 16 == 2
    _check(_estimate(t[1:], 0.02), qh.estimate_quantiles(ref.as_f32(x[1:], "fp16"), 0.02), "unaligned")


def test_slot_wrap(dev):
    """More blocks than slots: slots 0..2 take three blocks, the rest two, and the finish sees all 1024 slots."""
    blocks = 2 * SLOTS + 3
    g = torch.Generator(device=dev).manual_seed(8)
    tA = torch.randn(blocks * BLOCK, device=dev, generator=g)
    got = _estimate(tA, 1 / 512)
    _check(got, qh.estimate_quantiles(tA.cpu().numpy(), 1 / 512))


def test_order_of_special_values(dev):
    """One block of 256 at offset 0 (idx[t] = t: every sorted position is an entry): -NaN, -inf, ..., -0.0, +0.0, ...,
    +inf, +NaN."""
    x = np.random.default_rng(9).standard_normal(256).astype(np.float32)
    x[[3, 50, 77, 101, 200, 255]] = [POS_NAN, -0.0, np.inf, NEG_NAN, 0.0, -np.inf]
    got = _estimate(to_torch(x, "fp32", dev), 0.0)
    want = qh.estimate_quantiles(x, 0.0)
    neg = int(np.sum(x < 0))
    assert _bits(want)[0] == _bits(NEG_NAN) and want[1] == -np.inf and want[254] == np.inf
    assert _bits(want)[255] == _bits(POS_NAN)
    # -0.0 sorts before +0.0; both entries are +0.0, the sum starts there
    assert want[neg] < 0 < want[neg + 3] and np.all(_bits(want)[neg + 1:neg + 3] == 0)
    _check(got[1:255], want[1:255], "finite and infinite entries")
    _check(got, want, "NaN entries")


@pytest.mark.parametrize("kind", ["fp32", "fp16", "bf16"])
def test_poisoned_arena_short_block(dev, kind):
    """n = 1000 inside a larger buffer at an odd element offset: what lies around A would sort first if read."""
    n, lead = 1000, 3
    clean = ref.cast_out(np.random.default_rng(11).standard_normal(n).astype(np.float32), kind)
    neg_inf, neg_nan, bits = {"fp32": (0xFF800000, 0xFFC00000, np.uint32), "fp16": (0xFC00, 0xFE00, np.uint16),
                              "bf16": (0xFF80, 0xFFC0, np.uint16)}[kind]
    poison = np.full(2 * BLOCK, neg_inf, bits)
    poison[1::2] = neg_nan
    arena = to_torch(poison if kind == "bf16" else poison.view({"fp32": np.float32, "fp16": np.float16}[kind]), kind, dev)
    arena[lead:lead + n] = to_torch(clean, kind, dev)
    A = arena[lead:lead + n]
    assert A.data_ptr() % 16 != 0 and bool(torch.isinf(arena[lead - 1])) and bool(torch.isnan(arena[lead + n]))
    _check(_estimate(A, 1 / 512), qh.estimate_quantiles(ref.as_f32(clean, kind), 1 / 512), kind)


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "unaligned"])
def test_poisoned_arena_ignored_tail(dev, lead):
    """n = 4096 + 5: one full block; the five trailing elements and the arena beyond hold 1e30."""
    n = BLOCK + 5
    clean = _normal(BLOCK)
    arena = torch.full((3 * BLOCK,), 1e30, device=dev)
    arena[lead:lead + BLOCK] = to_torch(clean, "fp32", dev)
    A = arena[lead:lead + n]
    assert A.data_ptr() % 16 == 4 * lead
    _check(_estimate(A, 1 / 512), qh.estimate_quantiles(clean, 1 / 512))


def test_run_to_run_and_side_stream(dev):
    tA = to_torch(_normal(3 * BLOCK + 5), "fp32", dev)
    first = _estimate(tA, 1 / 512)
    _check(_estimate(tA, 1 / 512), first, "second call")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                  # another stream takes its own workspace: the same bits
        out = torch.full((256,), float("nan"), device=dev)
        _F().estimate_quantiles(tA, out=out)
    side.synchronize()
    _check(out.cpu().numpy(), first, "side stream")


def test_default_out_and_non_contiguous_input(dev):
    x = _normal(2 * BLOCK).reshape(2, BLOCK)
    got = _F().estimate_quantiles(to_torch(x, "fp32", dev).t())      # a transposed view is made contiguous
    assert got.dtype == torch.float32 and got.shape == (256,)
    _check(got.cpu().numpy(), qh.estimate_quantiles(np.ascontiguousarray(x.T), 1 / 512))


@pytest.mark.parametrize("num_quantiles", [255, 15])
def test_num_quantiles_subsampling(dev, num_quantiles):
    x = _normal(2 * BLOCK)
    tA = to_torch(x, "fp32", dev)
    got = _estimate(tA, 1 / 512, num_quantiles=num_quantiles)       # the default offset follows num_quantiles
    assert got.shape == (num_quantiles,)
    _check(got, qh.subsample(qh.estimate_quantiles(x, qh.default_offset(num_quantiles)), num_quantiles))
    # an explicit offset is kept
    got = _estimate(tA, 0.02, num_quantiles=num_quantiles)
    _check(got, qh.subsample(qh.estimate_quantiles(x, 0.02), num_quantiles))


def test_create_quantile_map_feeds_the_blockwise_codec(dev):
    F = _F()
    x = _normal(2 * BLOCK)
    qmap = F.create_quantile_map(to_torch(x, "fp32", dev))
    assert qmap.dtype == torch.float32 and qmap.shape == (256,)
    m = qmap.numpy()
    assert np.all(np.diff(m) >= 0) and np.abs(m).max() == 1.0 and np.any(m == 0)
    q255 = qh.subsample(qh.estimate_quantiles(x, 1 / 510), 255)
    want = np.sort(np.concatenate([q255, np.zeros(1, np.float32)]))
    _check(m, want / np.abs(want).max(), "map")
    y = x[:BLOCK]
    got, state = F.quantize_blockwise(to_torch(y, "fp32", dev), code=qmap.to(dev), blocksize=256)
    absmax, codes = ref.quantize_blockwise(y, 256, "8bit", code=m)
    assert np.array_equal(state.absmax.cpu().numpy(), absmax)
    assert np.array_equal(got.cpu().numpy().reshape(-1), codes)


# ---------------------------------------------------------------- histogram
def _hist_case(dev, i1, i2, src, calls=1):
    F = _F()
    want = np.full((256, 256), 3.0, np.float32)
    hist = torch.full((256, 256), 3.0, device=dev)
    args = [torch.from_numpy(a).to(dev) for a in (i1, i2, src)]
    for _ in range(calls):
        F.histogram_scatter_add_2d(hist, *args)
        np.add.at(want, (i1, i2), src)
    assert np.array_equal(hist.cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 513, 100000])
def test_histogram_random_bins(dev, n):
    rng = np.random.default_rng(n)
    i1, i2 = (rng.integers(0, 256, n).astype(np.int32) for _ in range(2))
    _hist_case(dev, i1, i2, rng.integers(-4, 5, n).astype(np.float32))


def test_histogram_one_bin_contention(dev):
    n = 100000
    _hist_case(dev, np.full(n, 7, np.int32), np.full(n, 201, np.int32), np.ones(n, np.float32))


def test_histogram_two_calls_accumulate_and_empty_call(dev):
    rng = np.random.default_rng(3)
    i1, i2 = (rng.integers(0, 256, 513).astype(np.int32) for _ in range(2))
    _hist_case(dev, i1, i2, rng.integers(-4, 5, 513).astype(np.float32), calls=2)
    empty = np.zeros(0, np.int32)
    _hist_case(dev, empty, empty, np.zeros(0, np.float32))
