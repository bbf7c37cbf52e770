"""bench.py --dump-outputs (dump_outputs): the sampled rows of the step's output land in DIR/y.npy as float32, exactly
(bf16 -> float32 is exact), the same rows on every call, under 64 MB at the metric shape."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_dump_outputs_sample_is_exact_and_fixed(tmp_path):
    m, n = bench.DUMP_ROWS + 37, 24                 # more rows than the sample holds
    y = torch.randn(m, n, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "a"), y)
    bench.dump_outputs(str(tmp_path / "b"), y)
    a, b = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_ROWS, n)
    assert np.array_equal(a, b)
    # every dumped row is a row of y, bit for bit, in ascending row order
    full = y.float().numpy()
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(11))[:bench.DUMP_ROWS].sort().values.numpy()
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, full[rows])
    assert bench.DUMP_ROWS * bench.N * 4 <= 64_000_000


def test_dump_outputs_small_output_is_whole(tmp_path):
    y = torch.arange(12, dtype=torch.float32).reshape(4, 3).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path), y)
    assert np.array_equal(np.load(tmp_path / "y.npy"), y.float().numpy())
