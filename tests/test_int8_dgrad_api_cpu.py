"""CPU-only checks of the int8 input-gradient interface: the two cdequantize_int8_rows_t_* symbols load with their
argument types and are declared in the header, the shape rule and the static route of int8_linear_dgrad as a truth
table, and no CPU fallback.  No GPU compute is called."""
import ctypes as ct
import os

import pytest
import torch

NAMES = ["cdequantize_int8_rows_t_bf16", "cdequantize_int8_rows_t_fp16"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _F():
    import python_src_quants.functional as F
    return F


def test_int8_transposing_dequantise_symbols_and_argtypes():
    import python_src_quants as bnb
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    for name in NAMES:
        fn = getattr(bnb.lib, name)
        assert fn.restype is ct.c_int
        # CB, SCB, out, rows, cols, ldo
        assert fn.argtypes == [ct.c_void_p] * 3 + [ct.c_int] * 3


def test_header_and_loader_declare_the_int8_transposing_dequantise():
    header = open(os.path.join(ROOT, "include", "bnb_hip.h")).read()
    loader = open(os.path.join(ROOT, "bitsandbytes-sycl_amd", "python_src_quants", "cextension.py")).read()
    for name, t in zip(NAMES, ("bnb_bf16", "bnb_fp16")):
        assert (f"int {name}(const signed char* CB, const float* SCB, {t}* out, int rows, int cols, int ldo);"
                in header)
        assert f'"{name}"' in loader


def test_int8_dgrad_shape_rule_on_integers():
    F = _F()
    ok = F.int8_linear_dgrad_shape_ok
    assert ok(1, 64, 16) and ok(3, 64, 64) and ok(130, 192, 336) and ok(4096, 4096, 11008) and ok(16, 11008, 4096)
    assert not ok(5, 72, 64)              # N % 64: the contraction runs in k_hgemm's 64-wide k-tiles
    assert not ok(5, 64, 24)              # K % 16: the transposing dequantise's 16-B chunks of a weight row
    assert not ok(5, 64, 328)             # (K % 8 == 0 is not enough)
    assert not ok(0, 64, 64)              # no rows
    assert not ok(8, 32768, 65536)        # K * N = 2^31
    assert ok(8, 32768, 65536 - 16)
    assert not ok(2 ** 20, 4096, 4096)    # rows * K * 2 bytes beyond one launch's 32-bit offsets


@pytest.mark.parametrize("rows,N,K,dtype,route", [
    (130, 192, 336, torch.bfloat16, "hgemm"),
    (130, 192, 336, torch.float16, "hgemm"),
    (130, 192, 336, torch.float32, "library"),      # fp32 gradients keep the previous expression
    (130, 72, 336, torch.bfloat16, "library"),      # N % 64
    (130, 192, 328, torch.bfloat16, "library"),     # K % 16
    (0, 192, 336, torch.bfloat16, "library"),       # no rows
    # the probed Llama-2-7B weights: "hgemm" measured ahead at every row count, the wide product at few rows included
    (4096, 4096, 4096, torch.bfloat16, "hgemm"), (256, 4096, 4096, torch.bfloat16, "hgemm"),
    (16, 4096, 4096, torch.bfloat16, "hgemm"),
    (4096, 11008, 4096, torch.bfloat16, "hgemm"), (256, 11008, 4096, torch.bfloat16, "hgemm"),
    (16, 11008, 4096, torch.bfloat16, "hgemm"),
    (4096, 4096, 11008, torch.bfloat16, "hgemm"), (256, 4096, 11008, torch.bfloat16, "hgemm"),
    (16, 4096, 11008, torch.bfloat16, "hgemm"), (1, 4096, 11008, torch.float16, "hgemm"),
])
def test_int8_dgrad_static_route_truth_table(rows, N, K, dtype, route):
    F = _F()
    assert F.INT8_DGRAD_ROUTES == ("hgemm", "library")
    assert F.int8_linear_dgrad_static_route(rows, N, K, dtype) == route
    if dtype == torch.bfloat16:
        assert F.int8_linear_dgrad_static_route(rows, N, K) == route      # the default dtype


def test_int8_dgrad_supported_on_tensors():
    F = _F()
    CB = torch.zeros(192, 336, dtype=torch.int8)
    SCB = torch.ones(192)
    sup = F.int8_linear_dgrad_supported
    assert sup(torch.zeros(130, 192, dtype=torch.bfloat16), CB, SCB)
    assert sup(torch.zeros(2, 65, 192, dtype=torch.float16), CB, SCB)
    assert not sup(torch.zeros(130, 192, dtype=torch.float32), CB, SCB)
    assert not sup(torch.zeros(130, 336, dtype=torch.bfloat16), CB, SCB)          # width is not N
    assert not sup(torch.zeros(0, 192, dtype=torch.bfloat16), CB, SCB)
    assert not sup(torch.zeros(130, 192, dtype=torch.bfloat16), None, SCB)        # a CxB-only state
    assert not sup(torch.zeros(130, 192, dtype=torch.bfloat16), CB, None)
    assert not sup(torch.zeros(130, 192, dtype=torch.bfloat16), CB, SCB.double())
    assert not sup(torch.zeros(130, 192, dtype=torch.bfloat16), CB, torch.ones(191))
    assert not sup(torch.zeros(130, 192, dtype=torch.bfloat16), CB.to(torch.uint8), SCB)
    CBt = torch.zeros(336, 192, dtype=torch.int8).t()                              # not contiguous
    assert CBt.shape == (192, 336) and not sup(torch.zeros(130, 192, dtype=torch.bfloat16), CBt, SCB)
    assert not sup(torch.zeros(5, 72, dtype=torch.bfloat16), torch.zeros(72, 64, dtype=torch.int8), torch.ones(72))


def test_int8_dgrad_ops_refuse_cpu_tensors():
    """No silent CPU fallback, as the other ops (test_abi_and_host.py::test_gpu_ops_refuse_cpu_tensors)."""
    F = _F()
    CB = torch.zeros(64, 64, dtype=torch.int8)
    SCB = torch.ones(64)
    with pytest.raises(NotImplementedError):
        F.dequantize_int8_t(CB, SCB, torch.bfloat16)
    with pytest.raises(NotImplementedError):
        F.int8_linear_dgrad(torch.zeros(3, 64, dtype=torch.bfloat16), CB, SCB)
