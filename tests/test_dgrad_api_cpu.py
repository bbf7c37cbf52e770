"""CPU-only checks of the 4-bit input-gradient interface: the eight cdequantize_blockwise{,_nested}_t_* symbols load
with their argument types, the shape rule of gemm_4bit_dgrad, and no CPU fallback.  No GPU compute is called."""
import ctypes as ct

import pytest
import torch

NAMES = [f"cdequantize_blockwise{nested}_t_{t}_{q}" for nested in ("", "_nested") for t in ("bf16", "fp16")
         for q in ("nf4", "fp4")]


def _F():
    import python_src_quants.functional as F
    return F


def test_transposing_dequantise_symbols_and_argtypes():
    import python_src_quants as bnb
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    assert len(NAMES) == 8
    for name in NAMES:
        fn = getattr(bnb.lib, name)
        assert fn.restype is ct.c_int
        if "_nested_" in name:
            # A, absmax_q, code2, absmax2, offset, out, blocksize, blocksize2, rows, cols, ldo
            assert fn.argtypes == [ct.c_void_p] * 6 + [ct.c_int] * 5
        else:
            # A, absmax, out, blocksize, rows, cols, ldo
            assert fn.argtypes == [ct.c_void_p] * 3 + [ct.c_int] * 4


def test_header_declares_the_transposing_dequantise():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "bnb_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in txt


def _state(N, K, dtype=torch.bfloat16, blocksize=64):
    F = _F()
    blocks = (N * K + blocksize - 1) // blocksize
    return F.QuantState(absmax=torch.ones(blocks), shape=torch.Size([N, K]), dtype=dtype, blocksize=blocksize,
                        quant_type="nf4", code=F.get_4bit_type("nf4", device="cpu"))


def test_dgrad_shape_rule_on_integers():
    F = _F()
    ok = F.gemm_4bit_dgrad_shape_ok
    assert ok(1, 64, 8) and ok(3, 64, 64) and ok(130, 192, 328) and ok(4096, 4096, 11008) and ok(16, 11008, 4096)
    assert not ok(5, 72, 64)              # N % 64: the contraction runs in k_hgemm's 64-wide k-tiles
    assert not ok(5, 64, 100)             # K % 8: the transposing dequantise's packed dwords
    assert not ok(0, 64, 64)              # no rows
    assert not ok(8, 32768, 65536)        # K * N = 2^31
    assert ok(8, 32768, 65536 - 8)
    assert not ok(2 ** 20, 4096, 4096)    # rows * K * 2 bytes beyond one launch's 32-bit offsets
    route = F.gemm_4bit_dgrad_static_route
    assert route(130, 192, 328, torch.bfloat16) == "hgemm" and route(130, 192, 328, torch.float16) == "hgemm"
    assert route(130, 192, 328, torch.float32) == "library"
    assert route(130, 72, 328, torch.bfloat16) == "library"
    # few rows against a weight with K >= 2 N stay on the library pair (measured), more rows and other weights do not
    assert route(16, 4096, 11008) == "library" and route(F.GEMM_4BIT_DGRAD_WIDE_MAX_ROWS, 4096, 11008) == "library"
    assert route(F.GEMM_4BIT_DGRAD_WIDE_MAX_ROWS + 1, 4096, 11008) == "hgemm"
    assert route(16, 11008, 4096) == "hgemm" and route(16, 4096, 4096) == "hgemm"
    assert F.GEMM_4BIT_DGRAD_MIN_ROWS >= 1
    assert route(F.GEMM_4BIT_DGRAD_MIN_ROWS - 1, 192, 328, torch.bfloat16) == "library"


def test_dgrad_supported_on_tensors():
    F = _F()
    st = _state(192, 328)
    assert F.gemm_4bit_dgrad_supported(torch.zeros(130, 192, dtype=torch.bfloat16), st)
    assert F.gemm_4bit_dgrad_supported(torch.zeros(2, 65, 192, dtype=torch.float16), st)
    assert not F.gemm_4bit_dgrad_supported(torch.zeros(130, 192, dtype=torch.float32), st)
    assert not F.gemm_4bit_dgrad_supported(torch.zeros(130, 328, dtype=torch.bfloat16), st)   # width is not N
    assert not F.gemm_4bit_dgrad_supported(torch.zeros(0, 192, dtype=torch.bfloat16), st)
    assert not F.gemm_4bit_dgrad_supported(torch.zeros(5, 72, dtype=torch.bfloat16), _state(72, 64))
    assert not F.gemm_4bit_dgrad_supported(torch.zeros(5, 64, dtype=torch.bfloat16), _state(64, 100))


def test_dgrad_ops_refuse_cpu_tensors():
    """No silent CPU fallback, as the other 4-bit ops (test_abi_and_host.py::test_gpu_ops_refuse_cpu_tensors)."""
    F = _F()
    st = _state(64, 64)
    q = torch.zeros(64 * 64 // 2, 1, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        F.dequantize_4bit_t(q, st)
    with pytest.raises(NotImplementedError):
        F.gemm_4bit_dgrad(torch.zeros(3, 64, dtype=torch.bfloat16), q, st)
