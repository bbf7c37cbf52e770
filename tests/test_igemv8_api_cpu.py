"""CPU-only checks of the int8 decode interface: the four C symbols (header, library, return and argument types), the
shape-only coverage predicate, the mode knob and the layer's route predicate.  No GPU compute is called."""
import ctypes as ct
import os
import re
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("int m, int n, int k, const {a}* A, const int8_t* B, bnb_fp16* out, {rs} const float* colStats, "
        "const bnb_fp16* bias, int lda, int ldb, int ldc);")


def _F():
    import python_src_quants.functional as F
    return F


def test_header_declares_the_four_symbols():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "bnb_hip.h")).read())
    assert "int cigemv_row_dequant_fp16(" + ARGS.format(a="int8_t", rs="const float* rowStats,") in flat
    assert "int cint8_linear_rows_fp16(" + ARGS.format(a="bnb_fp16", rs="float* rowStats_out,") in flat
    assert "int cigemv_set_mode(int mode);" in flat
    assert "int cigemv_max_rows(void);" in flat


def test_library_exports_them_with_their_types():
    import python_src_quants as bnb
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    for name in ("cigemv_row_dequant_fp16", "cint8_linear_rows_fp16"):
        fn = getattr(bnb.lib, name)
        assert fn.restype is ct.c_int
        assert fn.argtypes == [ct.c_int] * 3 + [ct.c_void_p] * 6 + [ct.c_int] * 3
    assert bnb.lib.cigemv_set_mode.restype is ct.c_int and bnb.lib.cigemv_set_mode.argtypes == [ct.c_int]
    assert bnb.lib.cigemv_max_rows.restype is ct.c_int and bnb.lib.cigemv_max_rows.argtypes == []
    for name in ("igemv_dequant", "int8_linear_rows", "igemv_supported"):
        assert callable(getattr(bnb.functional, name))


def test_igemv_supported_from_shapes_alone():
    ok = _F().igemv_supported
    assert ok(1, 1, 16) and ok(32, 17, 64) and ok(3, 100, 1040) and ok(1, 11008, 4096) and ok(32, 8192, 28672)
    assert not ok(0, 64, 64) and not ok(33, 64, 64) and not ok(-1, 64, 64)      # rows outside 1..32
    assert not ok(1, 64, 200) and not ok(1, 64, 8) and not ok(1, 64, 0)         # rows of B not 16-B aligned / empty
    assert not ok(1, 0, 64)
    assert not ok(1, 64, 2 ** 27) and ok(1, 64, 2 ** 27 - 16)                   # a 16-row group within 2^31 bytes
    assert _F().IGEMV_MAX_ROWS == 32


def test_set_mode_returns_the_previous_value_and_moves_the_row_limit():
    lib = _F().lib
    first = lib.cigemv_set_mode(1)
    try:
        assert first == 0                                     # auto is the default
        assert lib.cigemv_max_rows() == 32
        assert lib.cigemv_set_mode(-1) == 1
        assert lib.cigemv_max_rows() == 0
        assert lib.cigemv_set_mode(0) == -1
        assert lib.cigemv_max_rows() == 8                     # the measured all-shapes limit of the automatic route
        assert lib.cigemv_set_mode(7) == 0 and lib.cigemv_set_mode(-9) == 1     # any sign counts
        assert lib.cigemv_set_mode(0) == -1
    finally:
        lib.cigemv_set_mode(first)


def test_fused_forward_row_limit_follows_mode_and_weight_size():
    F = _F()
    lib = F.lib
    prev = lib.cigemv_set_mode(0)
    try:
        assert F.int8_linear_rows_limit(4096, 4096) == F.IGEMV_FUSED_ROWS_SMALL == 8
        assert F.int8_linear_rows_limit(11008, 4096) == 8 and F.int8_linear_rows_limit(4096, 11008) == 8
        assert F.int8_linear_rows_limit(11008, 4112) == F.IGEMV_FUSED_ROWS == 4
        assert F.int8_linear_rows_limit(8192, 28672) == 4
        lib.cigemv_set_mode(1)
        assert F.int8_linear_rows_limit(8192, 28672) == 32 and F.int8_linear_rows_limit(64, 64) == 32
        lib.cigemv_set_mode(-1)
        assert F.int8_linear_rows_limit(64, 64) == 0
    finally:
        lib.cigemv_set_mode(prev)


def test_not_covered_calls_launch_nothing_without_a_gpu():
    """The entries decide coverage before they touch the device: 2 for what the kernel does not take, 0 for an empty
    product, and no error is recorded."""
    lib = _F().lib
    prev = lib.cigemv_set_mode(1)
    try:
        for fn in (lib.cigemv_row_dequant_fp16, lib.cint8_linear_rows_fp16):
            assert fn(33, 64, 64, 16, 16, 16, None, 16, None, 64, 64, 64) == 2       # rows
            assert fn(1, 64, 200, 16, 16, 16, None, 16, None, 200, 200, 64) == 2     # k % 16
            assert fn(1, 64, 8, 16, 16, 16, None, 16, None, 8, 8, 64) == 2
            assert fn(1, 64, 64, 8, 16, 16, None, 16, None, 64, 64, 64) == 2         # A not 16-B aligned
            assert fn(1, 64, 64, 16, 16, 16, None, 16, None, 48, 64, 64) == 2        # lda < k
            assert fn(1, 64, 64, 16, 16, 16, None, 16, None, 64, 64, 63) == 2        # ldc < n
            assert fn(0, 64, 64, 16, 16, 16, None, 16, None, 64, 64, 64) == 0        # nothing to do
        lib.cigemv_set_mode(-1)
        assert lib.cigemv_row_dequant_fp16(1, 64, 64, 16, 16, 16, None, 16, None, 64, 64, 64) == 2
        assert lib.cget_last_error() == 0
    finally:
        lib.cigemv_set_mode(prev)


def test_layer_route_predicate():
    """MatMul8bitLt takes the one-launch step only for inference without outliers on a stored int8 weight, with a bias
    the epilogue can fuse and a row count within the current limit."""
    from python_src_quants.autograd._functions import _decode_rows
    lib = _F().lib

    def state(**kw):
        d = dict(threshold=0.0, has_fp16_weights=False, CB=torch.zeros(48, 64, dtype=torch.int8))
        d.update(kw)
        return types.SimpleNamespace(**d)

    A = torch.zeros(4, 64, dtype=torch.float16)
    prev = lib.cigemv_set_mode(1)
    try:
        assert _decode_rows(A, state(), None, False, True)
        assert _decode_rows(A, state(), torch.zeros(48, dtype=torch.float16), False, True)
        assert not _decode_rows(A, state(), torch.zeros(48, dtype=torch.float32), False, True)
        assert not _decode_rows(A, state(), None, True, True)                    # an input needs a gradient
        assert not _decode_rows(A, state(), None, False, False)                  # no int8 GEMM wanted
        assert not _decode_rows(A, state(threshold=6.0), None, False, True)      # outliers
        assert not _decode_rows(A, state(CB=None), None, False, True)            # only the tiled CxB
        assert not _decode_rows(A, state(has_fp16_weights=True), None, False, True)
        assert not _decode_rows(torch.zeros(33, 64, dtype=torch.float16), state(), None, False, True)
        assert not _decode_rows(torch.zeros(4, 72, dtype=torch.float16),
                                state(CB=torch.zeros(48, 72, dtype=torch.int8)), None, False, True)
        lib.cigemv_set_mode(-1)
        assert not _decode_rows(A, state(), None, False, True)
        lib.cigemv_set_mode(0)                                                   # auto: the measured row limits
        assert _decode_rows(torch.zeros(8, 64, dtype=torch.float16), state(), None, False, True)
        assert not _decode_rows(torch.zeros(9, 64, dtype=torch.float16), state(), None, False, True)
    finally:
        lib.cigemv_set_mode(prev)
