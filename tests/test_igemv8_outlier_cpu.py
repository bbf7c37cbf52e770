"""CPU-only checks of the threshold > 0 int8 decode interface (csrc/igemv8_outlier.hip): the C symbol (header, ctypes
types), the Python keywords, coverage decided before the device is touched, and the kernel's build-time resources
(hipcc cross-compiles for gfx950)."""
import ctypes as ct
import inspect
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitsandbytes-sycl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
DECL = ("int cint8_linear_rows_outlier_fp16(int m, int n, int k, const bnb_fp16* A, const int8_t* B, bnb_fp16* out, "
        "float* rowStats_out, int* outlier_cols_out, const float* colStats, const bnb_fp16* bias, float threshold, "
        "int lda, int ldb, int ldc);")


def _F():
    import python_src_quants.functional as F
    return F


def test_header_declares_the_entry():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "bnb_hip.h")).read())
    assert DECL in flat


def test_ctypes_types_and_python_keywords():
    import python_src_quants as bnb
    from python_src_quants.autograd._functions import MatmulLtState
    from python_src_quants.nn import Linear8bitLt
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    fn = bnb.lib.cint8_linear_rows_outlier_fp16
    assert fn.restype is ct.c_int
    assert fn.argtypes == [ct.c_int] * 3 + [ct.c_void_p] * 7 + [ct.c_float] + [ct.c_int] * 3
    sig = inspect.signature(bnb.functional.int8_linear_rows)
    assert sig.parameters["threshold"].default == 0.0
    assert inspect.signature(bnb.functional.int8_linear_rows_limit).parameters["threshold"].default == 0.0
    assert MatmulLtState().fused_outlier_decode is False
    assert inspect.signature(Linear8bitLt.__init__).parameters["fused_outlier_decode"].default is False
    assert Linear8bitLt(16, 16, fused_outlier_decode=True).state.fused_outlier_decode is True
    assert Linear8bitLt(16, 16).state.fused_outlier_decode is False


def test_coverage_is_decided_without_a_gpu():
    """2 for what the kernel does not take (the threshold and k <= 65536 included), 0 for an empty product; no error."""
    lib = _F().lib
    prev = lib.cigemv_set_mode(1)
    try:
        fn = lib.cint8_linear_rows_outlier_fp16
        assert fn(33, 64, 64, 16, 16, 16, None, None, 16, None, 6.0, 64, 64, 64) == 2        # rows
        assert fn(1, 64, 200, 16, 16, 16, None, None, 16, None, 6.0, 200, 200, 64) == 2      # k % 16
        assert fn(1, 64, 8, 16, 16, 16, None, None, 16, None, 6.0, 8, 8, 64) == 2
        assert fn(1, 8, 65552, 16, 16, 16, None, None, 16, None, 6.0, 65552, 65552, 8) == 2  # beyond the column mask
        assert fn(1, 64, 64, 8, 16, 16, None, None, 16, None, 6.0, 64, 64, 64) == 2          # A not 16-B aligned
        assert fn(1, 64, 64, 16, 16, 16, None, None, 16, None, 6.0, 48, 64, 64) == 2         # lda < k
        for thr in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(1, 64, 64, 16, 16, 16, None, None, 16, None, thr, 64, 64, 64) == 2
        assert fn(0, 64, 64, 16, 16, 16, None, None, 16, None, 6.0, 64, 64, 64) == 0         # nothing to do
        lib.cigemv_set_mode(-1)
        assert fn(0, 64, 64, 16, 16, 16, None, None, 16, None, 6.0, 64, 64, 64) == 2
        assert lib.cget_last_error() == 0
    finally:
        lib.cigemv_set_mode(prev)


def test_row_limit_with_a_threshold_follows_the_mode():
    F = _F()
    lib = F.lib
    prev = lib.cigemv_set_mode(0)
    try:
        assert F.int8_linear_rows_limit(4096, 4096, 6.0) == F.IGEMV_OUTLIER_ROWS_SMALL
        assert F.int8_linear_rows_limit(8192, 28672, 6.0) == F.IGEMV_OUTLIER_ROWS
        assert 1 <= F.IGEMV_OUTLIER_ROWS <= F.IGEMV_OUTLIER_ROWS_SMALL <= F.IGEMV_MAX_ROWS
        lib.cigemv_set_mode(1)
        assert F.int8_linear_rows_limit(8192, 28672, 6.0) == 32
        lib.cigemv_set_mode(-1)
        assert F.int8_linear_rows_limit(64, 64, 6.0) == 0
    finally:
        lib.cigemv_set_mode(prev)


def test_layer_route_predicate_with_a_threshold():
    """threshold > 0 reaches the one-launch step only when the state asks for it, under the other conditions."""
    from python_src_quants.autograd._functions import _decode_rows
    lib = _F().lib

    def state(**kw):
        d = dict(threshold=6.0, has_fp16_weights=False, CB=torch.zeros(48, 64, dtype=torch.int8),
                 fused_outlier_decode=True)
        d.update(kw)
        return types.SimpleNamespace(**d)

    A = torch.zeros(4, 64, dtype=torch.float16)
    prev = lib.cigemv_set_mode(1)
    try:
        assert _decode_rows(A, state(), None, False, True)
        assert _decode_rows(A, state(), torch.zeros(48, dtype=torch.float16), False, True)
        assert not _decode_rows(A, state(fused_outlier_decode=False), None, False, True)
        assert _decode_rows(A, state(threshold=0.0, fused_outlier_decode=False), None, False, True)
        assert not _decode_rows(A, state(threshold=-1.0), None, False, True)
        assert not _decode_rows(A, state(), None, True, True)                    # an input needs a gradient
        assert not _decode_rows(A, state(), torch.zeros(48, dtype=torch.float32), False, True)
        assert not _decode_rows(A, state(has_fp16_weights=True), None, False, True)
        assert not _decode_rows(torch.zeros(33, 64, dtype=torch.float16), state(), None, False, True)
        wide = state(CB=torch.zeros(1, 65552, dtype=torch.int8))
        assert not _decode_rows(torch.zeros(1, 65552, dtype=torch.float16), wide, None, False, True)
        lib.cigemv_set_mode(-1)
        assert not _decode_rows(A, state(), None, False, True)
    finally:
        lib.cigemv_set_mode(prev)


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    s = tmp_path_factory.mktemp("igemv8_outlier") / "k.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "igemv8_outlier.hip"), "-o", str(s),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_igemv8_outl" in k}


def test_outlier_kernel_resources(remarks):
    assert len(remarks) == 2, sorted(remarks)                # 1 and 2 activation fragments
    for name, r in remarks.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] <= 32 * 1024, (name, r)
        # an 8-wave workgroup is two waves per SIMD: one must fit, and the 1-fragment form keeps room for the second
        # one, as k_igemv8<1, true> does (it overlaps one workgroup's start and epilogue with another's stream)
        assert r["Occupancy [waves/SIMD]"] >= (4 if "Li1E" in name else 2), (name, r)
