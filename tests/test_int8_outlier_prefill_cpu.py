"""CPU-only checks of the thresholded LLM.int8 prefill without a host round trip (csrc/int8_outlier_prefill.hip): the C
symbols (header, ctypes), the Python flags and the layer's routing predicate, coverage decided before the device is
touched, the numpy restatement against the oracle, and the kernels' build-time resources (hipcc cross-compiles for
gfx950)."""
import ctypes as ct
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from int8_outlier_prefill_helpers import prefill_reference, workspace_layout
from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitsandbytes-sycl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
DECLS = (
    "long long cint8_outlier_workspace_bytes(int k);",
    "int cint8_outlier_quant_fp16(int m, int k, const bnb_fp16* A, float threshold, char* CA, float* rowStats, "
    "void* ws, long long ws_bytes);",
    "int cint8_outlier_side_fp16(int m, int n, int k, const bnb_fp16* A, const int8_t* B, const float* colStats, "
    "bnb_fp16* out, int ldc, const void* ws);",
)


def _F():
    import python_src_quants.functional as F
    return F


def test_header_declares_the_entries():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "bnb_hip.h")).read())
    for decl in DECLS:
        assert decl in flat, decl


def test_ctypes_types_and_python_keywords():
    import python_src_quants as bnb
    from python_src_quants.autograd._functions import MatmulLtState
    from python_src_quants.nn import Linear8bitLt
    assert bnb.HIP_AVAILABLE, "libbitsandbytes_hip.so did not load"
    lib = bnb.lib
    assert lib.cint8_outlier_workspace_bytes.restype is ct.c_longlong
    assert lib.cint8_outlier_workspace_bytes.argtypes == [ct.c_int]
    assert lib.cint8_outlier_quant_fp16.restype is ct.c_int
    assert lib.cint8_outlier_quant_fp16.argtypes == ([ct.c_int] * 2 + [ct.c_void_p, ct.c_float] + [ct.c_void_p] * 3
                                                     + [ct.c_longlong])
    assert lib.cint8_outlier_side_fp16.restype is ct.c_int
    assert lib.cint8_outlier_side_fp16.argtypes == [ct.c_int] * 3 + [ct.c_void_p] * 4 + [ct.c_int, ct.c_void_p]
    sig = inspect.signature(bnb.functional.int8_linear_outliers)
    assert list(sig.parameters) == ["A", "CB", "SCB", "bias", "threshold", "out", "row_stats"]
    assert sig.parameters["threshold"].default == 6.0
    assert MatmulLtState().fused_outlier_prefill is False
    assert inspect.signature(Linear8bitLt.__init__).parameters["fused_outlier_prefill"].default is False
    assert Linear8bitLt(16, 16, fused_outlier_prefill=True).state.fused_outlier_prefill is True
    layer = Linear8bitLt(16, 16)
    assert layer.state.fused_outlier_prefill is False and layer.state.fused_outlier_decode is False


def test_workspace_bytes_and_supported_shapes():
    F = _F()
    for k in (8, 64, 1040, 4096, 65552):
        assert F.lib.cint8_outlier_workspace_bytes(k) == workspace_layout(k)[0]
    assert F.lib.cint8_outlier_workspace_bytes(0) == 0
    assert F.int8_linear_outliers_supported(33, 17, 64) and F.int8_linear_outliers_supported(1, 1, 8)
    assert F.int8_linear_outliers_supported(4096, 11008, 65552)
    assert not F.int8_linear_outliers_supported(5, 24, 12) and not F.int8_linear_outliers_supported(0, 24, 64)
    assert not F.int8_linear_outliers_supported(5, 0, 64) and not F.int8_linear_outliers_supported(5, 24, 4)


def test_coverage_is_decided_without_a_gpu():
    """2 for what the kernels do not take, 0 for an empty product; no error recorded.  (Pointers are never followed.)"""
    lib = _F().lib
    q, s = lib.cint8_outlier_quant_fp16, lib.cint8_outlier_side_fp16
    big = 1 << 20
    assert q(5, 12, 16, 6.0, 16, 16, 16, big) == 2                               # k % 8
    assert q(5, 64, 8, 6.0, 16, 16, 16, big) == 2                                # A not 16-B aligned
    assert q(5, 64, 16, 6.0, 16, 16, None, big) == 2                             # no workspace
    assert q(5, 64, 16, 6.0, 16, 16, 16, workspace_layout(64)[0] - 1) == 2       # workspace too small
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert q(5, 64, 16, thr, 16, 16, 16, big) == 2
    assert q(0, 64, 16, 6.0, 16, 16, 16, big) == 0                               # nothing to do
    assert s(5, 24, 12, 16, 16, 16, 16, 24, 16) == 2
    assert s(5, 24, 64, 8, 16, 16, 16, 24, 16) == 2
    assert s(5, 24, 64, 16, 16, 16, 16, 24, None) == 2
    assert s(5, 24, 64, 16, 16, 16, 16, 16, 16) == 2                             # ldc < n
    assert s(5, 0, 64, 16, 16, 16, 16, 24, 16) == 0
    assert lib.cget_last_error() == 0


def test_bad_threshold_raises():
    F = _F()
    A = torch.zeros(4, 64, dtype=torch.float16)
    CB = torch.zeros(8, 64, dtype=torch.int8)
    SCB = torch.ones(8)
    for thr in (0.0, -6.0, float("nan")):
        with pytest.raises(ValueError):
            F.int8_linear_outliers(A, CB, SCB, threshold=thr)


def test_layer_route_predicate():
    """The new path is taken only when the state asks for it, under every other condition, and after the decode step."""
    from python_src_quants.autograd._functions import _decode_rows, _prefill_outliers
    lib = _F().lib

    def state(**kw):
        d = dict(threshold=6.0, has_fp16_weights=False, CB=torch.zeros(48, 64, dtype=torch.int8),
                 fused_outlier_decode=False, fused_outlier_prefill=True)
        d.update(kw)
        return types.SimpleNamespace(**d)

    A = torch.zeros(40, 64, dtype=torch.float16)
    assert _prefill_outliers(A, state(), None, False, True)
    assert _prefill_outliers(A, state(), torch.zeros(48, dtype=torch.float16), False, True)
    assert _prefill_outliers(torch.zeros(1, 64, dtype=torch.float16), state(), None, False, True)   # any row count
    assert not _prefill_outliers(A, state(fused_outlier_prefill=False), None, False, True)
    assert not _prefill_outliers(A, types.SimpleNamespace(threshold=6.0, has_fp16_weights=False, CB=state().CB),
                                 None, False, True)                              # a state without the field
    assert not _prefill_outliers(A, state(threshold=0.0), None, False, True)
    assert not _prefill_outliers(A, state(threshold=-1.0), None, False, True)
    assert not _prefill_outliers(A, state(threshold=float("nan")), None, False, True)
    assert not _prefill_outliers(A, state(), None, True, True)                   # an input needs a gradient
    assert not _prefill_outliers(A, state(), None, False, False)                 # no int8 GEMM
    assert not _prefill_outliers(A, state(), torch.zeros(48, dtype=torch.float32), False, True)
    assert not _prefill_outliers(A, state(has_fp16_weights=True), None, False, True)
    assert not _prefill_outliers(A, state(CB=None), None, False, True)
    odd = state(CB=torch.zeros(48, 12, dtype=torch.int8))
    assert not _prefill_outliers(torch.zeros(40, 12, dtype=torch.float16), odd, None, False, True)
    # precedence: with both flags three rows are the decode step's, which the forward asks first; 40 rows are not
    A3 = torch.zeros(3, 64, dtype=torch.float16)
    prev = lib.cigemv_set_mode(1)
    try:
        assert _decode_rows(A3, state(fused_outlier_decode=True), None, False, True)
        assert not _decode_rows(A3, state(), None, False, True)
        assert not _decode_rows(A, state(fused_outlier_decode=True), None, False, True)
    finally:
        lib.cigemv_set_mode(prev)


def test_helper_against_the_oracle():
    """On one planted shape the restatement's S, CA and first16 are what ref.colrow_absmax / ref.double_quant /
    ref.mm_dequant give."""
    rng = np.random.default_rng(4)
    rows, n, k, thr = 9, 20, 96, 6.0
    A = np.clip(rng.standard_normal((rows, k)), -5, 5).astype(np.float16)
    A[0, 0], A[8, 95], A[2, 18], A[3, 21], A[4, 33] = 40.0, -9.0, 17.0, -8.0, thr
    A[5, 34] = np.nextafter(np.float16(thr), np.float16(0))
    A[1] = 0
    B = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
    cs = rng.uniform(0.5, 2, n).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float16)
    for b in (None, bias):
        r = prefill_reference(A, B, cs, b, thr)
        assert list(r["S"]) == [0, 18, 21, 33, 95]
        rs, _, nnz = ref.colrow_absmax(A, thr)
        assert np.array_equal(r["row_stats"].view(np.uint32), rs.view(np.uint32)) and int(nnz.sum()) == 5
        with np.errstate(invalid="ignore", divide="ignore"):
            q, _ = ref.double_quant(A, rs, np.ones(k, dtype=np.float32), thr)
        cols = np.zeros(k, dtype=bool)
        cols[r["S"]] = True
        assert np.array_equal(r["CA"], np.where(cols[None, :], np.int8(0), q))
        assert not np.array_equal(r["CA"], q)                # whole columns, not only the entries
        assert not r["CA"][1].any() and rs[1] == 0.0         # the zero row
        first = ref.mm_dequant(ref.igemmlt(r["CA"], B), rs, cs, b)
        assert np.array_equal(r["first16"].view(np.uint16), first.view(np.uint16))
        side = (A[:, r["S"]].astype(np.float64) @ B[:, r["S"]].astype(np.float64).T) * (cs.astype(np.float64) / 127)
        assert np.array_equal(r["exact"], first.astype(np.float64) + side)
        assert np.all(r["tol"] > 0) and np.all(r["tol"] < r["unfused_tol"])


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    s = tmp_path_factory.mktemp("int8_outlier_prefill") / "k.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "int8_outlier_prefill.hip"), "-o", str(s),
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
    return out


def test_kernel_resources(remarks):
    names = sorted(remarks)
    assert len(names) == 4, names                            # scan, quantise + list, the side product x {16-B, scalar}
    assert sum("k_outl_scan" in x for x in names) == 1 and sum("k_outl_quant" in x for x in names) == 1
    assert sum("k_outlier_side" in x for x in names) == 2
    for name, r in remarks.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] <= 20 * 1024, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 4, (name, r)   # a 256-thread workgroup is one wave per SIMD
