"""Build-time invariant of the K-strided int8 GEMM (csrc/igemm_strided.hip): its four kernels compile for gfx950
under the library's flags without VGPR spills (64 accumulators, 32 staging and 32 fragment registers per lane at two
waves per SIMD leave no room for scratch traffic in the main loop).  CPU-only: hipcc cross-compiles here; only the
compiler's resource-usage remarks are read."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitsandbytes-sycl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_igemm_strided_compiles_spill_free(tmp_path):
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-Wall",
                        "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "igemm_strided.hip"), "-o",
                        str(tmp_path / "k.s"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, scratch = {}, {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name and "k_igemm_strided" in name:
            kernels[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "k_igemm_strided" in name:
            scratch[name] = int(m.group(1))
    # one instance per (X, Y) in {K-contiguous, K-strided}^2
    assert len(kernels) == 4 and len(scratch) == 4, (kernels, scratch)
    assert all(n == 0 for n in kernels.values()), kernels
    # and no stack either: the unaligned loads' funnel shift must stay in registers, not be indexed through scratch
    assert all(n == 0 for n in scratch.values()), scratch
