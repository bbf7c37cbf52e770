"""Build-time invariants of the transposing int8 row dequantise (csrc/dequant_int8_t.hip), CPU-only (hipcc
cross-compiles for gfx950): both instantiations compile without spills at 8 waves per SIMD within the LDS DESIGN.md
section 4d states (the 16 KiB tile, nothing else).  Read from the compiler's resource remarks alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitsandbytes-sycl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    s = tmp_path_factory.mktemp("dequant_int8_t") / "k.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "dequant_int8_t.hip"), "-o", str(s),
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
    return {k: v for k, v in out.items() if "k_dequantize_int8_t" in k}


def test_dequant_int8_t_resources(remarks):
    assert len(remarks) == 2, sorted(remarks)          # bf16, fp16
    for name, r in remarks.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] == 8, (name, r)
        assert r["VGPRs"] <= 64, (name, r)
        assert r["LDS Size [bytes/block]"] == 16384, (name, r)


def test_design_states_the_lds_size():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = txt[txt.index("### 4d."):]
    assert "16384" in section or "16 KiB" in section
