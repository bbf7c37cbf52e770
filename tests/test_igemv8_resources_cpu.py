"""Build-time invariants of the int8 decode kernel (csrc/igemv8.hip), CPU-only (hipcc cross-compiles for gfx950): no
scratch and no spills in any instantiation, the plain forms keep two 8-wave workgroups per CU,
and the weight stream is non-temporal 16-B buffer loads while the activations are not."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitsandbytes-sycl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    s = tmp_path_factory.mktemp("igemv8") / "k.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "igemv8.hip"), "-o", str(s),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return s.read_text(), r.stderr


def _remarks(text):
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if "k_igemv8" in k}


def test_igemv8_resources(device_asm):
    kernels = _remarks(device_asm[1])
    assert len(kernels) == 4, sorted(kernels)            # {1, 2 activation fragments} x {int8, fused fp16 activations}
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] <= 18 * 1024, (name, r)
        fused = "Lb1E" in name
        # an 8-wave workgroup is two waves per SIMD: the plain forms must leave room for a second one
        assert r["Occupancy [waves/SIMD]"] >= (2 if fused else 4), (name, r)


def test_igemv8_memory_instructions(device_asm):
    bodies = re.findall(r"^(_ZN3bnb8k_igemv8\w+):[^\n]*\n(.*?)^\.Lfunc_end", device_asm[0], re.S | re.M)
    assert len(bodies) == 4
    for name, body in bodies:
        ins = [ln.split(";")[0].strip() for ln in body.splitlines()]
        wide = [i for i in ins if i.startswith("buffer_load_dwordx4")]
        streamed = [i for i in wide if i.endswith(" nt")]
        mt, fused = (2 if "Li2E" in name else 1), "Lb1E" in name
        # per 16-B weight load: one activation load per fragment, two when the activations are fp16
        assert streamed and len(wide) - len(streamed) == len(streamed) * mt * (2 if fused else 1), (name, len(wide))
        assert any(i.startswith("v_mfma_i32_16x16x64_i8") for i in ins), name
        assert not any(re.match(r"(global|buffer|flat)_atomic", i) for i in ins), name
