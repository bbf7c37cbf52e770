"""Build-time invariants of the transposing 4-bit dequantise (csrc/dequant_t.hip), CPU-only (hipcc cross-compiles for
gfx950): every instantiation compiles without spills at 8 waves per SIMD within the LDS DESIGN.md section 4b states, the
tile goes to LDS in 32-bit writes and leaves it in 16-B reads, and the output is stored 16 B wide write-through."""
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
    s = tmp_path_factory.mktemp("dequant_t") / "k.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-ffp-contract=off", "-I", CSRC, os.path.join(CSRC, "dequant_t.hip"), "-o", str(s),
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
    return {k: v for k, v in out.items() if "k_dequantize_4bit_t" in k}


def test_dequant_t_resources(device_asm):
    kernels = _remarks(device_asm[1])
    assert len(kernels) == 8, sorted(kernels)          # {bf16, fp16} x {nf4, fp4} x {plain, nested}
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] == 8, (name, r)
        assert r["VGPRs"] <= 64, (name, r)
        # 16 KiB tile + 2 KiB pair table (+ 1 KiB second-level code when nested)
        assert r["LDS Size [bytes/block]"] in (18432, 19456), (name, r)


def test_dequant_t_memory_instructions(device_asm):
    bodies = re.findall(r"^(_ZN3bnb19k_dequantize_4bit_t\w+):[^\n]*\n(.*?)^\.Lfunc_end", device_asm[0], re.S | re.M)
    assert len(bodies) == 8
    for name, body in bodies:
        ins = [ln.split(";")[0].strip() for ln in body.splitlines()]
        stores = [i for i in ins if re.match(r"(global|buffer|flat)_store", i)]
        assert len(stores) == 4 and all(re.match(r"buffer_store_dwordx4 .* sc1$", i) for i in stores), (name, stores)
        lds_writes = [i.split()[0] for i in ins if i.startswith("ds_write")]
        tile_writes = sum({"ds_write_b32": 1, "ds_write2_b32": 2}.get(w, 0) for w in lds_writes)
        # 16 packed 32-bit tile writes per lane (+ one for the second-level code table when nested); nothing narrower
        assert tile_writes in (16, 17) and not any("b16" in w or "b8" in w for w in lds_writes), (name, lds_writes)
        assert sum(i.startswith("ds_read_b128") for i in ins) == 4, name
        assert sum(bool(re.match(r"global_load_dword .* nt$", i)) for i in ins) == 4, name
