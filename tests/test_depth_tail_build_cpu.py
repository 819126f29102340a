"""CPU: both depth_tail_kernel instantiations of the shipped library keep the two held source-row lerps, the window chunks and the 36 weight fragments
in registers.  Reads the gfx950 code object's kernel metadata only (in the manner of tests/test_capi_symbols.py::test_igemm_kernels_use_no_scratch)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_depth_tail_kernels_use_no_scratch(tmp_path):
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(objdump) or not os.path.exists(readelf) or not os.path.exists(so):
        pytest.skip("llvm tools or the built library are not present")
    local = str(tmp_path / "lib.so")
    shutil.copy(so, local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    bundles = [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]
    assert bundles
    seen = {}
    for b in bundles:
        notes = subprocess.run([readelf, "--notes", str(tmp_path / b)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            vgpr = re.search(r"\.vgpr_count:\s+(\d+)", blk)
            if name and scratch and vgpr and "depth_tail_kernel" in name.group(1):
                seen[name.group(1)] = (int(scratch.group(1)), int(vgpr.group(1)))
    assert len(seen) == 2, f"expected the bf16 and the fp16 instantiation of depth_tail_kernel, found {sorted(seen)}"
    for name, (scratch, vgpr) in seen.items():
        assert scratch == 0, f"{name} uses {scratch} bytes of scratch per lane"
        assert vgpr <= 256, f"{name} needs {vgpr} VGPRs: 512 threads per workgroup leave 256"
