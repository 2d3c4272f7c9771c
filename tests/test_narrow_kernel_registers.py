"""
The narrow audio first pass (rips_cloud_kernel<512, 1, u32, false, true>) runs three 512-thread workgroups per CU, six
waves per SIMD: that residency holds only while the kernel stays within 80 VGPRs, and its speed only while nothing spills
(csrc/rips.hip, the comment above rips_cloud_kernel).  Read off the metadata of the built code object, as the AGPR check
in tests/test_capi_and_host.py does: no GPU needed.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narrow_audio_kernel_80_vgprs_no_scratch_no_agprs(tmp_path):
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    lib = os.path.join(ROOT, "tda_eeg_audio_amd", "libtdaeeg.so")
    if not (os.path.exists(objdump) and os.path.exists(readelf) and os.path.exists(lib)):
        pytest.skip("ROCm binutils or the built library are not here")
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    seen = 0
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for entry in notes.split(".agpr_count:")[1:]:           # one metadata entry per kernel, .agpr_count its first key
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if "rips_cloud_kernelILi512ELi1EjLb0ELb1E" not in name:
                continue
            seen += 1
            agpr = int(re.match(r"\s*(\d+)", entry).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
            vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
            print(f"{name}: {vgpr} VGPRs, {agpr} AGPRs, private segment {scratch} bytes")
            assert agpr == 0, f"{name} uses {agpr} AGPRs"
            assert scratch == 0, f"{name} has a private segment of {scratch} bytes"
            assert vgpr <= 80, f"{name} uses {vgpr} VGPRs: three workgroups of 512 per CU need 80 or fewer"
    assert seen == 1, seen
