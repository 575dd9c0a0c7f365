"""The LK kernels as the compiler left them in libsvo_hip.so: register counts and scratch from the code-object metadata, read with the
ROCm llvm-readelf.  No GPU: the device code objects are cut out of the library's fat binary on the host.  Pins the default build's
budget (w = 21 grey, exact sums: at most 80 VGPRs = six waves per SIMD, no scratch) and that the dispatcher's whole table is built."""
import os
import re
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "stereo_visual_odometry_amd", "libsvo_hip.so")
EM_AMDGPU = 224


def find_readelf():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf")):
        if c and os.path.exists(c):
            return c
    return None


READELF = find_readelf()
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or READELF is None, reason="libsvo_hip.so is not built or llvm-readelf is missing")


def device_code_objects(path):
    """Every AMDGPU ELF image inside the file (the fat binary holds one per translation unit, uncompressed)."""
    blob = open(path, "rb").read()
    out = []
    pos = blob.find(b"\x7fELF", 1)
    while pos >= 0:
        hdr = blob[pos:pos + 64]
        if len(hdr) == 64 and hdr[4] == 2 and hdr[5] == 1 and struct.unpack_from("<H", hdr, 18)[0] == EM_AMDGPU:
            shoff, = struct.unpack_from("<Q", hdr, 40)
            shentsize, shnum = struct.unpack_from("<HH", hdr, 58)
            out.append(blob[pos:pos + shoff + shentsize * shnum])
        pos = blob.find(b"\x7fELF", pos + 4)
    return out


@pytest.fixture(scope="module")
def lk_kernels(tmp_path_factory):
    """{(W, CN, FS): metadata dict} of every k_lk_chain in the library"""
    d = tmp_path_factory.mktemp("co")
    found = {}
    objs = device_code_objects(LIB)
    assert objs, "no AMDGPU code object found in %s (a compressed fat binary?)" % LIB
    for i, img in enumerate(objs):
        p = d / ("co%d.elf" % i)
        p.write_bytes(img)
        notes = subprocess.run([READELF, "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        # one YAML map per kernel: "- .agpr_count: ..." up to the next list item
        for block in re.split(r"\n\s*- \.agpr_count:", notes):
            m = re.search(r"\.name:\s+_Z10k_lk_chainILi(\d+)ELi(\d+)ELb([01])EEv", block)
            if not m:
                continue
            vals = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|group_segment_fixed_size):\s+(\d+)", block)}
            found[(int(m.group(1)), int(m.group(2)), bool(int(m.group(3))))] = vals
    return found


def test_default_build_keeps_six_waves_without_scratch(lk_kernels):
    k = lk_kernels.get((21, 1, False))
    assert k is not None, sorted(lk_kernels)
    print("k_lk_chain<21, 1, false>:", k)
    assert k["vgpr_count"] <= 80, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= 16, k          # the exact-sums build uses no LDS beyond the placeholder array


def test_every_dispatched_window_has_a_kernel(lk_kernels):
    """lk_built() in svo_kernels_lk.hip: grey 5..31 and BGR 5..21, each in both summation modes."""
    want = [(w, 1, fs) for w in range(5, 32) for fs in (False, True)] + [(w, 3, fs) for w in range(5, 22) for fs in (False, True)]
    missing = [k for k in want if k not in lk_kernels]
    assert not missing, missing
    assert len(lk_kernels) == len(want), sorted(set(lk_kernels) - set(want))
