"""The kernels as the compiler left them in libsvo_hip.so, for the test_*_code_object.py files: register counts, scratch and LDS
from the code-object metadata, read with the ROCm llvm-readelf.  No GPU: the device code objects are cut out of the library's fat
binary on the host, once per process, however many of those files are collected."""
import functools
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "stereo_visual_odometry_amd", "libsvo_hip.so")
EM_AMDGPU = 224
FIELDS = r"\.(agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)"


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


@functools.lru_cache(maxsize=None)
def kernels():
    """{mangled kernel name: {field of FIELDS: int}} of every kernel of every code object in the library"""
    objs = device_code_objects(LIB)
    assert objs, "no AMDGPU code object found in %s (a compressed fat binary?)" % LIB
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for i, img in enumerate(objs):
            p = os.path.join(d, "co%d.elf" % i)
            with open(p, "wb") as f:
                f.write(img)
            notes = subprocess.run([READELF, "--notes", p], capture_output=True, text=True, check=True).stdout
            # one YAML map per kernel: "- .agpr_count: ..." up to the next list item; the look-ahead keeps agpr_count with its kernel
            for block in re.split(r"\n\s*- (?=\.agpr_count:)", notes):
                m = re.search(r"\.name:\s+(\S+)", block)
                if m:
                    found[m.group(1)] = {k: int(v) for k, v in re.findall(FIELDS, block)}
    return found


def by_name(table):
    """{key of `table`: metadata} of the kernels whose mangled name is a key of `table`"""
    return {name: k for name, k in kernels().items() if name in table}


def by_prefix(table):
    """{key of `table`: metadata} of the kernels whose mangled name starts with a key of `table` (the first such key)"""
    found = {}
    for name, k in kernels().items():
        key = next((p for p in table if name.startswith(p)), None)
        if key:
            found[key] = k
    return found
