"""The pose-covariance kernel (svo_kernels_pnp.hip, k_pose_cov) as the compiler left it in libsvo_hip.so, read like
test_pnp_code_object.py reads its neighbours.  A co-resident context launches the `_lean` build beside four LK waves of 104
registers, which leave 96 per lane: it may hold no more, in VGPRs and AGPRs together.  The full build keeps the 28 sums in
registers (no scratch).  Both share PcShared.  The counts as built are in profiles/r11_pose_cov_code_object.md."""
import re
import subprocess

import pytest

from test_lk_code_object import LIB, READELF, device_code_objects
from test_lk_code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

KERNELS = {"_Z10k_pose_cov10DevBuffers7CovArgs": "k_pose_cov", "_Z15k_pose_cov_lean10DevBuffers7CovArgs": "k_pose_cov_lean"}
FIELDS = r"\.(agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|group_segment_fixed_size):\s+(\d+)"


@pytest.fixture(scope="module")
def cov_kernels(tmp_path_factory):
    d = tmp_path_factory.mktemp("co_cov")
    found = {}
    objs = device_code_objects(LIB)
    assert objs, "no AMDGPU code object found in %s (a compressed fat binary?)" % LIB
    for i, img in enumerate(objs):
        p = d / ("co%d.elf" % i)
        p.write_bytes(img)
        notes = subprocess.run([READELF, "--notes", str(p)], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- (?=\.agpr_count:)", notes):
            m = re.search(r"\.name:\s+(\S+)", block)
            if m and m.group(1) in KERNELS:
                found[KERNELS[m.group(1)]] = {k: int(v) for k, v in re.findall(FIELDS, block)}
    return found


def test_both_builds_exist(cov_kernels):
    print(cov_kernels)
    assert sorted(cov_kernels) == sorted(KERNELS.values()), sorted(cov_kernels)


def test_co_resident_build_fits_beside_four_lk_waves(cov_kernels):
    k = cov_kernels["k_pose_cov_lean"]
    print(k)
    assert k["vgpr_count"] + k["agpr_count"] <= 96, k


def test_full_build_has_no_scratch(cov_kernels):
    k = cov_kernels["k_pose_cov"]
    print(k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k


def test_builds_share_their_lds_layout(cov_kernels):
    full, lean = cov_kernels["k_pose_cov"], cov_kernels["k_pose_cov_lean"]
    assert full["group_segment_fixed_size"] == lean["group_segment_fixed_size"] > 0, (full, lean)
