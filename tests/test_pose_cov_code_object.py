"""The pose-covariance kernel (svo_kernels_pnp.hip, k_pose_cov) as the compiler left it in libsvo_hip.so, read like
test_pnp_code_object.py reads its neighbours.  A co-resident context launches the `_lean` build beside four LK waves of 104
registers, which leave 96 per lane: it may hold no more, in VGPRs and AGPRs together.  The full build keeps the 28 sums in
registers (no scratch).  Both share PcShared.  The counts as built are in profiles/r11_pose_cov_code_object.md."""

import pytest

from code_object import by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

KERNELS = {"_Z10k_pose_cov10DevBuffers7CovArgs": "k_pose_cov", "_Z15k_pose_cov_lean10DevBuffers7CovArgs": "k_pose_cov_lean"}


@pytest.fixture(scope="module")
def cov_kernels():
    return {KERNELS[name]: k for name, k in by_name(KERNELS).items()}


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
