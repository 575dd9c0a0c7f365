"""The descriptor kernels (svo_kernels_desc.hip: k_track_desc, k_track_desc_lean, k_describe_points) as the compiler left them in
libsvo_hip.so, read like test_clahe_code_object.py reads the CLAHE kernels: all three present, no scratch, no spills, the LDS the
layout implies — four waves x (a 32 x 32 byte patch + a 31 x 32 and a 27 x 32 u16 sum plane) + four 32-byte rows = 19072 bytes — and
within the VGPR bounds: the lean build at or below the 48 of k_track_obs_lean, the others at or below 64, the step below which a
SIMD holds eight waves of a kernel.  Found when they were written (profiles/r21_descriptor_code_object.md): 29, 29 and 31 VGPRs."""

import pytest

from code_object import by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

LDS = 4 * (32 * 32 + 31 * 32 * 2 + 27 * 32 * 2) + 4 * 32
# Itanium-mangled kernel symbol -> (readable name, VGPR bound)
DESC = {
    "_Z12k_track_desc10DevBuffers8DescArgs": ("k_track_desc", 64),
    "_Z17k_track_desc_lean10DevBuffers8DescArgs": ("k_track_desc_lean", 48),
    "_Z17k_describe_pointsPKhiiiPK15HIP_vector_typeIfLj2EEiPhPi": ("k_describe_points", 64),
}


@pytest.fixture(scope="module")
def desc_kernels():
    return by_name(DESC)


def test_every_descriptor_kernel_is_built(desc_kernels):
    missing = [v[0] for k, v in DESC.items() if k not in desc_kernels]
    assert not missing, (missing, sorted(desc_kernels))


@pytest.mark.parametrize("sym", sorted(DESC), ids=lambda s: DESC[s][0])
def test_descriptor_kernel_budget(desc_kernels, sym):
    name, vgprs = DESC[sym]
    k = desc_kernels[sym]
    print(name, k)
    assert LDS == 19072
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == LDS, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
