"""The CLAHE kernels (svo_kernels_img.hip: k_clahe_lut<BPP>, k_clahe_apply<BPP>, BPP = 1 .. 4) as the compiler left them in
libsvo_hip.so, read like test_detect_mask_code_object.py reads the masked detection kernels: every instantiation present, no scratch,
no spills, and within the LDS and VGPR figures found when they were written (profiles/r13_clahe_code_object.md): k_clahe_lut 20 - 21
VGPRs and 4128 bytes of LDS (four per-wave histograms and the two partial-sum rows), k_clahe_apply 41 VGPRs and 8192 bytes (two LUT
rows of 16 tiles).  Both stay at or below 64 VGPRs, the step below which a SIMD holds eight waves of a kernel."""

import pytest

from code_object import by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# Itanium-mangled kernel symbol -> (readable name, LDS bytes, VGPR bound)
CLAHE = {}
for bpp in (1, 2, 3, 4):
    CLAHE["_Z11k_clahe_lutILi%dEEv9ClaheArgs" % bpp] = ("k_clahe_lut<%d>" % bpp, 4128, 24)
    CLAHE["_Z13k_clahe_applyILi%dEEv9ClaheArgs" % bpp] = ("k_clahe_apply<%d>" % bpp, 8192, 48)


@pytest.fixture(scope="module")
def clahe_kernels():
    return by_name(CLAHE)


def test_every_clahe_kernel_is_built(clahe_kernels):
    missing = [v[0] for k, v in CLAHE.items() if k not in clahe_kernels]
    assert not missing, (missing, sorted(clahe_kernels))


@pytest.mark.parametrize("sym", sorted(CLAHE), ids=lambda s: CLAHE[s][0])
def test_clahe_kernel_budget(clahe_kernels, sym):
    name, lds, vgprs = CLAHE[sym]
    k = clahe_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= vgprs, k
