"""The masked detection kernels (svo_kernels_img.hip: k_fast_masked, k_fast_strided_masked, k_fast_score_map_masked) as the compiler
left them in libsvo_hip.so, read like test_detect_code_object.py reads the plain ones: present, no scratch, no spills, the LDS of
one FAST tile (5432 bytes, as the plain kernels), and at most 64 VGPRs — the step below which a SIMD holds eight waves of a kernel,
where the plain FAST kernels (50 and 61 registers) sit too.  Found when they were written (profiles/r12_detect_mask_code_object.md):
k_fast_masked 53 VGPRs, k_fast_strided_masked 62, k_fast_score_map_masked 50; 5432 bytes of LDS each; no scratch, no spills.  That
the plain kernels did not move is test_detect_code_object.py's and test_img_code_object.py's business."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# Itanium-mangled prefix of the kernel symbol -> (readable name, LDS bytes, VGPR bound)
MASKED = {
    "_Z13k_fast_masked10DevBuffers8MaskArgs": ("k_fast_masked", 5432, 64),
    "_Z21k_fast_strided_masked10DevBuffers8MaskArgs": ("k_fast_strided_masked", 5432, 64),
    "_Z23k_fast_score_map_maskedPKh": ("k_fast_score_map_masked", 5432, 64),
}


@pytest.fixture(scope="module")
def masked_kernels():
    return by_prefix(MASKED)


def test_every_masked_kernel_is_built(masked_kernels):
    missing = [v[0] for k, v in MASKED.items() if k not in masked_kernels]
    assert not missing, (missing, sorted(masked_kernels))


@pytest.mark.parametrize("sym", sorted(MASKED), ids=lambda s: MASKED[s][0])
def test_masked_kernel_budget(masked_kernels, sym):
    name, lds, vgprs = MASKED[sym]
    k = masked_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= vgprs, k
