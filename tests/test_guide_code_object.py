"""The guided search's kernels (svo_kernels_guide.hip: k_guide_project, k_desc_match_guided) as the compiler left them in
libsvo_hip.so, read like test_reloc_code_object.py reads the relocaliser's: both present, no scratch, no spills, no AGPRs, no LDS;
k_desc_match_guided in no more VGPRs than k_desc_match's 38 (the gate must not cost the search its occupancy; 22 as built),
k_guide_project in at most 64 (18 as built)."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

GUIDE = {"_Z15k_guide_project": ("k_guide_project", 64), "_Z19k_desc_match_guided": ("k_desc_match_guided", 38)}


@pytest.fixture(scope="module")
def guide_kernels():
    return by_prefix(GUIDE)


def test_the_guide_kernels_are_built(guide_kernels):
    missing = [v[0] for k, v in GUIDE.items() if k not in guide_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(GUIDE), ids=lambda s: GUIDE[s][0])
def test_guide_kernel_budget(guide_kernels, sym):
    name, vgprs = GUIDE[sym]
    k = guide_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
