"""The descriptor index's kernels (svo_kernels_match.hip: k_desc_match, k_desc_match_merge) as the compiler left them in
libsvo_hip.so, read like test_descriptor_code_object.py reads the descriptor kernels: both present, no scratch, no spills, no AGPRs,
at or below 64 VGPRs — the step below which a SIMD holds eight waves of a kernel — and the LDS the layout implies: none, an index row
reaches the 64 lanes of a wave through scalar registers, and the merge folds its lanes with cross-lane moves."""

import pytest

from code_object import by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

LDS = 0                                               # no row is staged in LDS, and the merge folds its lanes in registers
# Itanium-mangled kernel symbol -> (readable name, VGPR bound)
MATCH = {
    "_Z12k_desc_matchPKjPKmS0_i10MatchRangeP12MatchPartial": ("k_desc_match", 64),
    "_Z18k_desc_match_mergePK12MatchPartialPKmiiP14svo_desc_match": ("k_desc_match_merge", 64),
}


@pytest.fixture(scope="module")
def match_kernels():
    return by_name(MATCH)


def test_both_match_kernels_are_built(match_kernels):
    missing = [v[0] for k, v in MATCH.items() if k not in match_kernels]
    assert not missing, (missing, sorted(match_kernels))


@pytest.mark.parametrize("sym", sorted(MATCH), ids=lambda s: MATCH[s][0])
def test_match_kernel_budget(match_kernels, sym):
    name, vgprs = MATCH[sym]
    k = match_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == LDS, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
