"""The landmark fusion's kernels (svo_kernels_fuse.hip) as the compiler left them in libsvo_hip.so, read like
test_align_code_object.py reads the alignment's: the four kernels present, no scratch, no spills, no AGPRs, no LDS in any of them
(the search kernel's ballots and the counts' popcounts need none), within the registers of their block sizes: 512 for the one wave of
the search kernel, 256 for the 256 threads of the other three.
As built: k_desc_match_near 25 VGPRs / 50 SGPRs, k_fuse_map 12 / 22, k_fuse_insert 11 / 33, k_fuse_sweep 14 / 26.  Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, bytes of LDS, most VGPRs)
FUSE = {"_Z17k_desc_match_near": ("k_desc_match_near", 0, 512), "_Z10k_fuse_map": ("k_fuse_map", 0, 256),
        "_Z13k_fuse_insert": ("k_fuse_insert", 0, 256), "_Z12k_fuse_sweep": ("k_fuse_sweep", 0, 256)}


@pytest.fixture(scope="module")
def fuse_kernels():
    return by_prefix(FUSE)


def test_the_fuse_kernels_are_built(fuse_kernels):
    missing = [v[0] for k, v in FUSE.items() if k not in fuse_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(FUSE), ids=lambda s: FUSE[s][0])
def test_fuse_kernel_budget(fuse_kernels, sym):
    name, lds, vgprs = FUSE[sym]
    k = fuse_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
