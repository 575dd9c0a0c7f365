"""The place candidates' kernels (svo_kernels_place.hip) as the compiler left them in libsvo_hip.so, read like
test_fuse_code_object.py reads the fusion's: the kernels present — the sweep in both builds, with and without the wave-combined
atomics — no scratch, no spills, no AGPRs, static LDS at most what the kernel declares (the sweep's set is dynamic LDS, 64 KiB at most,
and is not in the metadata: 0; the pick's sixteen wave maxima: 128 bytes), within the registers of their block sizes: 256 for the
256 threads of the sweep and the compaction, 128 for the 1024 threads of the pick.
As built: k_place_sweep<true> 22 VGPRs / 48 SGPRs, k_place_sweep<false> 12 / 47, k_place_compact 8 / 20, k_place_pick 38 / 46.
Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, most bytes of static LDS, most VGPRs)
PLACE = {"_Z13k_place_sweepILb1EE": ("k_place_sweep<combine>", 0, 256), "_Z13k_place_sweepILb0EE": ("k_place_sweep<plain>", 0, 256),
         "_Z15k_place_compact": ("k_place_compact", 0, 256), "_Z12k_place_pick": ("k_place_pick", 128, 128)}


@pytest.fixture(scope="module")
def place_kernels():
    return by_prefix(PLACE)


def test_the_place_kernels_are_built(place_kernels):
    missing = [v[0] for k, v in PLACE.items() if k not in place_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(PLACE), ids=lambda s: PLACE[s][0])
def test_place_kernel_budget(place_kernels, sym):
    name, lds, vgprs = PLACE[sym]
    k = place_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
