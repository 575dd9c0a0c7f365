"""The batched place candidates' kernels (svo_kernels_place_batch.hip) as the compiler left them in libsvo_hip.so, read like
test_place_code_object.py reads the single calls': the kernels present, no scratch, no spills, no AGPRs, static LDS at most what
the kernel declares (the insert's four wave sums: 16 bytes; the pick's sixteen wave maxima, sixteen wave counts and 64 chosen bins:
448 bytes; the list and the sweep hold nothing in LDS — the table is global), within the registers of their block sizes: 256 for
the 256 threads of the list, the insert and the sweep, 128 for the 1024 threads of the pick.
As built: k_place_batch_list 8 VGPRs / 26 SGPRs, k_place_batch_insert 15 / 43, k_place_batch_sweep 36 / 56, k_place_batch_pick 66 / 57.
Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, most bytes of static LDS, most VGPRs)
PLACE_BATCH = {"_Z18k_place_batch_list": ("k_place_batch_list", 0, 256), "_Z20k_place_batch_insert": ("k_place_batch_insert", 16, 256),
               "_Z19k_place_batch_sweep": ("k_place_batch_sweep", 0, 256), "_Z18k_place_batch_pick": ("k_place_batch_pick", 448, 128)}


@pytest.fixture(scope="module")
def place_batch_kernels():
    return by_prefix(PLACE_BATCH)


def test_the_place_batch_kernels_are_built(place_batch_kernels):
    missing = [v[0] for k, v in PLACE_BATCH.items() if k not in place_batch_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(PLACE_BATCH), ids=lambda s: PLACE_BATCH[s][0])
def test_place_batch_kernel_budget(place_batch_kernels, sym):
    name, lds, vgprs = PLACE_BATCH[sym]
    k = place_batch_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
