"""The consolidation's kernels (svo_kernels_consolidate.hip) as the compiler left them in libsvo_hip.so, read like
test_place_code_object.py reads the place candidates': the six kernels present, no scratch, no spills, no AGPRs, static LDS at most
what the kernel declares (the scan's four wave sums: 16 bytes; the group kernel keeps its views in registers: none), within the 256
registers of a block of 256 threads.
As built: k_cons_insert 12 VGPRs / 33 SGPRs, k_cons_place 14 / 28, k_cons_scan 13 / 16, k_cons_offsets 4 / 18, k_cons_scatter 14 / 32,
k_cons_group 36 / 44.
Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, most bytes of static LDS, most VGPRs)
CONS = {"_Z13k_cons_insert": ("k_cons_insert", 0, 256), "_Z12k_cons_place": ("k_cons_place", 0, 256), "_Z11k_cons_scan": ("k_cons_scan", 16, 256),
        "_Z14k_cons_offsets": ("k_cons_offsets", 0, 256), "_Z14k_cons_scatter": ("k_cons_scatter", 0, 256), "_Z12k_cons_group": ("k_cons_group", 0, 256)}


@pytest.fixture(scope="module")
def cons_kernels():
    return by_prefix(CONS)


def test_the_consolidation_kernels_are_built(cons_kernels):
    missing = [v[0] for k, v in CONS.items() if k not in cons_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(CONS), ids=lambda s: CONS[s][0])
def test_consolidation_kernel_budget(cons_kernels, sym):
    name, lds, vgprs = CONS[sym]
    k = cons_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
