"""The insertion's kernels (svo_kernels_insert.hip) as the compiler left them in libsvo_hip.so, read like
test_consolidate_code_object.py reads the consolidation's: the three kernels present, no scratch, no spills, no AGPRs, static LDS at
most what the kernel declares (the scan's sixteen wave sums: 64 bytes; the other two none), and registers within what a block of
its size may hold: 256 for the 256-thread kernels, 128 for the scan's 1024 threads.
Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, most bytes of static LDS, most VGPRs)
INSERT = {"_Z14k_insert_count": ("k_insert_count", 0, 256), "_Z13k_insert_scan": ("k_insert_scan", 64, 128), "_Z12k_insert_put": ("k_insert_put", 0, 256)}


@pytest.fixture(scope="module")
def insert_kernels():
    return by_prefix(INSERT)


def test_the_insertion_kernels_are_built(insert_kernels):
    missing = [v[0] for k, v in INSERT.items() if k not in insert_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(INSERT), ids=lambda s: INSERT[s][0])
def test_insertion_kernel_budget(insert_kernels, sym):
    name, lds, vgprs = INSERT[sym]
    k = insert_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
