"""The index-maintenance kernels (svo_kernels_retire.hip) as the compiler left them in libsvo_hip.so, read like
test_guide_code_object.py reads the guided search's: all nine present, no scratch, no spills, no AGPRs, at most 64 VGPRs (22 at most
as built), and LDS only where the block scan has its four waves meet — 16 bytes in k_retire_count, k_retire_scan and k_retire_rank,
none anywhere else.  Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, bytes of LDS); the length prefix keeps k_retire_put apart from anything longer
RETIRE = {"_Z14k_retire_flags": ("k_retire_flags", 0), "_Z15k_retire_insert": ("k_retire_insert", 0), "_Z15k_retire_latest": ("k_retire_latest", 0),
          "_Z14k_retire_count": ("k_retire_count", 16), "_Z13k_retire_scan": ("k_retire_scan", 16), "_Z13k_retire_rank": ("k_retire_rank", 16),
          "_Z15k_retire_gather": ("k_retire_gather", 0), "_Z12k_retire_put": ("k_retire_put", 0), "_Z18k_transform_points": ("k_transform_points", 0)}


@pytest.fixture(scope="module")
def retire_kernels():
    return by_prefix(RETIRE)


def test_the_retire_kernels_are_built(retire_kernels):
    missing = [v[0] for k, v in RETIRE.items() if k not in retire_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(RETIRE), ids=lambda s: RETIRE[s][0])
def test_retire_kernel_budget(retire_kernels, sym):
    name, lds = RETIRE[sym]
    k = retire_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= 64 and k["agpr_count"] == 0, k
