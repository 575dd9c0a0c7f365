"""The relocaliser's kernel (svo_kernels_reloc.hip: k_reloc_select) as the compiler left it in libsvo_hip.so, read like
test_desc_match_code_object.py reads the search kernels: present, no scratch, no spills, no AGPRs, at most 128 VGPRs — what a wave of
a 1024-thread block may hold — and the static LDS the layout implies: 4096 ids of 8 bytes, 4096 keys of 4 bytes and the 16 wave
totals, 49 216 bytes, inside the 64 KiB a block may take."""

import pytest

from code_object import by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

LDS = 4096 * 8 + 4096 * 4 + 16 * 4
RELOC = {"_Z14k_reloc_select9RelocArgs": ("k_reloc_select", 128)}


@pytest.fixture(scope="module")
def reloc_kernels():
    return by_name(RELOC)


def test_the_reloc_kernel_is_built(reloc_kernels):
    missing = [v[0] for k, v in RELOC.items() if k not in reloc_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(RELOC), ids=lambda s: RELOC[s][0])
def test_reloc_kernel_budget(reloc_kernels, sym):
    name, vgprs = RELOC[sym]
    k = reloc_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == LDS <= 64 * 1024, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
