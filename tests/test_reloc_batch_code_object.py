"""The batched relocalisation's kernels (svo_kernels_reloc_batch.hip) as the compiler left them in libsvo_hip.so, read like
test_desc_retire_code_object.py reads the maintenance kernels: the three the call is built on and the inlier gather present, no
scratch, no spills, no AGPRs, the LDS the file's header states — 8192 bytes of projections in the search, 32768 of sort entries in
the order kernel, 49216 in the selection as in k_reloc_select — and at most 64 VGPRs in the search kernel, whose block is 16 waves.
As built: k_desc_match_guided_batch 42 VGPRs / 98 SGPRs, k_reloc_batch_order 30 / 36, k_reloc_select_batch 44 / 93,
k_reloc_batch_inliers 4 / 17.  Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, bytes of LDS, most VGPRs)
BATCH = {"_Z25k_desc_match_guided_batch": ("k_desc_match_guided_batch", 8192, 64), "_Z19k_reloc_batch_order": ("k_reloc_batch_order", 32768, 64),
         "_Z20k_reloc_select_batch": ("k_reloc_select_batch", 49216, 64), "_Z21k_reloc_batch_inliers": ("k_reloc_batch_inliers", 0, 64)}


@pytest.fixture(scope="module")
def batch_kernels():
    return by_prefix(BATCH)


def test_the_batch_kernels_are_built(batch_kernels):
    missing = [v[0] for k, v in BATCH.items() if k not in batch_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(BATCH), ids=lambda s: BATCH[s][0])
def test_batch_kernel_budget(batch_kernels, sym):
    name, lds, vgprs = BATCH[sym]
    k = batch_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
