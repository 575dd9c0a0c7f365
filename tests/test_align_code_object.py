"""The map alignment's kernels (svo_kernels_align.hip) as the compiler left them in libsvo_hip.so, read like
test_reloc_batch_code_object.py reads the batch's: the three kernels present, no scratch, no spills, no AGPRs, and the LDS the
file's header states — 49216 bytes in the pair kernel, as in k_reloc_select; none in the scoring kernel; 880 in the fit kernel —
within the registers of their block sizes: 128 for the 1024 threads of the pair kernel, 256 for the 256 of the other two.
As built: k_align_pairs 51 VGPRs / 98 SGPRs, k_align_score 124 / 36, k_align_fit 178 / 48.  Metadata only."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# mangled prefix -> (name, bytes of LDS, most VGPRs)
ALIGN = {"_Z13k_align_pairs": ("k_align_pairs", 49216, 128), "_Z13k_align_score": ("k_align_score", 0, 256), "_Z11k_align_fit": ("k_align_fit", 880, 256)}


@pytest.fixture(scope="module")
def align_kernels():
    return by_prefix(ALIGN)


def test_the_align_kernels_are_built(align_kernels):
    missing = [v[0] for k, v in ALIGN.items() if k not in align_kernels]
    assert not missing, missing


@pytest.mark.parametrize("sym", sorted(ALIGN), ids=lambda s: ALIGN[s][0])
def test_align_kernel_budget(align_kernels, sym):
    name, lds, vgprs = ALIGN[sym]
    k = align_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= vgprs and k["agpr_count"] == 0, k
