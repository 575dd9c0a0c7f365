"""The pyramid kernels (ingest, pyrDown, borders) as the compiler left them in libsvo_hip.so, read like test_lk_code_object.py reads
the LK kernels.  They run beside the LK kernel's six waves of 80 registers, which leave 32 registers per lane, so none
may need more; none may use scratch; and their LDS follows from the tile constants (k_front_a / k_front_b run a pyramid body
beside a detection body, so theirs is the larger of the two)."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# Itanium-mangled prefix of the kernel symbol -> (readable name, LDS bytes)
PYRAMID = {
    "_Z8k_ingestILi1ELb0EEv": ("k_ingest<1, false>", 0), "_Z8k_ingestILi1ELb1EEv": ("k_ingest<1, true>", 0),
    "_Z8k_ingestILi3ELb0EEv": ("k_ingest<3, false>", 0), "_Z8k_ingestILi3ELb1EEv": ("k_ingest<3, true>", 0),
    "_Z13k_ingest_pyr1ILi32ELi8ELb0EEv": ("k_ingest_pyr1<32, 8, false>", 2512), "_Z13k_ingest_pyr1ILi32ELi8ELb1EEv": ("k_ingest_pyr1<32, 8, true>", 2512),
    "_Z13k_ingest_pyr1ILi64ELi16ELb0EEv": ("k_ingest_pyr1<64, 16, false>", 9104), "_Z13k_ingest_pyr1ILi64ELi16ELb1EEv": ("k_ingest_pyr1<64, 16, true>", 9104),
    "_Z9k_pyrdown10DevBuffers": ("k_pyrdown", 2512), "_Z10k_pyrdown210DevBuffers": ("k_pyrdown2", 7376), "_Z13k_pad_pyramid10DevBuffers": ("k_pad_pyramid", 0),
}
# lone stream only, nothing runs beside them: (name, LDS bytes = their larger half's, the register count they were merged with)
FRONT = {"_Z9k_front_aILb0EEv": ("k_front_a<false>", 7952, 50), "_Z9k_front_aILb1EEv": ("k_front_a<true>", 7952, 50), "_Z9k_front_b10DevBuffers": ("k_front_b", 7424, 30)}


@pytest.fixture(scope="module")
def img_kernels():
    return by_prefix(list(PYRAMID) + list(FRONT))


def test_every_pyramid_kernel_is_built(img_kernels):
    missing = [v[0] for k, v in list(PYRAMID.items()) + list(FRONT.items()) if k not in img_kernels]
    assert not missing, (missing, sorted(img_kernels))


@pytest.mark.parametrize("sym", sorted(PYRAMID), ids=lambda s: PYRAMID[s][0])
def test_pyramid_kernel_fits_beside_lk(img_kernels, sym):
    k = img_kernels[sym]
    print(PYRAMID[sym][0], k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == PYRAMID[sym][1], k
    assert k["vgpr_count"] <= 32, k


@pytest.mark.parametrize("sym", sorted(FRONT), ids=lambda s: FRONT[s][0])
def test_fused_front_kernel_budget(img_kernels, sym):
    k = img_kernels[sym]
    print(FRONT[sym][0], k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == FRONT[sym][1], k
    assert k["vgpr_count"] <= FRONT[sym][2], k
