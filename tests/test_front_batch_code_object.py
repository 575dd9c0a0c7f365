"""The kernels of the many-sequence front as the compiler left them in libsvo_hip.so, read like test_img_code_object.py reads the
pyramid kernels: the batch FAST kernel and the re-tiled plane kernel exist, nothing uses scratch or spills, the image stream's
kernels fit the 32 registers per lane the LK kernel's six waves leave, k_deriv_levels keeps no LDS, and k_fast_batch
needs no more registers than k_fast<0>, whose place it takes."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# Itanium-mangled prefix of the kernel symbol -> readable name
IMAGE_STREAM = {
    "_Z13k_ingest_pyr1ILi64ELi16ELb0EEv": "k_ingest_pyr1<64, 16, false>", "_Z10k_pyrdown210DevBuffers": "k_pyrdown2",
    "_Z9k_pyrdown10DevBuffers": "k_pyrdown", "_Z13k_pad_pyramid10DevBuffers": "k_pad_pyramid", "_Z14k_deriv_levels10DevBuffers": "k_deriv_levels",
}
FAST_BATCH, FAST_0 = "_Z12k_fast_batch10DevBuffers", "_Z6k_fastILi0EEv"
FAST_BATCH_LDS = 40 * 76 + 34 * 68 + 2 * 34 * 66 + 4 + 4         # pixels (64 x 32 + 4 halo, rows of 76), scores, the candidate queue, its count (+ 4 of alignment)


@pytest.fixture(scope="module")
def kernels():
    return by_prefix(list(IMAGE_STREAM) + [FAST_BATCH, FAST_0])


def test_the_new_symbols_exist(kernels):
    missing = [s for s in list(IMAGE_STREAM) + [FAST_BATCH, FAST_0] if s not in kernels]
    assert not missing, (missing, sorted(kernels))


@pytest.mark.parametrize("sym", sorted(IMAGE_STREAM) + [FAST_BATCH], ids=lambda s: IMAGE_STREAM.get(s, "k_fast_batch"))
def test_no_scratch_and_no_spills(kernels, sym):
    k = kernels[sym]
    print(sym, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


@pytest.mark.parametrize("sym", sorted(IMAGE_STREAM), ids=lambda s: IMAGE_STREAM[s])
def test_image_stream_kernel_fits_beside_lk(kernels, sym):
    assert kernels[sym]["vgpr_count"] <= 32, kernels[sym]


def test_plane_and_border_kernels_keep_no_lds(kernels):
    assert kernels["_Z14k_deriv_levels10DevBuffers"]["group_segment_fixed_size"] == 0
    assert kernels["_Z13k_pad_pyramid10DevBuffers"]["group_segment_fixed_size"] == 0


def test_batch_fast_needs_no_more_registers_than_the_tile_it_replaces(kernels):
    b, f = kernels[FAST_BATCH], kernels[FAST_0]
    print(b, f)
    assert b["vgpr_count"] <= f["vgpr_count"], (b, f)
    assert b["group_segment_fixed_size"] == FAST_BATCH_LDS, b
