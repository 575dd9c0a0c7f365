"""The converting ingest kernels (include/svo.h, input formats) as the compiler left them in libsvo_hip.so, read like
test_img_code_object.py reads the plain ones.  Only the tile fill differs from the plain kernel of the same tile, so the LDS is
the plain kernel's; none may use scratch; and the non-rectifying many-sequence forms run on the image stream beside the LK
kernel's six waves of 80 registers, which leave 32 registers per lane.  The rectifying x converting forms are
printed: DESIGN.md section 2 records their counts and what a count above 32 costs the build-ahead path."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

BPPS = (2, 3, 4)                                  # yuv422 | bgr8 rgb8 | bgra8 rgba8
RECT = {False: "Lb0E", True: "Lb1E"}

# Itanium-mangled prefix of the kernel symbol -> (readable name, LDS bytes, VGPR limit or None)
KERNELS = {}
for bpp in BPPS:
    for rect in (False, True):
        KERNELS["_Z13k_ingest_greyILi%dE%sEv" % (bpp, RECT[rect])] = ("k_ingest_grey<%d, %s>" % (bpp, rect), 0, None)
        KERNELS["_Z18k_ingest_pyr1_greyILi%dELi32ELi8E%sEv" % (bpp, RECT[rect])] = ("k_ingest_pyr1_grey<%d, 32, 8, %s>" % (bpp, rect), 2512, None)
        KERNELS["_Z18k_ingest_pyr1_greyILi%dELi64ELi16E%sEv" % (bpp, RECT[rect])] = (
            "k_ingest_pyr1_grey<%d, 64, 16, %s>" % (bpp, rect), 9104, None if rect else 32)
        KERNELS["_Z14k_front_a_greyILi%dE%sEv" % (bpp, RECT[rect])] = ("k_front_a_grey<%d, %s>" % (bpp, rect), 7952, None)
    KERNELS["_Z14k_convert_grayILi%dEEv" % bpp] = ("k_convert_gray<%d>" % bpp, 0, None)


@pytest.fixture(scope="module")
def kernels():
    return by_prefix(KERNELS)


def test_every_converting_kernel_is_built(kernels):
    missing = [v[0] for k, v in KERNELS.items() if k not in kernels]
    assert not missing, (missing, sorted(kernels))


@pytest.mark.parametrize("sym", sorted(KERNELS), ids=lambda s: KERNELS[s][0])
def test_converting_kernel_budget(kernels, sym):
    name, lds, vgprs = KERNELS[sym]
    k = kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    if vgprs is not None:
        assert k["vgpr_count"] <= vgprs, k
