"""The geometry kernels (triangulation, RANSAC-PnP) as the compiler left them in libsvo_hip.so, read like test_lk_code_object.py
reads the LK kernels.  The `_lean` builds exist to start beside four LK waves of 104 registers, which leave 96 per lane: none may
hold more, in VGPRs and AGPRs together.  The full EPnP builds keep their linear algebra in registers (no scratch) and their arena
in static LDS, (64 / EP_G_LONE) hypotheses of EP_STRIDE doubles; the two refine builds share LmShared."""
import os
import re

import pytest

from code_object import ROOT, by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# Itanium-mangled symbol -> readable name: the twelve kernels of svo_kernels_pnp.hip
KERNELS = {
    "_Z13k_triangulate10DevBuffersi": "k_triangulate", "_Z18k_triangulate_lean10DevBuffersi": "k_triangulate_lean",
    "_Z13k_pnp_subsets10DevBuffers": "k_pnp_subsets", "_Z10k_pnp_epnp10DevBuffersii": "k_pnp_epnp", "_Z10k_tri_epnp10DevBuffersiii": "k_tri_epnp",
    "_Z15k_pnp_epnp_lean10DevBuffersii": "k_pnp_epnp_lean", "_Z11k_pnp_score10DevBuffersii": "k_pnp_score", "_Z12k_pnp_decide10DevBuffersi": "k_pnp_decide",
    "_Z11k_pnp_final10DevBuffers": "k_pnp_final", "_Z16k_pnp_final_lean10DevBuffers": "k_pnp_final_lean", "_Z9k_pnp_p3p10DevBuffers": "k_pnp_p3p",
    "_Z19k_inverse_transformPKdS0_Pd": "k_inverse_transform",
}


def source_define(name):
    """the integer a `#define name <integer>` of svo_kernels_pnp.hip gives"""
    txt = open(os.path.join(ROOT, "stereo_visual_odometry_amd", "csrc", "svo_kernels_pnp.hip")).read()
    return int(re.search(r"^#define %s (\d+)\b" % name, txt, re.M).group(1))


@pytest.fixture(scope="module")
def pnp_kernels():
    return {KERNELS[name]: k for name, k in by_name(KERNELS).items()}


def test_all_twelve_kernels_are_built(pnp_kernels):
    missing = sorted(set(KERNELS.values()) - set(pnp_kernels))
    assert not missing, (missing, sorted(pnp_kernels))


@pytest.mark.parametrize("name", ["k_triangulate_lean", "k_pnp_epnp_lean", "k_pnp_final_lean"])
def test_lean_build_fits_beside_four_lk_waves(pnp_kernels, name):
    k = pnp_kernels[name]
    print(name, k)
    assert k["vgpr_count"] <= 96, k
    assert k["agpr_count"] == 0, k


@pytest.mark.parametrize("name", ["k_pnp_epnp", "k_tri_epnp"])
def test_full_epnp_stays_in_registers_with_its_static_arena(pnp_kernels, name):
    k = pnp_kernels[name]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == (64 // source_define("EP_G_LONE")) * source_define("EP_STRIDE") * 8, k


def test_refine_builds_share_their_lds_layout(pnp_kernels):
    full, lean = pnp_kernels["k_pnp_final"], pnp_kernels["k_pnp_final_lean"]
    print(full, lean)
    assert full["group_segment_fixed_size"] == lean["group_segment_fixed_size"] > 0, (full, lean)


@pytest.mark.parametrize("name", ["k_triangulate", "k_pnp_score"])
def test_no_scratch(pnp_kernels, name):
    k = pnp_kernels[name]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
