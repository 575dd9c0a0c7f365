"""The track-id kernels (svo_kernels_img.hip) as the compiler left them in libsvo_hip.so, read like test_pose_cov_code_object.py
reads its kernel, and the row's size through ctypes.  k_track_obs is loads and stores: neither build may use scratch, and the lean
build — what a co-resident context launches beside four LK waves of 104 registers — may hold no more than the 96 they leave."""
import ctypes as C

import pytest

from code_object import by_name
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

KERNELS = {
    "_Z11k_track_obs10DevBuffers6IdArgs12TrackObsArgs": "k_track_obs",
    "_Z16k_track_obs_lean10DevBuffers6IdArgs12TrackObsArgs": "k_track_obs_lean",
    "_Z13k_ids_compact10DevBuffers6IdArgs": "k_ids_compact",
    "_Z17k_bucket_emit_ids10DevBuffers6IdArgsi": "k_bucket_emit_ids",
    "_Z25k_bucket_emit_strided_ids10DevBuffers6IdArgsii": "k_bucket_emit_strided_ids",
    "_Z12k_ids_assign10DevBuffers6IdArgs": "k_ids_assign",
    "_Z11k_ids_reset6IdArgsii": "k_ids_reset",
}


@pytest.fixture(scope="module")
def kernels():
    return {KERNELS[name]: k for name, k in by_name(KERNELS).items()}


def test_the_new_kernels_exist(kernels):
    print(kernels)
    assert sorted(kernels) == sorted(KERNELS.values()), sorted(kernels)


@pytest.mark.parametrize("name", ["k_track_obs", "k_track_obs_lean"])
def test_track_obs_uses_no_scratch(kernels, name):
    k = kernels[name]
    print(k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k


def test_lean_build_fits_beside_four_lk_waves(kernels):
    k = kernels["k_track_obs_lean"]
    assert k["vgpr_count"] + k["agpr_count"] <= 96, k


def test_row_is_64_bytes():
    from stereo_visual_odometry_amd import _lib
    assert C.sizeof(_lib.SvoTrackObs) == 64 and _lib.TRACK_OBS_DTYPE.itemsize == 64
    assert [(n, getattr(_lib.SvoTrackObs, n).offset) for n, _ in _lib.SvoTrackObs._fields_] == [
        ("id", 0), ("l0", 8), ("r0", 16), ("l1", 24), ("r1", 32), ("xyz", 40), ("age", 52), ("flags", 56), ("pad", 60)]
    assert all(hasattr(_lib.lib, s) for s in ("svo_set_track_output", "svo_get_last_track_obs", "svo_get_feature_ids"))
