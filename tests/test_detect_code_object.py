"""The detection kernels (FAST tiles, the capacity-1 emit, the general walk and emit) as the compiler left them in libsvo_hip.so,
read like test_img_code_object.py reads the pyramid kernels.  The bodies are shared routines behind thin wrappers
(svo_kernels_img.hip: fast_tile, bucket_walk, bucket_order_emit); the budget of each wrapper is that of the kernel it replaced,
measured before the routines were shared (profiles/r09_detect_code_objects.md): the same LDS, no scratch, no more registers."""

import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

# Itanium-mangled prefix of the kernel symbol -> (readable name, LDS bytes, VGPRs before the routines were shared)
DETECT = {
    "_Z6k_fastILi0EEv": ("k_fast<0>", 5432, 50), "_Z6k_fastILi2EEv": ("k_fast<2>", 5432, 50),
    "_Z14k_fast_strided10DevBuffers": ("k_fast_strided", 5432, 61),
    "_Z16k_fast_score_mapPKh": ("k_fast_score_map", 5432, 50),                    # was k_fast<1>
    "_Z13k_bucket_emit10DevBuffers": ("k_bucket_emit", 52, 30), "_Z21k_bucket_emit_strided10DevBuffers": ("k_bucket_emit_strided", 52, 50),
    "_Z17k_gen_bucket_walk10DevBuffers": ("k_gen_bucket_walk", 0, 31), "_Z17k_gen_bucket_emit10DevBuffers": ("k_gen_bucket_emit", 68, 30),
}


@pytest.fixture(scope="module")
def detect_kernels():
    return by_prefix(DETECT)


def test_every_detection_kernel_is_built(detect_kernels):
    missing = [v[0] for k, v in DETECT.items() if k not in detect_kernels]
    assert not missing, (missing, sorted(detect_kernels))


@pytest.mark.parametrize("sym", sorted(DETECT), ids=lambda s: DETECT[s][0])
def test_detection_kernel_budget(detect_kernels, sym):
    name, lds, vgprs = DETECT[sym]
    k = detect_kernels[sym]
    print(name, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["vgpr_count"] <= vgprs, k
