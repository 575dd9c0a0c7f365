"""The LK kernels as the compiler left them in libsvo_hip.so: register counts and scratch from the code-object metadata, read with the
ROCm llvm-readelf.  No GPU: the device code objects are cut out of the library's fat binary on the host.  Pins the default build's
budget (w = 21 grey, exact sums: at most 80 VGPRs = six waves per SIMD, no scratch) and that the dispatcher's whole table is built."""
import re

import pytest

from code_object import kernels
from code_object import pytestmark  # noqa: F401  (the skip rule: the library and llvm-readelf must exist)


@pytest.fixture(scope="module")
def lk_kernels():
    """{(W, CN, FS): metadata dict} of every k_lk_chain in the library"""
    found = {}
    for name, k in kernels().items():
        m = re.match(r"_Z10k_lk_chainILi(\d+)ELi(\d+)ELb([01])EEv", name)
        if m:
            found[(int(m.group(1)), int(m.group(2)), bool(int(m.group(3))))] = k
    return found


def test_default_build_keeps_six_waves_without_scratch(lk_kernels):
    k = lk_kernels.get((21, 1, False))
    assert k is not None, sorted(lk_kernels)
    print("k_lk_chain<21, 1, false>:", k)
    assert k["vgpr_count"] <= 80, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= 16, k          # the exact-sums build uses no LDS beyond the placeholder array


def test_every_dispatched_window_has_a_kernel(lk_kernels):
    """lk_built() in svo_kernels_lk.hip: grey 5..31 and BGR 5..21, each in both summation modes."""
    want = [(w, 1, fs) for w in range(5, 32) for fs in (False, True)] + [(w, 3, fs) for w in range(5, 22) for fs in (False, True)]
    missing = [k for k in want if k not in lk_kernels]
    assert not missing, missing
    assert len(lk_kernels) == len(want), sorted(set(lk_kernels) - set(want))
