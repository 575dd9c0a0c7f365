"""The motion-prior LK kernels as the compiler left them in libsvo_hip.so (no GPU: tests/code_object.py reads the metadata).  A frame
with a prior launches k_lk_chain_prior<W> in k_lk_chain<W, 1, false>'s place, so the default build's budget is pinned for it too
(w = 21: at most 80 VGPRs = six waves per SIMD, no scratch, no LDS), and every window the dispatcher can ask for must be built."""
import re

import pytest

from code_object import kernels
from code_object import pytestmark  # noqa: F401  (the skip rule: the library and llvm-readelf must exist)


def found(pattern):
    out = {}
    for name, k in kernels().items():
        m = re.match(pattern, name)
        if m:
            out[int(m.group(1))] = k
    return out


@pytest.fixture(scope="module")
def chain_prior():
    return found(r"_Z16k_lk_chain_priorILi(\d+)EEv")


def test_every_window_has_a_prior_kernel(chain_prior):
    assert sorted(chain_prior) == list(range(5, 32)), sorted(chain_prior)
    assert sorted(found(r"_Z17k_lk_single_guessILi(\d+)EEv")) == list(range(5, 32))


def test_default_build_keeps_six_waves_without_scratch(chain_prior):
    k = chain_prior[21]
    print("k_lk_chain_prior<21>:", k)
    assert k["vgpr_count"] <= 80, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] <= 16, k


def test_the_prior_costs_no_wave(chain_prior):
    """the guess is dead before the Newton loop: no window's prior build needs a larger register block than its k_lk_chain"""
    base = found(r"_Z10k_lk_chainILi(\d+)ELi1ELb0EEv")
    worse = {w: (base[w]["vgpr_count"], chain_prior[w]["vgpr_count"]) for w in chain_prior
             if 512 // ((chain_prior[w]["vgpr_count"] + 7) // 8 * 8) < 512 // ((base[w]["vgpr_count"] + 7) // 8 * 8)}
    assert not worse, worse
