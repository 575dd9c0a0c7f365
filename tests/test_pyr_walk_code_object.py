"""The walking pyramid kernels and the row-wise border kernel as the compiler left them in libsvo_hip.so: both forms of
k_pyr_walk exist beside the kernels they stand in for (which every other context, and SVO_PYR_WALK=0, still launch), nothing uses
scratch or spills, and none of them keeps LDS.

Registers.  k_pad_pyramid, which every context runs, fits the 32 per lane the LK kernel's six waves leave, like every image-stream
kernel before.  k_pyr_walk does not: the two running column sums, the row being summed, six source dwords, the edge form's five
selectors and, in the ingest form, the level-0 bytes on their way out come to 47 (levels) and 83 (ingest).  It runs in the gap
between two LK launches of many-sequence contexts only, so what it must keep is enough waves to cover memory latency, and that
gives the bound here: a wave has 64 lanes x 48 bytes of two source rows in flight = 3 KB; 8 TB/s x 2 us of latency is 16 MB for
the device = 64 KB per compute unit = 21 waves = 5 per SIMD with room to spare, and five waves of a 512-register file are
96 registers (the allocation granule is 8)."""
import pytest

from code_object import by_prefix
from code_object import pytestmark  # noqa: F401  (same skip rule: the library and llvm-readelf must exist)

WALK = {"_Z10k_pyr_walkILb1EEv10DevBuffers": "k_pyr_walk<true>", "_Z10k_pyr_walkILb0EEv10DevBuffers": "k_pyr_walk<false>"}
PAD = "_Z13k_pad_pyramid10DevBuffers"
PARENT = {"_Z13k_ingest_pyr1ILi64ELi16ELb0EEv": "k_ingest_pyr1<64, 16, false>", "_Z13k_ingest_pyr1ILi64ELi16ELb1EEv": "k_ingest_pyr1<64, 16, true>",
          "_Z13k_ingest_pyr1ILi32ELi8ELb0EEv": "k_ingest_pyr1<32, 8, false>", "_Z10k_pyrdown210DevBuffers": "k_pyrdown2", "_Z9k_pyrdown10DevBuffers": "k_pyrdown"}
WALK_VGPRS = 96


@pytest.fixture(scope="module")
def kernels():
    return by_prefix(list(WALK) + [PAD] + list(PARENT))


def test_the_new_symbols_exist(kernels):
    assert not [s for s in WALK if s not in kernels], sorted(kernels)


def test_the_parents_symbols_are_still_there(kernels):
    assert not [s for s in list(PARENT) + [PAD] if s not in kernels], sorted(kernels)


@pytest.mark.parametrize("sym", sorted(WALK) + [PAD], ids=lambda s: WALK.get(s, "k_pad_pyramid"))
def test_no_scratch_no_spills_no_lds(kernels, sym):
    k = kernels[sym]
    print(sym, k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k


def test_registers(kernels):
    assert kernels[PAD]["vgpr_count"] <= 32, kernels[PAD]
    for s in WALK:
        assert kernels[s]["vgpr_count"] + kernels[s]["agpr_count"] <= WALK_VGPRS, (WALK[s], kernels[s])
