"""The guard of what tests/test_gpu_batch_wide.py plays (tests/batch_wide_cases.py): the six streams must put their slots into
different states inside one launch, and the schedules must hit the edges of the 64-thread blocks that the one-thread-per-sequence
kernels run in.  The oracle runs here on the CPU; no GPU needed.  Where a stream stops meeting a property, its parameters change —
not the assertion."""
import os
import re

import numpy as np
import pytest

import batch_wide_cases as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_visual_odometry_amd", "csrc")
A, B_, C_, D, E, F = range(6)


@pytest.fixture(scope="module")
def full():
    """The oracle on all eight frames of every stream -> per stream, per frame the statistics."""
    return [[fr[2] for fr in bw.oracle_run(s, range(bw.N_FRAMES))] for s in range(bw.N_STREAMS)]


def test_the_restated_launch_constants_are_the_kernels():
    text = lambda name: open(os.path.join(CSRC, name)).read()
    per_seq = r"\(\(?(launch_seqs\(d\)|ns|n) \+ 63\) / 64\), dim3\(64\)"
    assert bw.BLOCK == 64
    assert len(re.findall(per_seq, text("svo_kernels_img.hip"))) >= 2 and len(re.findall(per_seq, text("svo_kernels_pnp.hip"))) >= 3
    # the first RANSAC chunk of a many-sequence context: 16 hypotheses (test_some_slot_leaves_the_first_ransac_chunk)
    assert re.search(r"pnp_first_chunk\(const DevBuffers& d\) \{ const int c = d\.B <= SVO_LONE_MAX_SEQ \? 32 : 16;", text("svo_internal.hpp"))
    assert int(re.search(r"^#define SVO_RING (\d+)", text("svo_internal.hpp"), re.M).group(1)) > 3      # three frames in flight fit


def test_sizes_put_threads_into_the_second_and_third_block():
    assert bw.SIZES == (65, 130, 256)
    assert bw.SIZES[0] == bw.BLOCK + 1 and bw.SIZES[1] > 2 * bw.BLOCK and -(-bw.SIZES[1] // bw.BLOCK) == 3 and bw.SIZES[2] == 4 * bw.BLOCK
    assert bw.BLOCK % bw.N_STREAMS, "the streams would repeat with the blocks"
    for edge in (64, 128):                                           # different streams on either side of a block edge
        assert bw.stream_of(edge - 1) != bw.stream_of(edge) and bw.stream_of(edge) != bw.stream_of(edge - bw.BLOCK)
    for B in bw.SIZES:
        r = bw.read_slots(B)
        assert {0, B - 1} <= set(r) and all(0 <= i < B for i in r) and len(r) <= 35
        assert all({e - 1, e} <= set(r) for e in (64, 128) if e < B)
        assert {bw.stream_of(i) for i in r} == set(range(bw.N_STREAMS))


def test_streams_are_eight_frames_of_the_context_size():
    for (name, args, black), (L, R) in zip(bw.STREAMS, bw.streams()):
        assert len(L) == len(R) == bw.N_FRAMES
        assert all(a.shape == (bw.H, bw.W) and a.dtype == np.uint8 and a.flags.c_contiguous and not a.flags.writeable for a in L + R)
        for k in range(bw.N_FRAMES):
            assert (not L[k].any() and not R[k].any()) == (k in black), (name, k)
    assert bw.streams() is bw.streams()                             # rendered once


def test_every_fail_reason_of_a_running_context_occurs(full):
    reasons = {st["fail_reason"] for per in full for st in per}
    assert reasons >= {0, 1, 2, 4}, reasons


def test_one_frame_holds_slots_with_and_without_the_second_pass(full):
    assert any({per[k]["second_pass"] for per in full} == {0, 1} for k in range(1, bw.N_FRAMES))


def test_some_frame_has_nothing_to_track(full):
    assert any(per[k]["n_into_lk"] == 0 for per in full for k in range(1, bw.N_FRAMES))
    k = next(k for k in range(1, bw.N_FRAMES) if full[E][k]["n_into_lk"] == 0)
    assert any(per[k]["n_into_lk"] > 100 for per in full), "no slot tracks beside the one that has nothing to track"


def test_some_slot_leaves_the_first_ransac_chunk(full):
    assert any(st["ransac_iters"] > 16 for per in full for st in per)
    # and inside one frame some slots stop in the first chunk while another goes on: pnp_need differs within one k_pnp_decide block
    assert any(max(per[k]["ransac_iters"] for per in full) > 16 and 0 < min(per[k]["ransac_iters"] for per in full if per[k]["ransac_iters"]) <= 16
               for k in range(1, bw.N_FRAMES))


def test_the_plain_scenes_give_a_pose_on_every_frame(full):
    for s in (A, B_):
        assert full[s][0]["fail_reason"] == 1
        assert all(st["fail_reason"] == 0 and st["n_into_lk"] > 100 for st in full[s][1:]), bw.STREAMS[s][0]


def test_the_ragged_schedule_hits_the_block_edges():
    act = bw.ragged_schedule()
    assert act.shape == (bw.N_FRAMES, 130) and act.dtype == bool
    counts = act.sum(1).tolist()
    first = [int(np.argmax(a)) if a.any() else None for a in act]
    assert bw.BLOCK in counts and bw.BLOCK + 1 in counts and 0 in counts and counts.count(130) >= 3
    k65 = counts.index(bw.BLOCK + 1)
    assert first[k65] < bw.BLOCK <= np.flatnonzero(act[k65])[-1], "the 65-entry list does not cross sequence 64"
    k64 = counts.index(bw.BLOCK)
    assert first[k64] >= bw.BLOCK, "the 64-entry list names a sequence below 64"
    assert any(0 < c < bw.BLOCK and np.flatnonzero(a)[-1] >= bw.BLOCK for c, a in zip(counts, act)), "no short list that names a sequence >= 64"
    assert any(c == 1 and first[k] >= bw.BLOCK for k, c in enumerate(counts)), "no single active sequence >= 64"
    assert counts[0] == counts[1] == 130, "the first frames must start every slot"
    assert counts.index(0) < bw.N_FRAMES - 1 and counts[-1] == 130, "nothing follows the all-idle frame"
    # every stream is played under every history, so tier 2 has at least two slots per (stream, history) pair to compare
    pairs, which = bw.distinct_pairs(act)
    assert len({h for s, h in pairs}) == 5 and len(pairs) == 5 * bw.N_STREAMS - (bw.N_STREAMS - 1)       # slot 129's history is its own
    assert sorted(np.bincount(which).tolist())[1] >= 2


def test_the_outputs_schedule_has_twelve_stream_history_pairs():
    act = bw.outputs_schedule()
    pairs, which = bw.distinct_pairs(act)
    assert len(pairs) == 12 and {s for s, h in pairs} == set(range(bw.N_STREAMS)) and {h for s, h in pairs} == {(0, 1, 3), (0, 1, 2, 3)}
    assert act[2].sum() == bw.BLOCK + 1 and not act[2][0] and act[2][bw.BLOCK]
    assert min(np.bincount(which)) >= 5


def test_oracle_results_are_memoised_with_their_prefixes():
    a = bw.oracle_run(C_, (0, 1, 3))
    assert bw.oracle_run(C_, (0, 1, 3))[2] is a[2] and len(bw.oracle_run(C_, (0, 1))) == 2
    b = bw.oracle_run(C_, (0, 1, 2, 3))
    for p in (bw.oracle_run(C_, (0, 1))[1], b[1]):                  # a prefix, whichever run it was kept from, is the same result
        assert p[2] == a[1][2] and np.array_equal(p[1], a[1][1]) and np.array_equal(p[3][0], a[1][3][0])
    assert len(b) == 4 and b[3][2] != a[2][2], "skipping a frame left the statistics unchanged: the histories would not differ"
    idle = bw.idle_stats()
    assert idle["fail_reason"] == 5 and sum(idle.values()) == 5 and set(idle) == set(a[0][2])
