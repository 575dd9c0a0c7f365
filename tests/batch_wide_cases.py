"""What tests/test_gpu_batch_wide.py plays into contexts of 65, 130 and 256 sequences, and what the CPU oracle makes of it: six short
streams, the schedules that say which slot takes which frame, and the oracle's results memoised by (stream, frames taken).  No GPU:
tests/test_batch_wide_cases.py guards on the CPU that the streams and schedules hold what the GPU tests need them for.

Slot i of a context plays stream (i + rot) % 6.  Six does not divide 64, so the slots on either side of a block edge of the
one-thread-per-sequence kernels ((n + 63) / 64 blocks of 64) play different streams.  On frame k an active slot takes frame k of
its stream (an idle slot skips it), so a slot's history is the tuple of frame numbers it took since its last reset.

The streams, and what they are for (tests/test_batch_wide_cases.py asserts the properties, not the figures):
- A, B: plain scenes: hundreds of features into LK and a pose on every frame from the second on.
- C:    large cells: few features, the second detection pass on every frame.
- D:    larger cells still: too few tracks at first (fail_reason 2), then poses from about twenty tracks.
- E:    a scene whose frame 3 is black in both views: reason 2 around it, a frame with nothing to track (n_into_lk = 0), recovery.
- F:    C's scene under an independently moving layer: the motion gate (reason 4), RANSAC past its first chunk of 16 iterations."""
import functools

import numpy as np

import gpu_kit
import oracle_lib as orc

W, H = 320, 160
N_FRAMES = 8
N_STREAMS = 6
OVER = dict(win_w=21, win_h=21, max_level=3, max_translation_norm=2.0, ransac_reprojection_error=0.5)
STREAMS = (                                                          # (name, StereoSequence arguments, frames set to zero)
    ("A", dict(seed=300), ()),
    ("B", dict(seed=331), ()),
    ("C", dict(seed=362, cell_px=70), ()),
    ("D", dict(seed=393, cell_px=110), ()),
    ("E", dict(seed=424), (3,)),
    ("F", dict(seed=362, movers=0.6), ()),
)
BLOCK = 64                                                           # threads of a block of the one-thread-per-sequence kernels
SIZES = (65, 130, 256)                                               # one thread in the second block; a third block; bench.py's context


def calib():
    return gpu_kit.calib(W, H)


def projections():
    return gpu_kit.projections(W, H)


@functools.lru_cache(maxsize=None)
def streams():
    """-> ((lefts, rights), ...) of the six streams; the arrays are shared by every caller and must stay unchanged."""
    from stereo_visual_odometry_amd import synthetic as syn
    out = []
    for name, args, black in STREAMS:
        s = syn.StereoSequence(cal=calib(), n_frames=N_FRAMES, step=0.3, **args)
        L = [np.ascontiguousarray(a) for a in s.left[:N_FRAMES]]; R = [np.ascontiguousarray(a) for a in s.right[:N_FRAMES]]
        for k in black:
            L[k] = np.zeros_like(L[k]); R[k] = np.zeros_like(R[k])
        for a in L + R:
            a.setflags(write=False)
        out.append((tuple(L), tuple(R)))
    return tuple(out)


def stream_of(slot, rot=0):
    return (slot + rot) % N_STREAMS


def read_slots(B):
    """The slots whose features and tracks a GPU test reads back (every slot's row and statistics are checked): the first and last
    six, and both sides of the block edges at 64 and 128."""
    want = list(range(0, 6)) + list(range(58, 71)) + list(range(122, 130)) + list(range(B - 6, B))
    return sorted({i for i in want if 0 <= i < B})


# ------------------------------------------------------------------------------------------------------------------ schedules
def full_schedule(B, n=N_FRAMES):
    return np.ones((n, B), bool)


def slots(lo, hi, B):
    a = np.zeros(B, bool); a[lo:hi + 1] = True
    return a


def ragged_schedule(B=130):
    """f0, f1 all; f2 slots 33..97 (65 entries, crossing index 64); f3 slots 66..129 (64 entries, all >= 64); f4 slot 129 alone;
    f5 none; f6, f7 all."""
    assert B == 130
    act = np.ones((N_FRAMES, B), bool)
    act[2] = slots(33, 97, B); act[3] = slots(66, 129, B); act[4] = slots(129, 129, B); act[5] = False
    return act


def outputs_schedule(B=130):
    """f0, f1 all; f2 slots 33..97; f3 all: two histories per stream."""
    act = np.ones((4, B), bool)
    act[2] = slots(33, 97, B)
    return act


def histories(act, upto=None):
    """act (frames x B) -> per slot the tuple of frame numbers it took in frames 0 .. upto (default: all)."""
    n = len(act) if upto is None else upto + 1
    return [tuple(k for k in range(n) if act[k][i]) for i in range(act.shape[1])]


def distinct_pairs(act, rot=0):
    """The distinct (stream, history) pairs of a schedule, sorted, and for every slot its index among them."""
    hist = histories(act)
    pairs = sorted({(stream_of(i, rot), h) for i, h in enumerate(hist)})
    return pairs, [pairs.index((stream_of(i, rot), h)) for i, h in enumerate(hist)]


# ------------------------------------------------------------------------------------------------------------------ the oracle
_memo = {}


def stats_dict(st):
    return {f[0]: getattr(st, f[0]) for f in st._fields_}


def oracle_run(stream, frames):
    """A fresh oracle_lib.VisualOdometry fed frames `frames` (a tuple of frame numbers) of stream `stream` -> per frame taken
    (ok, T (4, 4), statistics dict, (xy, ages, strengths), tracks dict).  Memoised by (stream, frames) and by every prefix of it;
    the results are shared and must stay unchanged."""
    frames = tuple(frames)
    key = (stream, frames)
    if key not in _memo:
        L, R = streams()[stream]
        Pl, Pr = projections()
        o = orc.VisualOdometry(orc.default_config(**OVER)); o.initalize_projection_matricies(Pl, Pr)
        per = []
        for j, k in enumerate(frames):
            ok, T = o.stereo_callback(L[k], R[k])
            per.append((ok, T.copy(), stats_dict(o.stats), tuple(a.copy() for a in o.features()),
                        {n: a.copy() for n, a in o.last_tracks().items()}))
            _memo.setdefault((stream, frames[:j + 1]), per)          # a prefix's results are the first j + 1 of this list
    return _memo[key][:len(frames)]


def idle_stats():
    """The statistics of an idle slot's row: fail_reason 5, every counter zero."""
    d = {f[0]: 0 for f in orc.OrcFrameStats._fields_}
    d["fail_reason"] = 5
    return d
