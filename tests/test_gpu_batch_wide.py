"""Contexts of 65, 130 and 256 sequences, slot by slot, against the CPU oracle (tests/batch_wide_cases.py holds the streams, the
schedules and the oracle's results; tests/test_batch_wide_cases.py guards them on the CPU).

What only a wide context runs: the second and later blocks of the one-thread-per-sequence kernels ((n + 63) / 64 blocks of 64:
k_frame_end, k_frame_begin, k_pick_next, k_reset_seq, k_pnp_subsets, k_pnp_decide, k_pnp_p3p, k_prior_predict, k_ids_reset), the
active list of a ragged frame at its block edges, the per-sequence grids and offsets (seq * CAP, seq * K, the pyramid slots, the
pitches of the pinned rings) at a large sequence number, and one launch that serves slots in different states: slot i plays
stream i % 6, so a second detection pass, a frame with nothing to track, too few tracks, the motion gate and a RANSAC that leaves
its first chunk sit next to plain frames, on both sides of every block edge.

Three references:
- tier 1, the oracle: oracle_lib.VisualOdometry fed exactly the frames a slot took (a fresh one after a reset).  Per slot and frame
  taken: ok and every statistics field equal, the pose within test_gpu_parity's POSE_TOL_T / POSE_TOL_R; where the state is read
  back, the feature set (xy bits, ages, strengths) and the tracks pl0 pr0 pl1 pr1 bit-equal.  An idle slot's row is ok = 0,
  fail_reason 5, zero counters and its last transform bit for bit, and its state is untouched.
- tier 2, slot identity: slots with the same stream and history agree bit for bit in T (as uint64), ok, the statistics and
  gpu_kit.snap — contamination between slots that stays below the pose tolerance shows here.
- tier 3, B-invariance of the optional outputs: a wide context gives, slot for slot, the bits of a 12-sequence context that runs
  the 12 distinct (stream, history) pairs with the same settings; the existing suites pin those outputs to their CPU references
  at about that size.

Rows, statistics and tier 2 cover every slot; features and tracks are read back for bw.read_slots(B) only (the first and last six
slots and both sides of the block edges at 64 and 128): a read synchronises and copies, and reading every slot on every frame
would cost more than the frames."""
import numpy as np
import pytest

import batch_wide_cases as bw
from gpu_kit import api, f32_bits as bits, raw_bits, same, snap  # noqa: F401  (the fixture is found by name)
from test_gpu_parity import POSE_TOL_R, POSE_TOL_T, rot_angle

pytestmark = pytest.mark.gpu

W, H, N = bw.W, bw.H, bw.N_FRAMES


def context(api, B):
    vo = api.BatchVisualOdometry(W, H, B, api.default_config(**bw.OVER))
    vo.initalize_projection_matricies(*bw.projections())
    return vo


def rows_of(vo, ok, T):
    return [(bool(ok[i]), T[i].reshape(16).copy(), vo.stats[i].as_dict()) for i in range(vo.n_seq)]


def snaps_of(vo, B):
    return {i: snap(vo, i) for i in bw.read_slots(B)}


def host_frame(vo, which, k, a):
    """Frame k of its stream for every slot with a[i] set, through the host-image entry point -> rows."""
    S = bw.streams()
    L = [S[which[i]][0][k] if a[i] else None for i in range(vo.n_seq)]
    R = [S[which[i]][1][k] if a[i] else None for i in range(vo.n_seq)]
    ok, T = vo.stereo_callback_batch(L, R, active=None if a.all() else a)
    return rows_of(vo, ok, T)


def assert_row(r, want, where):
    """tier 1 for a result row: `want` is one frame of bw.oracle_run (or any (ok, T (4, 4), statistics, ...))."""
    ok, T, st = r
    assert ok == want[0] and st == want[2], (where, ok, st, want[0], want[2])
    T = T.reshape(4, 4)
    assert np.abs(T[:3, 3] - want[1][:3, 3]).max() < POSE_TOL_T and rot_angle(T[:3, :3], want[1][:3, :3]) < POSE_TOL_R, (where, "pose", T, want[1])


def assert_state(s, want, first, where):
    """tier 1 for a gpu_kit.snap: the feature set, and from a sequence's second frame on the tracks, against the oracle's bits."""
    f, t = want[3], want[4]
    assert np.array_equal(s[0], bits(f[0])) and np.array_equal(s[1], f[1]) and np.array_equal(s[2], f[2]), (where, "feature set")
    if not first:
        for j, key in enumerate(("pl0", "pr0", "pl1", "pr1")):
            assert np.array_equal(s[3 + j], bits(t[key])), (where, key)


class Book:
    """Per slot: the stream it plays, the frames it took since its last reset, its last row's T.  frame() checks one collected frame
    of a context against tiers 1 and 2."""

    def __init__(self, which, what):
        self.which, self.what, self.B = list(which), what, len(which)
        self.taken = [() for _ in which]
        self.last_T = [np.eye(4).reshape(16) for _ in which]
        self.last_snap = {}

    def reset(self, i=-1):
        for j in (range(self.B) if i < 0 else (i,)):
            self.taken[j] = ()

    def take(self, k, a):
        for i in range(self.B):
            if a[i]:
                self.taken[i] += (k,)

    def frame(self, k, a, rows, snaps=None):
        """The context has collected frame k, taken by the slots with a[i] set; take(k, a) has been called for it."""
        where = lambda i: (self.what, "frame", k, "slot", i, "stream", bw.STREAMS[self.which[i]][0], "took", self.taken[i])
        for i in range(self.B):
            if a[i]:
                want = bw.oracle_run(self.which[i], self.taken[i])[-1]
                assert_row(rows[i], want, where(i))
                if snaps is not None and i in snaps:
                    assert_state(snaps[i], want, len(self.taken[i]) == 1, where(i))
            else:
                ok, T, st = rows[i]
                assert not ok and st == bw.idle_stats(), (where(i), "idle row", ok, st)
                assert np.array_equal(T.view(np.uint64), self.last_T[i].view(np.uint64)), (where(i), "idle row's transform")
                if snaps is not None and i in snaps and i in self.last_snap:
                    assert same(snaps[i], self.last_snap[i]), (where(i), "an idle frame changed the slot's state")
            self.last_T[i] = rows[i][1]
        if snaps is not None:
            self.last_snap = dict(snaps)
        self.identity(rows, snaps, a, where)

    def identity(self, rows, snaps, a, where):
        """tier 2: slots of equal stream and history agree in every bit."""
        lead, lead_snap = {}, {}
        for i in range(self.B):
            key = (self.which[i], self.taken[i], bool(a[i]))
            j = lead.setdefault(key, i)
            if j != i:
                assert rows[i][0] == rows[j][0] and rows[i][2] == rows[j][2], (where(i), "differs from slot", j, rows[i][2], rows[j][2])
                assert np.array_equal(rows[i][1].view(np.uint64), rows[j][1].view(np.uint64)), (where(i), "T differs from slot", j, rows[i][1], rows[j][1])
            if snaps is not None and i in snaps:
                j = lead_snap.setdefault(key, i)
                assert j == i or same(snaps[i], snaps[j]), (where(i), "state differs from slot", j)


def play_host(vo, book, act, frames=None, path=0):
    """Host images, one synchronous call per frame, the state of bw.read_slots read back after every frame."""
    for n, k in enumerate(frames if frames is not None else range(len(act))):
        a = act[n]
        book.take(k, a)
        rows = host_frame(vo, book.which, k, a)
        if path and a.any():
            assert vo.last_frame_path() & path == path, (book.what, k, vo.last_frame_path())
        book.frame(k, a, rows, snaps_of(vo, vo.n_seq))


# ------------------------------------------------------------------------------------------------------------ 1. full frames
@pytest.mark.parametrize("B", bw.SIZES)
def test_full_frames(api, B):
    """Every slot on every one of the eight frames, host images: tiers 1 and 2; the frames take the build-ahead path."""
    vo = context(api, B)
    try:
        book = Book([bw.stream_of(i) for i in range(B)], "B = %d" % B)
        play_host(vo, book, bw.full_schedule(B), path=api._lib.PATH_INGEST_AHEAD)
        assert all(len(t) == N for t in book.taken)
    finally:
        vo.close()


# ------------------------------------------------------------------------------------------------- 2. device frames in flight
def test_device_frames_three_in_flight(api):
    """B = 130, frames resident on the device with rows 3 bytes wider than the image (the bytes beyond a row hold 0xA5), three
    frames in flight; features and tracks after the last collect only."""
    import torch
    B, stride = 130, W + 3
    dev = []
    for L, R in bw.streams():
        per = []
        for k in range(N):
            pair = []
            for img in (L[k], R[k]):
                buf = np.full((H, stride), 0xA5, np.uint8); buf[:, :W] = img
                pair.append(torch.from_numpy(buf).cuda())
            per.append(pair)
        dev.append(per)
    torch.cuda.synchronize()
    vo = context(api, B)
    try:
        book = Book([bw.stream_of(i) for i in range(B)], "device frames")
        ones = np.ones(B, bool)
        submit = lambda k: vo.submit_device([dev[s][k][0].data_ptr() for s in book.which], [dev[s][k][1].data_ptr() for s in book.which], stride)
        for k in range(3):
            submit(k)
        kept = []
        for k in range(N):
            ok, T = vo.collect()
            kept.append(rows_of(vo, ok, T))
            if k + 3 < N:
                submit(k + 3)
        snaps = snaps_of(vo, B)
        for k in range(N):
            book.take(k, ones)
            book.frame(k, ones, kept[k], snaps if k == N - 1 else None)
    finally:
        vo.close()


# ----------------------------------------------------------------------------------------------------------- 3. ragged frames
def test_ragged_frames_at_the_block_edges(api):
    """B = 130, host images, active lists of 65 entries across sequence 64, of 64 entries all >= 64, of slot 129 alone, of none:
    tier 1 per slot on the frames it took, idle rows and untouched idle state, tier 2 among slots of equal stream and history."""
    B = 130
    act = bw.ragged_schedule(B)
    vo = context(api, B)
    try:
        book = Book([bw.stream_of(i) for i in range(B)], "ragged")
        play_host(vo, book, act, path=api._lib.PATH_INGEST_AHEAD)
        assert book.taken == bw.histories(act)
        assert vo.last_frame_path() != 0
    finally:
        vo.close()


# ------------------------------------------------------------------------------------------------------------------ 4. resets
def test_reset_of_every_sequence(api):
    """B = 130: three frames, reset_sequence(-1) (k_reset_seq with seq = -1: one thread per sequence), three more frames — the
    second three are a fresh context's first three (the oracle is a fresh object fed frames 3, 4, 5)."""
    B = 130
    vo = context(api, B)
    try:
        book = Book([bw.stream_of(i) for i in range(B)], "reset all")
        play_host(vo, book, bw.full_schedule(B, 3), frames=(0, 1, 2))
        vo.reset_sequence()
        book.reset()
        play_host(vo, book, bw.full_schedule(B, 3), frames=(3, 4, 5))
        assert all(t == (3, 4, 5) for t in book.taken)
    finally:
        vo.close()


def test_reset_of_single_sequences_at_the_block_edges(api):
    """B = 130: three frames, slots 63, 64 and 129 reset one call each, three more frames: the reset slots restart (their first frame
    fails with reason 1), their neighbours 62, 65 and 128 — every other slot — continue."""
    B = 130
    vo = context(api, B)
    try:
        book = Book([bw.stream_of(i) for i in range(B)], "reset 63, 64, 129")
        play_host(vo, book, bw.full_schedule(B, 3), frames=(0, 1, 2))
        for i in (63, 64, 129):
            vo.reset_sequence(i)
            book.reset(i)
        play_host(vo, book, bw.full_schedule(B, 3), frames=(3, 4, 5))
        for i in range(B):
            assert book.taken[i] == ((3, 4, 5) if i in (63, 64, 129) else (0, 1, 2, 3, 4, 5)), i
        assert all(bw.oracle_run(bw.stream_of(i), (3,))[0][2]["fail_reason"] == 1 for i in (63, 64, 129))
    finally:
        vo.close()


# -------------------------------------------------------------------------------------------------- 5. optional outputs together
def run_with_outputs(api, which, act, what):
    """A context of len(which) sequences with the pose covariance, the observation rows, the descriptors and the predicted motion prior
    all on, over the schedule `act` -> per frame, per slot a dict of everything the frame returned, as bits."""
    B = len(which)
    lb = api._lib
    vo = context(api, B)
    try:
        vo.set_pose_covariance("residual")
        vo.set_track_output(256)
        vo.set_descriptor_output(True)
        vo.set_motion_prior_mode("last_rotation")
        out = []
        for k in range(len(act)):
            rows = host_frame(vo, which, k, act[k])
            path = vo.last_frame_path()
            assert not path & (lb.PATH_LEAN | lb.PATH_LK_CHAINED), (what, k, path)       # the full builds, unchained: what the other context ran
            want = lb.PATH_INGEST_AHEAD | lb.PATH_POSE_COV | lb.PATH_TRACK_IDS | lb.PATH_DESCRIPTORS | lb.PATH_PRIOR_PREDICTED | lb.PATH_MOTION_PRIOR
            assert path & want == want, (what, k, path)
            cov_T, cov_p, valid = vo.last_pose_covariance()
            per = []
            for i in range(B):
                obs, n_tracks = vo.last_track_obs(i, with_count=True)
                pr = vo.last_motion_prior(i)
                per.append(dict(row=rows[i], cov_T=cov_T[i].view(np.uint64).copy(), cov_p=cov_p[i].view(np.uint64).copy(), valid=bool(valid[i]),
                                obs=obs.tobytes(), ids=obs["id"].copy(), n_rows=len(obs), n_tracks=n_tracks, desc=vo.last_track_descriptors(i),
                                prior=None if pr is None else (raw_bits(pr[0]), raw_bits(pr[1]), pr[2])))
            for i in bw.read_slots(B):
                per[i]["snap"] = snap(vo, i); per[i]["feature_ids"] = vo.feature_ids(i)
            out.append(per)
        return out
    finally:
        vo.close()


def test_optional_outputs_are_the_narrow_context_s(api):
    """B = 130 with the covariance, the observation rows (256 per sequence: the plain scenes overflow them), the descriptors and the
    predicted prior on at once; f0, f1 all, f2 slots 33..97, f3 all.  The reference here — for the poses and statistics too — is a
    12-sequence context that runs the 12 distinct (stream, history) pairs with the same settings, NOT the oracle: the predicted
    prior seeds LK and so may change what is tracked, and the oracle has no prior.  The two contexts run one after the other (the
    first is closed before the second exists), so both run the unchained full builds.  Tier 3: every optional output of a wide slot
    equals the narrow slot's, bit for bit; tier 1 (ok, statistics, pose tolerance) against the narrow slot; tier 2 inside the wide
    context; idle slots have zero rows."""
    B = 130
    act = bw.outputs_schedule(B)
    pairs, slot_pair = bw.distinct_pairs(act)
    assert len(pairs) == 12
    narrow_act = np.array([[k in h for s, h in pairs] for k in range(len(act))])
    narrow = run_with_outputs(api, [s for s, h in pairs], narrow_act, "narrow")
    wide = run_with_outputs(api, [bw.stream_of(i) for i in range(B)], act, "wide")
    book = Book([bw.stream_of(i) for i in range(B)], "outputs")
    seen = dict(valid=0, overflow=0, fits=0, predicted=0, desc=0)
    for k in range(len(act)):
        book.take(k, act[k])
        for i in range(B):
            g, w = wide[k][i], narrow[k][slot_pair[i]]
            where = ("frame", k, "slot", i, "narrow slot", slot_pair[i], "stream", bw.STREAMS[book.which[i]][0])
            if act[k][i]:
                assert_row(g["row"], (w["row"][0], w["row"][1].reshape(4, 4), w["row"][2]), where)
            else:
                assert not g["row"][0] and g["row"][2] == bw.idle_stats() and np.array_equal(g["row"][1].view(np.uint64), book.last_T[i].view(np.uint64)), (where, "idle row")
                assert not g["valid"] and not g["cov_T"].any() and not g["cov_p"].any(), (where, "idle covariance")
                assert g["n_tracks"] == 0 and g["n_rows"] == 0 and len(g["desc"]) == 0 and g["prior"] is None, (where, "idle rows")
            book.last_T[i] = g["row"][1]
            assert g["valid"] == w["valid"] and np.array_equal(g["cov_T"], w["cov_T"]) and np.array_equal(g["cov_p"], w["cov_p"]), (where, "covariance")
            assert g["n_tracks"] == w["n_tracks"] and g["n_rows"] == w["n_rows"] == min(g["n_tracks"], 256), (where, "row counts", g["n_tracks"], g["n_rows"], w["n_tracks"], w["n_rows"])
            assert np.array_equal(g["ids"], w["ids"]), (where, "ids")
            assert g["obs"] == w["obs"], (where, "observation rows")
            assert g["desc"].shape == w["desc"].shape == (g["n_rows"], 32) and np.array_equal(g["desc"], w["desc"]), (where, "descriptors")
            assert (g["prior"] is None) == (w["prior"] is None), (where, "prior")
            if g["prior"] is not None:
                assert g["prior"][2] == w["prior"][2] and np.array_equal(g["prior"][0], w["prior"][0]) and np.array_equal(g["prior"][1], w["prior"][1]), (where, "prior")
            if "snap" in g and "snap" in w:
                assert same(g["snap"], w["snap"]) and np.array_equal(g["feature_ids"], w["feature_ids"]), (where, "state / feature ids")
            seen["valid"] += g["valid"]; seen["overflow"] += g["n_tracks"] > 256; seen["fits"] += 0 < g["n_tracks"] <= 256
            seen["predicted"] += g["prior"] is not None and g["prior"][2] == 2; seen["desc"] += bool(g["desc"].any())
        book.identity([g["row"] for g in wide[k]], {i: wide[k][i]["snap"] for i in bw.read_slots(B)}, act[k],
                      lambda i: ("outputs", "frame", k, "slot", i))
    assert all(seen.values()), seen                                   # the comparison was not vacuous


# ------------------------------------------------------------------------------------------------ 6. two contexts of 256
def test_two_contexts_of_256_sharing_the_device(api):
    """bench.py's arrangement: two contexts of 256 sequences alive together, their calls interleaved for four frames, the second
    playing the streams rotated by one.  Tier 1 (and 2) per slot of both; both chain their LK launches from the second frame on."""
    B = 256
    ctx = [context(api, B), context(api, B)]
    try:
        books = [Book([bw.stream_of(i, c) for i in range(B)], "context %d of two" % c) for c in range(2)]
        ones = np.ones(B, bool)
        for k in range(4):
            for vo, book in zip(ctx, books):
                book.take(k, ones)
                rows = host_frame(vo, book.which, k, ones)
                path = vo.last_frame_path()
                if k >= 1:
                    assert path & api._lib.PATH_LK_CHAINED, (book.what, k, path)
                book.frame(k, ones, rows, snaps_of(vo, B))
    finally:
        for vo in ctx:
            vo.close()
