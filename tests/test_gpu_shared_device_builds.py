"""The 96-register builds of triangulation / EPnP / refine (`k_triangulate_lean`, `k_pnp_epnp_lean`, `k_pnp_final_lean`) at the
operating points that reach them in production: two contexts of more than 8 sequences on one device, with an LK build that leaves
>= 96 registers free (svo_get_lk_registers_left).  The configurations are picked on the device, every frame is held to the
oracle, and svo_get_last_frame_path proves which builds each frame took.  The lean builds promise the full builds' bits
(svo.h), so a context whose neighbour comes and goes must equal the same context run alone.  The forced-lean knob
(SVO_FORCE_LEAN=1) runs a fixed selection of the parity suite through the lean builds in a child process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
from gpu_kit import api, calib, raw_bits as bits, run_child  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POSE_TOL_T = 1e-6                       # as test_gpu_parity.py
POSE_TOL_R = 1e-6
W, H, B = 480, 200, 10                  # B > 8: a many-sequence context
LEAN_ROOM = 96                          # device_sharing() in svo_api.hip

# (window, channels, lk_float_sums): the builds whose LK leaves >= 96 registers by the compiler's counts
# (profiles/r04_lk_vgprs.md), plus the metric's window, which must not
CANDIDATES = [(22, 1, 0), (31, 1, 1), (17, 1, 1), (23, 1, 1), (10, 3, 1), (12, 3, 1), (21, 1, 0), (31, 1, 0), (21, 3, 0)]


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)))


def probe(api):
    """svo_get_lk_registers_left of every candidate build -> {(win, cn, fs): registers left}"""
    out = {}
    for win, cn, fs in CANDIDATES:
        vo = api.BatchVisualOdometry(W, H, 1, api.default_config(win_w=win, win_h=win, channels=cn, lk_float_sums=fs))
        out[(win, cn, fs)] = vo.lk_registers_left()
        vo.close()
    return out


@pytest.fixture(scope="module")
def lean_builds(api):
    room = probe(api)
    grey = [k for k, v in room.items() if k[1] == 1 and v >= LEAN_ROOM]
    bgr = [k for k, v in room.items() if k[1] == 3 and v >= LEAN_ROOM]
    assert grey, "no single-channel LK build leaves %d registers free (%s): the 96-register builds can no longer be reached " \
                 "in production — retire them or re-pick the builds" % (LEAN_ROOM, room)
    return dict(room=room, grey=grey[0], bgr=bgr[0] if bgr else None)


def test_lean_regime_is_reachable_in_production(api, lean_builds):
    """At least one single-channel build (and a 3-channel one, where any qualifies) leaves >= 96 registers; the metric's w = 21
    grey build does not (test_lk_kernel_register_budget pins its 32)."""
    room = lean_builds["room"]
    assert room[(21, 1, 0)] < LEAN_ROOM, room
    assert lean_builds["grey"] is not None
    print("lean-regime probe:", {"w%d c%d fs%d" % k: v for k, v in room.items()})


def over_for(build, **extra):
    win, cn, fs = build
    # a 1 px RANSAC threshold: with the mover layer RANSAC runs past the first chunk of 16 hypotheses
    return dict(dict(win_w=win, win_h=win, lk_float_sums=fs, channels=cn, max_translation_norm=2.0, ransac_reprojection_error=1.0), **extra)


def bgr(a):
    return np.ascontiguousarray(np.stack([a, np.roll(a, 1, 0), 255 - a], -1))


def make_streams(n_frames, cn, seeds=(70, 71, 72), movers=(0.0, 0.3, 0.3), black=2):
    """Three rendered streams; the third starts with `black` black frames (second FAST pass, empty sets, failure paths)."""
    from stereo_visual_odometry_amd import synthetic as syn
    out = []
    for s, (seed, mv) in enumerate(zip(seeds, movers)):
        sq = syn.StereoSequence(cal=calib(W, H), n_frames=n_frames, seed=seed, step=0.3, movers=mv)
        L, R = list(sq.left), list(sq.right)
        if s == 2 and black:
            z = np.zeros_like(L[0])
            L, R = [z] * black + L[:n_frames - black], [z] * black + R[:n_frames - black]
        if cn == 3:
            L, R = [bgr(a) for a in L], [bgr(a) for a in R]
        out.append((L, R))
    return out


def oracle_runs(streams, over, n_frames):
    from stereo_visual_odometry_amd import synthetic as syn
    Pl, Pr = syn.projection_matrices(calib(W, H))
    want = []
    for L, R in streams:
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        per = []
        for k in range(n_frames):
            ok, T = o.stereo_callback(L[k], R[k])
            st = {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}
            per.append((ok, T.copy(), st, [a.copy() for a in o.features()], o.last_tracks() if k else None))
        want.append(per)
    return want


class Ctx:
    """A B-sequence context whose slot i replays stream pick(i); frames from device-resident images."""

    def __init__(self, api, over, streams, pick):
        import torch
        from stereo_visual_odometry_amd import synthetic as syn
        self.vo = api.BatchVisualOdometry(W, H, B, api.default_config(**over))
        self.vo.initalize_projection_matricies(*syn.projection_matrices(calib(W, H)))
        self.pick, self.cn = pick, over.get("channels", 1)
        self.dev = [[(torch.from_numpy(np.ascontiguousarray(l)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda())
                     for l, r in zip(L, R)] for L, R in streams]
        torch.cuda.synchronize()

    def submit(self, k, active=None):
        a = [True] * B if active is None else active
        self.vo.submit_device([self.dev[self.pick(i)][k][0].data_ptr() if a[i] else None for i in range(B)],
                              [self.dev[self.pick(i)][k][1].data_ptr() if a[i] else None for i in range(B)], W * self.cn,
                              active=active)
        return self.vo.last_frame_path()

    def snap(self, i):
        f = self.vo.features(i); t = self.vo.last_tracks(i)
        return [bits(f[0]), f[1], f[2]] + [bits(t[k]) for k in ("pl0", "pr0", "pl1", "pr1", "world")] + [t["inlier"]]

    def close(self):
        self.vo.close()


def check_against_oracle(ctx, ok, T, want, k, tag):
    """run_both's bar (test_gpu_parity.py) for every sequence of a context."""
    vo = ctx.vo
    for i in range(B):
        ok_o, T_o, so, fo, to = want[ctx.pick(i)][k]
        sg = vo.stats[i].as_dict()
        assert bool(ok[i]) == ok_o and sg == so, (tag, k, i, sg, so)
        fg = vo.features(i)
        assert np.array_equal(bits(fg[0]), bits(fo[0])) and np.array_equal(fg[1], fo[1]) and np.array_equal(fg[2], fo[2]), (tag, k, i)
        if k > 0:
            tg = vo.last_tracks(i)
            for key in ("pl0", "pr0", "pl1", "pr1"):
                assert np.array_equal(bits(to[key]), bits(tg[key])), (tag, k, i, key)
            if so["fail_reason"] in (0, 3, 4) and so["n_after_bounds"] > 15:
                assert np.array_equal(bits(to["world"]), bits(tg["world"])), (tag, k, i)
                assert np.array_equal(to["inlier"], tg["inlier"]), (tag, k, i)
        assert np.abs(T[i][:3, 3] - T_o[:3, 3]).max() < POSE_TOL_T, (tag, k, i)
        assert rot_angle(T[i][:3, :3], T_o[:3, :3]) < POSE_TOL_R, (tag, k, i)


LEAN_SHARED = 1 | 2                     # SVO_PATH_LEAN | SVO_PATH_LK_CHAINED


def run_shared_pair(api, over, streams, n_frames):
    """Two many-sequence contexts, frames submitted interleaved (both in flight before either is collected); every sequence of
    both against the oracle on every frame, every frame on the lean builds with chained LK launches."""
    want = oracle_runs(streams, over, n_frames)
    ctx = [Ctx(api, over, streams, lambda i: i % 3), Ctx(api, over, streams, lambda i: (i + 2) % 3)]
    stats = []
    try:
        for k in range(n_frames):
            paths = [c.submit(k) for c in ctx]
            outs = [c.vo.collect() for c in ctx]
            for c, (ok, T), p in zip(ctx, outs, paths):
                assert p & LEAN_SHARED == LEAN_SHARED, (k, p)
                check_against_oracle(c, ok, T, want, k, "shared")
                stats += [s.as_dict() for s in c.vo.stats]
    finally:
        for c in ctx:
            c.close()
    return stats


@pytest.mark.parametrize("case", ["movers", "ransac1000", "bgr"])
def test_two_lean_contexts_match_the_oracle(api, lean_builds, case):
    """Movers make RANSAC iterate past the first chunk of 16 hypotheses, so the second k_pnp_epnp_lean launch (h0 > 0) decides
    frames; black frames spliced into one stream take the failure paths; 1000 iterations in one case."""
    if case == "bgr":
        build = lean_builds["bgr"]
        if build is None:                    # the probe asserted what exists; nothing 3-channel reaches the regime
            build = lean_builds["grey"]
    else:
        build = lean_builds["grey"]
    over = over_for(build, ransac_iterations=1000) if case == "ransac1000" else over_for(build)
    n = 5
    stats = run_shared_pair(api, over, make_streams(n, build[1]), n)
    assert max(s["ransac_iters"] for s in stats) > 16, "RANSAC never left the first chunk: the second lean EPnP launch was not tested"
    reasons = {s["fail_reason"] for s in stats}
    assert 0 in reasons and (1 in reasons or 2 in reasons), reasons
    assert any(s["n_after_bounds"] > 256 for s in stats), "no refine over more than 256 tracks: the lean block's second pass was idle"


def test_two_lean_contexts_direct_five_point_branch(api, lean_builds):
    """features_threshold = 0, max_features = 5: frames reach PnP with exactly five tracks, the direct branch (hend = 1) of the
    8-lane EPnP."""
    over = over_for(lean_builds["grey"], features_threshold=0, max_features=5, max_translation_norm=5.0, max_rotation_norm=3.0)
    stats = run_shared_pair(api, over, make_streams(4, 1, black=0), 4)
    assert any(s["n_after_bounds"] == 5 and s["n_inliers"] == 5 for s in stats)


def come_and_go(api, over, streams, n_frames, neighbour_at=(2, 5)):
    """Context A runs n_frames; context N (the neighbour) exists from before frame neighbour_at[0] to after frame neighbour_at[1]
    and processes frames of its own meanwhile.  -> per frame (ok, T, stats, snapshots, path) of A."""
    a = Ctx(api, over, streams, lambda i: i % 3)
    nb = None
    out = []
    try:
        for k in range(n_frames):
            if k == neighbour_at[0]:
                nb = Ctx(api, over, streams, lambda i: (i + 1) % 3)
            p = a.submit(k)
            if nb is not None:
                nb.submit(k)
                nb.vo.collect()
            ok, T = a.vo.collect()
            out.append((ok.copy(), T.copy(), [s.as_dict() for s in a.vo.stats], [a.snap(i) for i in range(B)], p))
            if k == neighbour_at[1]:
                nb.close(); nb = None
    finally:
        a.close()
        if nb is not None:
            nb.close()
    return out


def same_frames(x, y):
    for k, (a, b) in enumerate(zip(x, y)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k          # poses: identical bits
        assert a[2] == b[2], k
        for sa, sb in zip(a[3], b[3]):
            assert all(np.array_equal(u, v) for u, v in zip(sa, sb)), k


def alone(api, over, streams, n_frames):
    return come_and_go(api, over, streams, n_frames, neighbour_at=(-1, -1))


def test_neighbour_comes_and_goes(api, lean_builds):
    """A runs full -> lean -> full as its neighbour is created before frame 2 and destroyed after frame 5: every frame of A meets
    the oracle, the path bits follow the regime, and A equals A run alone bit for bit (svo.h: results identical either way)."""
    over = over_for(lean_builds["grey"])
    n = 8
    streams = make_streams(n, 1)
    want = oracle_runs(streams, over, n)
    got = come_and_go(api, over, streams, n)
    ref = alone(api, over, streams, n)
    for k, r in enumerate(got):
        shared = 2 <= k <= 5
        assert (r[4] & LEAN_SHARED) == (LEAN_SHARED if shared else 0), (k, r[4])
        assert ref[k][4] & LEAN_SHARED == 0, (k, ref[k][4])
        for i in range(B):                                    # the snapshots taken at the time against the oracle

            ok_o, T_o, so, fo, to = want[i % 3][k]
            assert bool(r[0][i]) == ok_o and r[2][i] == so, (k, i, r[2][i], so)
            sn = r[3][i]
            assert np.array_equal(sn[0], bits(fo[0])) and np.array_equal(sn[1], fo[1]) and np.array_equal(sn[2], fo[2]), (k, i)
            if k > 0:
                for j, key in enumerate(("pl0", "pr0", "pl1", "pr1")):
                    assert np.array_equal(sn[3 + j], bits(to[key])), (k, i, key)
                if so["fail_reason"] in (0, 3, 4) and so["n_after_bounds"] > 15:
                    assert np.array_equal(sn[7], bits(to["world"])) and np.array_equal(sn[8], to["inlier"]), (k, i)
            assert np.abs(r[1][i][:3, 3] - T_o[:3, 3]).max() < POSE_TOL_T and rot_angle(r[1][i][:3, :3], T_o[:3, :3]) < POSE_TOL_R
    same_frames(got, ref)
    assert any(s["n_after_bounds"] > 256 for r in got[2:6] for s in r[2]), "the lean refine never summed more than 256 tracks"


def test_neighbour_comes_and_goes_graph_mode(api, lean_builds, monkeypatch):
    """The same with SVO_GRAPH=1: A's captured graphs must be re-captured when the regime flips (g_co), so the replayed frames
    carry the lean bit exactly while the neighbour exists, and the results equal the launch-list run."""
    over = over_for(lean_builds["grey"])
    n = 8
    streams = make_streams(n, 1)
    monkeypatch.setenv("SVO_GRAPH", "0")
    listed = come_and_go(api, over, streams, n)
    monkeypatch.setenv("SVO_GRAPH", "1")
    graphed = come_and_go(api, over, streams, n)
    monkeypatch.delenv("SVO_GRAPH")
    for k, r in enumerate(graphed):
        assert r[4] & 32, (k, r[4])                              # SVO_PATH_GRAPH: the frame was replayed
        assert bool(r[4] & 1) == (2 <= k <= 5), (k, r[4])        # SVO_PATH_LEAN of the capture
    same_frames(graphed, listed)


def test_ragged_frames_under_lean_builds(api, lean_builds):
    """Idle masks in the lean regime (test_idle_invariance_bit_exact's pattern): sequence i's j-th active frame equals frame j of
    an unmasked run beside the same neighbour, bit for bit; idle rows keep their last pose with fail_reason 5."""
    over = over_for(lean_builds["grey"])
    steps = 8
    streams = make_streams(steps, 1)
    rng = np.random.default_rng(5)
    act = rng.random((steps, B)) < 0.65
    act[1] = True
    nb = Ctx(api, over, streams, lambda i: (i + 1) % 3)
    try:
        def run(mask):
            c = Ctx(api, over, streams, lambda i: i % 3)
            nxt = [0] * B
            got = [[] for _ in range(B)]
            last_T = [np.eye(4) for _ in range(B)]
            try:
                for k in range(steps):
                    a = np.ones(B, bool) if mask is None else mask[k]
                    nb.submit(k); nb.vo.collect()
                    # every sequence replays its own stream at its own pace: build the frame from per-sequence indices
                    idx = [nxt[i] if a[i] else None for i in range(B)]
                    lp = [c.dev[i % 3][j][0].data_ptr() if j is not None else None for i, j in enumerate(idx)]
                    rp = [c.dev[i % 3][j][1].data_ptr() if j is not None else None for i, j in enumerate(idx)]
                    c.vo.submit_device(lp, rp, W, active=None if mask is None else a)
                    p = c.vo.last_frame_path()
                    ok, T = c.vo.collect()
                    if a.any():
                        assert p & 1, (k, p)
                    for i in range(B):
                        if a[i]:
                            got[i].append((bool(ok[i]), T[i].copy(), c.vo.stats[i].as_dict(), c.snap(i)))
                            nxt[i] += 1
                            last_T[i] = T[i].copy()
                        else:
                            assert not ok[i] and np.array_equal(T[i], last_T[i]) and c.vo.stats[i].fail_reason == 5, (k, i)
            finally:
                c.close()
            return got
        masked = run(act)
        full = run(None)
    finally:
        nb.close()
    for i in range(B):
        assert len(masked[i]) >= 3, i
        for j, (g, w) in enumerate(zip(masked[i], full[i])):
            assert g[0] == w[0] and np.array_equal(g[1], w[1]) and g[2] == w[2], (i, j, g[2], w[2])
            assert all(np.array_equal(u, v) for u, v in zip(g[3], w[3])), (i, j)


# ------------------------------------------------------------------------------------------------ the forced-lean knob
# Run under SVO_FORCE_LEAN=1 in a fresh process (the knob is read once per process).  Left out on purpose: every test that
# asserts the full builds' path (test_two_many_sequence_contexts_sharing_the_device asserts its frames are NOT lean).
FORCED_SELECTION = [
    ("tests/test_gpu_parity.py", "camera_to_world or five_tracks or failure_paths or outlier_scene or cfg3 or fuzz"),
    ("tests/test_gpu_sequence_lifecycle.py", "idle_invariance or idle_rows or reset or all_idle or null_mask or masked_other"),
    # the stage entry on degenerate disparities through k_triangulate_lean; the tests themselves assert SVO_PATH_LEAN of every call
    ("tests/test_gpu_triangulate_edges.py", "test_stage"),
    # the pose stage at count, chunk and geometry edges through k_pnp_epnp_lean (8 lanes per hypothesis) and k_pnp_final_lean
    # (256 threads, two virtual threads each); every call asserts SVO_PATH_LEAN there too
    ("tests/test_gpu_pnp_edges.py", "test_stage"),
]
FORCED_MIN_PASSES = [30, 10, 8, 139]


def forced_env():
    env = dict(os.environ)
    env["SVO_FORCE_LEAN"] = "1"
    env.pop("SVO_GRAPH", None)
    return env


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["parity", "lifecycle", "triangulate", "pnp_edges"])
def test_forced_lean_parity_selection(which):
    path, expr = FORCED_SELECTION[which]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", path, "-k", expr],
                       cwd=ROOT, env=forced_env(), capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= FORCED_MIN_PASSES[which], tail
    assert not re.search(r"\d+ (skipped|xfailed|xpassed)", r.stdout), tail


def test_forced_lean_takes_the_lean_builds():
    """Under the knob, lone, many-sequence and stage contexts report the lean bit (tests/lean_child.py)."""
    r = run_child("lean_child.py", cwd=ROOT, env=forced_env())
    assert "lean child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
