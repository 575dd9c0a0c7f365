"""Ragged and continuous batching on a real GPU: per-frame idle masks (svo_process_batch_masked / svo_submit_batch_masked) and
sequence resets (svo_reset_sequence).  The yardstick is a one-sequence context fed only that sequence's active frames — a path
the parity tests pin to the oracle — and everything a frame produces must equal it bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gpu_kit
from gpu_kit import api, same as same_snap, snap  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

W, H = 320, 160


def make_streams(n_seq, n_frames, seed0, cn=1):
    return gpu_kit.streams(n_seq, n_frames, seed0, W, H, cn)


def projections(scale=1.0):
    Pl, Pr = gpu_kit.projections(W, H)
    Pl[0, 0] *= scale; Pr[0, 0] *= scale; Pr[0, 3] *= scale
    return Pl, Pr


def cfg_for(api, **over):
    return api.default_config(max_translation_norm=2.0, **over)


def row(ok, T, st):
    return bool(ok), np.asarray(T).reshape(16).copy(), st.as_dict()


def single_run(api, cfg, frames, P=None, snaps=True):
    """One-sequence context fed `frames` [(L, R)] -> [(row, snapshot)]."""
    Pl, Pr = P if P is not None else projections()
    vo = api.BatchVisualOdometry(W, H, 1, cfg); vo.initalize_projection_matricies(Pl, Pr)
    out = []
    for L, R in frames:
        ok, T = vo.stereo_callback_batch([L], [R])
        out.append((row(ok[0], T[0], vo.stats[0]), snap(vo, 0) if snaps else None))
    vo.close()
    return out


def check_idle_row(r, last_T):
    ok, T, st = r
    assert not ok and np.array_equal(T, last_T)
    assert st["fail_reason"] == 5 and all(v == 0 for k, v in st.items() if k != "fail_reason"), st


def schedule(n_steps, B, seed, p=0.65):
    rng = np.random.default_rng(seed)
    act = rng.random((n_steps, B)) < p
    act[1] = True                                                  # one full frame in the middle of the ragged ones
    return act


def masked_run(api, cfg, streams, act, device=False, graph_alternate=False):
    """A B-sequence context over the schedule `act` (steps x B); sequence i's j-th active frame is its stream's frame j.
    Host images: synchronous calls, snapshots after every frame.  Device images: submitted two frames ahead, rows only.
    Returns per sequence the list of (row, snapshot) of its active frames, and checks every idle row on the way."""
    B = len(streams)
    Pl, Pr = projections()
    vo = api.BatchVisualOdometry(W, H, B, cfg); vo.initalize_projection_matricies(Pl, Pr)
    cn = max(1, cfg.channels)
    nxt = [0] * B
    got = [[] for _ in range(B)]
    last_T = [np.eye(4).reshape(16) for _ in range(B)]
    plan = []                                                      # per frame: stream index of every sequence (None: idle), mask
    for k in range(len(act)):
        full = graph_alternate and k % 2 == 0                      # graph mode: every other frame unmasked (a replayed graph)
        a = np.ones(B, bool) if full else act[k]
        idx = [nxt[i] if a[i] else None for i in range(B)]
        for i in range(B):
            nxt[i] += int(a[i])
        plan.append((idx, None if full else a))
    if device:
        import torch
        dev = [[(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in zip(*s)] for s in streams]
        torch.cuda.synchronize()

        def submit(k):
            idx, a = plan[k]
            lp = [dev[i][j][0].data_ptr() if j is not None else None for i, j in enumerate(idx)]
            rp = [dev[i][j][1].data_ptr() if j is not None else None for i, j in enumerate(idx)]
            vo.submit_device(lp, rp, W * cn, active=a)
        submit(0)
        for k in range(len(plan)):
            if k + 1 < len(plan):
                submit(k + 1)
            ok, T = vo.collect()
            for i, j in enumerate(plan[k][0]):
                r = row(ok[i], T[i], vo.stats[i])
                if j is None:
                    check_idle_row(r, last_T[i])
                else:
                    got[i].append((r, None))
                last_T[i] = r[1]
        snaps_end = [snap(vo, i) for i in range(B)]
        vo.close()
        return got, snaps_end
    for k, (idx, a) in enumerate(plan):
        Ls = [streams[i][0][j] if j is not None else None for i, j in enumerate(idx)]
        Rs = [streams[i][1][j] if j is not None else None for i, j in enumerate(idx)]
        ok, T = vo.stereo_callback_batch(Ls, Rs, active=a)
        for i, j in enumerate(idx):
            r = row(ok[i], T[i], vo.stats[i])
            if j is None:
                check_idle_row(r, last_T[i])
            else:
                got[i].append((r, snap(vo, i)))
            last_T[i] = r[1]
    snaps_end = [snap(vo, i) for i in range(B)]
    vo.close()
    return got, snaps_end


def assert_matches_singles(api, cfg, streams, got, snaps_end=None):
    for i, (L, R) in enumerate(streams):
        n = len(got[i])
        want = single_run(api, cfg, list(zip(L[:n], R[:n])))
        assert n == len(want)
        for j, ((gr, gs), (wr, ws)) in enumerate(zip(got[i], want)):
            assert gr[0] == wr[0] and np.array_equal(gr[1], wr[1]) and gr[2] == wr[2], (i, j, gr, wr)
            if gs is not None:
                assert same_snap(gs, ws), (i, j)
        if snaps_end is not None and n:
            assert same_snap(snaps_end[i], want[-1][1]), i
        if n >= 3:
            assert any(r[0][2]["n_into_lk"] > 20 for r in want[1:]), "sequence %d never tracked: the comparison would be vacuous" % i


# ---------------------------------------------------------------------------------------------------------- 1. idle invariance
@pytest.mark.parametrize("B", [4, 12])
def test_idle_invariance_bit_exact(api, B):
    """B = 4: the lone-stream fused front; B = 12: the many-sequence path that builds the next frame's pyramids ahead."""
    act = schedule(8, B, seed=100 + B)
    streams = make_streams(B, 8, seed0=300 + B)
    cfg = cfg_for(api)
    got, end = masked_run(api, cfg, streams, act)
    assert_matches_singles(api, cfg, streams, got, end)


def test_idle_invariance_stage_timing_device_images(api, monkeypatch):
    """B = 12 with the stage-boundary events on (SVO_STAGE_TIMING=1), device images, two frames in flight."""
    monkeypatch.setenv("SVO_STAGE_TIMING", "1")
    B = 12
    act = schedule(8, B, seed=7)
    streams = make_streams(B, 8, seed0=500)
    cfg = cfg_for(api)
    got, end = masked_run(api, cfg, streams, act, device=True)
    monkeypatch.delenv("SVO_STAGE_TIMING")
    assert_matches_singles(api, cfg, streams, got, end)


# ---------------------------------------------------------------------------------------------- 2. idle rows, untouched state
def test_idle_rows_leave_state_untouched(api):
    B = 4
    streams = make_streams(B, 6, seed0=900)
    Pl, Pr = projections()
    vo = api.BatchVisualOdometry(W, H, B, cfg_for(api)); vo.initalize_projection_matricies(Pl, Pr)
    for k in range(3):
        ok, T = vo.stereo_callback_batch([s[0][k] for s in streams], [s[1][k] for s in streams])
    good_T = T[1].reshape(16).copy()                               # the row's T is last_transform whether the frame succeeded or not
    before = snap(vo, 1)
    act = np.array([1, 0, 1, 1], np.uint8)
    for k in range(3, 6):
        Ls = [s[0][k] if act[i] else None for i, s in enumerate(streams)]
        Rs = [s[1][k] if act[i] else None for i, s in enumerate(streams)]
        ok, T = vo.stereo_callback_batch(Ls, Rs, active=act)
        check_idle_row(row(ok[1], T[1], vo.stats[1]), good_T)
        assert vo.stats[0].fail_reason != 5
        assert same_snap(snap(vo, 1), before)
    vo.close()


# ------------------------------------------------------------------------------------------------------------------ 3. reset
def test_reset_mid_run(api):
    """Sequence 3 is reset (projection kept) and sequence 5 reset with new matrices after frame 4 of 8: their later outputs equal
    fresh contexts on the same frames, every other sequence equals the run without resets."""
    B, N, CUT = 12, 8, 4
    streams = make_streams(B, N, seed0=1200)
    cfg = cfg_for(api)
    Pl, Pr = projections()
    P2 = projections(1.02)

    def run(reset):
        vo = api.BatchVisualOdometry(W, H, B, cfg); vo.initalize_projection_matricies(Pl, Pr)
        rows = []
        for k in range(N):
            if reset and k == CUT:
                vo.reset_sequence(3)
                vo.reset_sequence(5, *P2)
            ok, T = vo.stereo_callback_batch([s[0][k] for s in streams], [s[1][k] for s in streams])
            rows.append([(row(ok[i], T[i], vo.stats[i]), snap(vo, i)) for i in range(B)])
        vo.close()
        return rows

    plain, reset = run(False), run(True)
    for i in range(B):
        if i in (3, 5):
            want = single_run(api, cfg, list(zip(streams[i][0][CUT:], streams[i][1][CUT:])), P=P2 if i == 5 else None)
            assert reset[CUT][i][0][2]["fail_reason"] == 1
            for k in range(CUT, N):
                (gr, gs), (wr, ws) = reset[k][i], want[k - CUT]
                assert gr[0] == wr[0] and np.array_equal(gr[1], wr[1]) and gr[2] == wr[2] and same_snap(gs, ws), (i, k)
            for k in range(CUT):
                assert np.array_equal(reset[k][i][0][1], plain[k][i][0][1])
        else:
            for k in range(N):
                (gr, gs), (wr, ws) = reset[k][i], plain[k][i]
                assert gr[0] == wr[0] and np.array_equal(gr[1], wr[1]) and gr[2] == wr[2] and same_snap(gs, ws), (i, k)
    assert any(reset[k][5][0][2]["n_into_lk"] > 20 for k in range(CUT + 1, N))


# ------------------------------------------------------------------------------------------------------------ 4. stream order
def test_reset_is_stream_ordered(api):
    """submit, submit, reset, submit, submit, collect x 4: the reset lands exactly between frames 2 and 3."""
    import torch
    B = 12
    streams = make_streams(B, 4, seed0=1500)
    cfg = cfg_for(api)
    Pl, Pr = projections()
    dev = [[(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in zip(*s)] for s in streams]
    torch.cuda.synchronize()
    vo = api.BatchVisualOdometry(W, H, B, cfg); vo.initalize_projection_matricies(Pl, Pr)
    submit = lambda k: vo.submit_device([dev[i][k][0].data_ptr() for i in range(B)], [dev[i][k][1].data_ptr() for i in range(B)], W)
    submit(0); submit(1)
    vo.reset_sequence(2)
    submit(2); submit(3)
    rows = []
    for _ in range(4):
        ok, T = vo.collect()
        rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(B)])
    vo.close()
    plain = single_run(api, cfg, list(zip(streams[2][0], streams[2][1])), snaps=False)
    fresh = single_run(api, cfg, list(zip(streams[2][0][2:], streams[2][1][2:])), snaps=False)
    for k, want in ((0, plain[0][0]), (1, plain[1][0]), (2, fresh[0][0]), (3, fresh[1][0])):
        g = rows[k][2]
        assert g[0] == want[0] and np.array_equal(g[1], want[1]) and g[2] == want[2], k
    assert rows[2][2][2]["fail_reason"] == 1 and rows[1][2][2]["fail_reason"] != 1
    other = single_run(api, cfg, list(zip(streams[7][0], streams[7][1])), snaps=False)
    for k in range(4):
        assert rows[k][7][2] == other[k][0][2] and np.array_equal(rows[k][7][1], other[k][0][1])


# ------------------------------------------------------------------------------------------------------------------ 5. edges
def test_all_idle_frame_then_continue(api):
    B = 4
    streams = make_streams(B, 4, seed0=1800)
    act = np.ones((5, B), bool); act[2] = False                    # frame 2 is all idle
    cfg = cfg_for(api)
    got, end = masked_run(api, cfg, streams, act)
    assert all(len(g) == 4 for g in got)
    assert_matches_singles(api, cfg, streams, got, end)


def test_null_mask_equals_unmasked_and_arg_errors(api):
    lib = api.lib
    B = 4
    streams = make_streams(B, 3, seed0=2100)
    cfg = cfg_for(api)
    Pl, Pr = projections()
    ctx = [C.c_void_p() for _ in range(3)]
    for c in ctx:
        api.check(lib.svo_create(C.byref(cfg), 0, B, W, H, C.byref(c)))
        api.check(lib.svo_set_projection(c, -1, api.ptr(Pl.reshape(12)), api.ptr(Pr.reshape(12))))
    ones = np.ones(B, np.uint8)
    for k in range(3):
        lp = (C.c_void_p * B)(*[s[0][k].ctypes.data for s in streams]); rp = (C.c_void_p * B)(*[s[1][k].ctypes.data for s in streams])
        outs = []
        for j, c in enumerate(ctx):
            T = np.zeros((B, 16)); ok = np.zeros(B, np.int32); st = (api.SvoFrameStats * B)()
            if j == 0:
                api.check(lib.svo_process_batch(c, lp, rp, W, 0, api.ptr(T), api.ptr(ok), st))
            else:
                api.check(lib.svo_process_batch_masked(c, lp, rp, W, 0, None if j == 1 else api.ptr(ones), api.ptr(T), api.ptr(ok), st))
            outs.append((T, ok, [s.as_dict() for s in st]))
        for o in outs[1:]:
            assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2], k
    c = ctx[0]
    act = np.array([1, 0, 1, 1], np.uint8)
    L = streams[0][0][0]
    lp = (C.c_void_p * B)(L.ctypes.data, None, None, L.ctypes.data); rp = (C.c_void_p * B)(L.ctypes.data, None, L.ctypes.data, L.ctypes.data)
    T = np.zeros((B, 16)); ok = np.zeros(B, np.int32)
    assert lib.svo_process_batch_masked(c, lp, rp, W, 0, api.ptr(act), api.ptr(T), api.ptr(ok), None) == api._lib.SVO_ERR_ARG
    assert lib.svo_submit_batch_masked(c, lp, rp, W, api.ptr(act)) == api._lib.SVO_ERR_ARG
    assert lib.svo_reset_sequence(c, B, None, None) == api._lib.SVO_ERR_ARG
    assert lib.svo_reset_sequence(c, -2, None, None) == api._lib.SVO_ERR_ARG
    assert lib.svo_reset_sequence(c, 0, api.ptr(Pl.reshape(12)), None) == api._lib.SVO_ERR_ARG
    assert lib.svo_reset_sequence(c, 0, None, api.ptr(Pr.reshape(12))) == api._lib.SVO_ERR_ARG
    for cc in ctx:
        lib.svo_destroy(cc)


def test_visual_odometry_reset_starts_over(api):
    streams = make_streams(1, 4, seed0=2400)
    L, R = streams[0]
    Pl, Pr = projections()
    vo = api.VisualOdometry(cfg=cfg_for(api)); vo.initalize_projection_matricies(Pl, Pr)
    vo.stereo_callback(L[0], R[0]); vo.stereo_callback(L[1], R[1])
    vo.reset()
    got = []
    for k in (2, 3):
        ok, T = vo.stereo_callback(L[k], R[k])
        got.append((ok, T.reshape(16).copy(), vo.stats.as_dict()))
    want = single_run(api, cfg_for(api), [(L[2], R[2]), (L[3], R[3])], snaps=False)
    assert got[0][2]["fail_reason"] == 1
    for g, (w, _) in zip(got, want):
        assert g[0] == w[0] and np.array_equal(g[1], w[1]) and g[2] == w[2]


# ------------------------------------------------------------------------------------------------- 6. other kernel families
@pytest.mark.parametrize("family", ["bgr", "features_per_bucket_3", "float_sums"])
def test_masked_other_kernel_families(api, family):
    over = {"bgr": dict(channels=3), "features_per_bucket_3": dict(features_per_bucket=3), "float_sums": dict(lk_float_sums=1)}[family]
    B = 12 if family == "features_per_bucket_3" else 4
    cfg = cfg_for(api, **over)
    act = schedule(6, B, seed=len(family))
    streams = make_streams(B, 6, seed0=2700, cn=cfg.channels)
    got, end = masked_run(api, cfg, streams, act)
    assert_matches_singles(api, cfg, streams, got, end)


def test_graph_mode_alternating_full_and_masked(api, monkeypatch):
    """SVO_GRAPH=1, B = 12: full frames replay captured graphs, ragged ones run from the launch list, two frames in flight — the
    build-ahead path then follows frames that did not go through it (the image stream must wait for them)."""
    monkeypatch.setenv("SVO_GRAPH", "1")
    B = 12
    act = schedule(8, B, seed=99)
    streams = make_streams(B, 8, seed0=3000)
    cfg = cfg_for(api)
    got, end = masked_run(api, cfg, streams, act, device=True, graph_alternate=True)
    monkeypatch.delenv("SVO_GRAPH")
    assert_matches_singles(api, cfg, streams, got, end)
