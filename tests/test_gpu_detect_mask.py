"""Detection masks on a real GPU (include/svo.h, "Detection masks"): the masked stage calls against the definition, the frame
pipeline against stereo_callback composed from the oracle's stages with a masked detection stage (tests/detect_mask_ref.py) —
features, tracks and inlier masks bit for bit, poses within 1e-6 — on lone-stream (1, 3 sequences) and many-sequence (10) launch
lists, with static, per-sequence and per-frame masks, frames in flight, second passes, dropped tracks, clearing, colour input,
rectification, ragged frames and SVO_GRAPH=1.  A mask belongs to a left image: the one set before call k is applied by call k + 1."""
import os

import numpy as np
import pytest

import detect_mask_ref as ref
import oracle_lib as orc
from gpu_kit import api, f32_bits as bits, run_child, same, snap  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

SIZES = {"even": (320, 160), "odd": (323, 163)}       # tests/test_gpu_input_format.py's: whole 64 x 16 FAST tiles, and partial ones on every side
OVER = dict(max_translation_norm=2.0)


def streams_of(n_seq, n_frames, w, h, seed0=900, blank=()):
    """n_seq streams (three distinct ones, reused in turn) and their projection matrices"""
    base = [ref.stream(n_frames, seed0 + 31 * i, w, h, blank) for i in range(min(n_seq, 3))]
    return [base[i % len(base)][0] for i in range(n_seq)], base[0][1]


# ------------------------------------------------------------------------------------------------ the driver
class InForce:
    """The test's model of the setter: shared and own masks; mask(i) = what svo_set_detection_mask says is in force for i."""

    def __init__(self, n):
        self.shared, self.own = None, [None] * n

    def set(self, vo, mask, seq=-1, device=False):
        if mask is None:
            vo.clear_detection_mask(seq)
            if seq < 0:
                self.shared, self.own = None, [None] * len(self.own)
            else:
                self.own[seq] = None
            return
        if device:
            import torch
            pitch = mask.shape[1] + 13                              # rows further apart than they are long
            t = torch.zeros((mask.shape[0], pitch), dtype=torch.uint8, device="cuda")
            t[:, :mask.shape[1]] = torch.from_numpy(mask).cuda()
            torch.cuda.synchronize()
            vo.set_detection_mask(t[:, :mask.shape[1]], seq)
            self.keep = getattr(self, "keep", []) + [t]             # the library has copied it on its stream; kept until the run ends
        else:
            vo.set_detection_mask(mask, seq)
        if seq < 0:
            self.shared = mask
        else:
            self.own[seq] = mask

    def mask(self, i):
        return self.own[i] if self.own[i] is not None else self.shared


def run_masked(api, w, h, streams, P, plan, mode="host", depth=3, active=None, cfg_over=None, setup=None, frames=None, oracle_frames=None):
    """A len(streams)-sequence context over every frame, against one MaskedOracleVO per sequence.
    plan(k, set): called before frame k is submitted; set(mask, seq=-1, device=False) installs or (mask None) clears.
    mode "host": synchronous frames, everything compared after every frame, and every pl0 must lie on a non-zero byte of the
    mask its detection applied.  mode "device": frames submitted `depth` ahead; poses per frame, features and tracks at the end.
    active: per frame None or flags (host mode).  frames: what the context is fed, when that differs from what the oracle sees
    (oracle_frames).  -> (paths, per-frame stats of the context, the oracle objects)."""
    B = len(streams)
    feed = frames if frames is not None else streams
    seen = oracle_frames if oracle_frames is not None else streams
    over = dict(OVER, **(cfg_over or {}))
    vo = api.BatchVisualOdometry(w, h, B, api.default_config(**over))
    vo.initalize_projection_matricies(*P)
    if setup:
        setup(vo)
    os_ = [ref.MaskedOracleVO(orc.default_config(**over)) for _ in range(B)]
    for o in os_:
        o.initalize_projection_matricies(*P)
    force = InForce(B)
    n = len(streams[0][0])
    paths, stats, want = [], [], []

    def oracle_step(k, on):
        want.append([os_[i].stereo_callback(seen[i][0][k], seen[i][1][k], force.mask(i)) if on[i] else None for i in range(B)])

    def compare_state(k, i, what):
        f, fo = vo.features(i), os_[i].features()
        assert np.array_equal(bits(f[0]), bits(fo[0])) and np.array_equal(f[1], fo[1]) and np.array_equal(f[2], fo[2]), "%s frame %d seq %d: feature set" % (what, k, i)
        to = os_[i].last_tracks()
        if to is None:
            return
        t = vo.last_tracks(i)
        for key in ("pl0", "pr0", "pl1", "pr1"):
            assert np.array_equal(bits(t[key]), bits(to[key])), "%s frame %d seq %d: %s" % (what, k, i, key)
        assert np.array_equal(t["inlier"], to["inlier"]), "%s frame %d seq %d: inlier mask" % (what, k, i)
        m = os_[i].scanned_mask
        if m is not None and len(t["pl0"]):                          # the property, independent of the reference's lists
            assert ref.mask_filter(t["pl0"], m).all(), "%s frame %d seq %d: a track starts on a masked-out pixel" % (what, k, i)

    def compare_row(k, i, ok, T, what):
        ok_o, T_o = want[k][i]
        assert bool(ok) == ok_o, "%s frame %d seq %d: ok %s vs %s" % (what, k, i, ok, ok_o)
        assert np.abs(T - T_o).max() < 1e-6, "%s frame %d seq %d: pose" % (what, k, i)

    if mode == "host":
        for k in range(n):
            plan(k, lambda mask, seq=-1, device=False: force.set(vo, mask, seq, device))
            act = active[k] if active else None
            on = [True] * B if act is None else [bool(x) for x in act]
            oracle_step(k, on)
            ok, T = vo.stereo_callback_batch([feed[i][0][k] if on[i] else None for i in range(B)],
                                             [feed[i][1][k] if on[i] else None for i in range(B)], active=act)
            paths.append(vo.last_frame_path()); stats.append([s.as_dict() for s in vo.stats])
            for i in range(B):
                if on[i]:
                    compare_row(k, i, ok[i], T[i], mode)
                compare_state(k, i, mode)                            # an idle sequence's state must not have moved either
    else:
        import torch
        dev = [[(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in zip(*s)] for s in feed]
        torch.cuda.synchronize()
        stride = feed[0][0][0].strides[0]
        sub = 0
        for k in range(n):
            while sub < n and sub - k < depth:
                plan(sub, lambda mask, seq=-1, device=False: force.set(vo, mask, seq, device))
                oracle_step(sub, [True] * B)
                vo.submit_device([dev[i][sub][0].data_ptr() for i in range(B)], [dev[i][sub][1].data_ptr() for i in range(B)], stride)
                paths.append(vo.last_frame_path()); sub += 1
            ok, T = vo.collect()
            stats.append([s.as_dict() for s in vo.stats])
            for i in range(B):
                compare_row(k, i, ok[i], T[i], mode)
        for i in range(B):
            compare_state(n - 1, i, mode)
        del dev
    vo.close()
    return paths, stats, os_


def masked_bits(api, paths):
    return [bool(p & api._lib.PATH_DETECT_MASKED) for p in paths]


# ------------------------------------------------------------------------------------------------ 1. stage parity
def stage_masks(img, w, h):
    """name -> mask.  `edge` runs through FAST tile boundaries (x = 64, y = 16) and bucket boundaries (the default grid's buckets
    are 3 x 2 pixels here: x = 63 / 66, y = 16 / 18) one pixel to either side; `nms` removes NMS winners only."""
    out = {"zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}
    yy, xx = np.mgrid[0:h, 0:w]
    out["checker"] = (((xx + yy) & 1) * 200).astype(np.uint8)
    e = np.zeros((h, w), np.uint8)
    e[16:, 64:] = 1; e[:16, 129:] = 9; e[17:33, :63] = 3; e[48:, 66:192] = 0; e[h - 20:, :] = 255
    out["edge"] = e
    winners = orc.fast_score_map(img, 20, True) != 0
    out["nms"] = np.where(winners, 0, 255).astype(np.uint8)
    return out


MASK_NAMES = ["zeros", "full", "checker", "edge", "nms"]


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("name", MASK_NAMES)
def test_stage_calls_equal_the_definition(api, size, name):
    w, h = SIZES[size]
    (L, _), _ = ref.stream(2, 41, w, h)
    img = L[0]
    mask = stage_masks(img, w, h)[name]
    for th in (20, 5):
        xy, resp = api.featureDetectionFast(img, th, mask=mask)
        wxy, wresp = ref.masked_detect(img, th, mask)
        assert np.array_equal(bits(xy), bits(wxy)) and np.array_equal(resp, wresp), (name, th, len(xy), len(wxy))
    if name == "nms":
        # every winner is masked out, and none of the neighbours it suppressed comes back: the mask is applied AFTER the suppression
        raw = orc.fast_score_map(img, 20, False) != 0
        assert raw.sum() > (orc.fast_score_map(img, 20, True) != 0).sum() > 50
        assert len(api.featureDetectionFast(img, 20, mask=mask)[0]) == 0
    cfg, ocfg = api.default_config(), orc.default_config()
    none = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    old = ref.masked_append(L[1], none, None, ocfg)                  # tracks from another image, aged so that they win buckets
    old = (old[0] + np.float32(0.37), old[1] + 3, old[2])
    for th in (20, 5):
        fs = api.FeatureSet()
        fs.points, fs.ages, fs.strengths = old[0].copy(), old[1].copy(), old[2].copy()
        fs.appendFeaturesFromImage(img, th, cfg, mask=mask)
        want = ref.masked_append(img, old, mask, ocfg, th)
        assert np.array_equal(bits(fs.points), bits(want[0])) and np.array_equal(fs.ages, want[1]) and np.array_equal(fs.strengths, want[2]), (name, th)
        assert api.last_stage_path() & api._lib.PATH_DETECT_MASKED
    if name in ("checker", "edge"):
        assert 0 < len(want[1]) < len(ref.masked_append(img, old, None, ocfg, 5)[1])


# ------------------------------------------------------------------------------------------------ 2. pipeline parity
@pytest.mark.parametrize("n_seq", [1, 3, 10])
def test_static_shared_mask(api, n_seq):
    w, h = SIZES["odd"]
    streams, P = streams_of(n_seq, 5, w, h)
    mask = ref.blob_mask(w, h, 5)
    paths, stats, _ = run_masked(api, w, h, streams, P, lambda k, set: set(mask) if k == 0 else None)
    assert masked_bits(api, paths) == [False] + [True] * 4           # call 0 scans nothing; call k scans image k - 1 with its mask
    L = api._lib
    assert not any(p & L.PATH_FRONT_FUSED for p in paths[1:])        # a masked lone-stream frame issues the unfused front
    assert all(s["fail_reason"] == 0 for s in stats[-1])


@pytest.mark.parametrize("n_seq", [3, 10])
def test_per_sequence_masks_with_one_sequence_left_without(api, n_seq):
    w, h = SIZES["odd"]
    streams, P = streams_of(n_seq, 4, w, h)

    def plan(k, set):
        if k == 0:
            for i in range(n_seq):
                if i != 1:                                           # sequence 1: a null entry in the launch's pointer row
                    set(ref.blob_mask(w, h, 20 + i), i)
    paths, stats, os_ = run_masked(api, w, h, streams, P, plan)
    assert masked_bits(api, paths) == [False, True, True, True]
    assert os_[1].scanned_mask is None and os_[0].scanned_mask is not None
    assert all(s["fail_reason"] == 0 for s in stats[-1])


@pytest.mark.parametrize("n_seq", [1, 10])
def test_a_different_mask_before_every_frame_with_frames_in_flight(api, n_seq):
    """The detection of call k + 1 uses the mask set before call k.  Three frames in flight, host and device masks alternating,
    the shared mask and one sequence's own."""
    w, h = SIZES["odd"]
    streams, P = streams_of(n_seq, 6, w, h)

    def plan(k, set):
        set(ref.band_mask(w, h, 40 * k, 40 * k + 90), device=k % 2 == 1)
        if n_seq > 1:
            set(ref.blob_mask(w, h, 70 + k), n_seq - 1, device=k % 2 == 0)
    paths, stats, _ = run_masked(api, w, h, streams, P, plan, mode="device", depth=3)
    assert masked_bits(api, paths) == [False] + [True] * 5
    assert all(s["fail_reason"] == 0 for s in stats[-1])


@pytest.mark.parametrize("n_seq", [1, 10])
def test_a_frame_that_takes_the_second_pass(api, n_seq):
    """A mask that leaves a small window open: fewer than pre_matching_feature_threshold features survive the first pass, and the
    second pass (a quarter of the threshold; the strided kernels with many sequences) applies the same mask."""
    w, h = SIZES["odd"]
    streams, P = streams_of(n_seq, 4, w, h)
    mask = np.zeros((h, w), np.uint8); mask[30:120, 100:230] = 1
    paths, stats, _ = run_masked(api, w, h, streams, P, lambda k, set: set(mask) if k == 0 else None, cfg_over=dict(pre_matching_feature_threshold=2000))
    assert all(s["second_pass"] == 1 for fr in stats[1:] for s in fr)
    assert all(s["n_after_detect"] > 50 for s in stats[-1])


def test_a_band_sweeping_across_the_image_drops_tracks(api):
    w, h = SIZES["odd"]
    streams, P = streams_of(3, 6, w, h)
    paths, stats, os_ = run_masked(api, w, h, streams, P, lambda k, set: set(ref.band_mask(w, h, 60 * k - 30, 60 * k + 50)))
    free, _ = streams_of(3, 6, w, h)
    o = orc.VisualOdometry(orc.default_config(**OVER)); o.initalize_projection_matricies(*P)
    for k in range(6):
        o.stereo_callback(free[0][0][k], free[0][1][k])
    assert stats[-1][0]["n_into_lk"] < o.stats.n_into_lk             # the band took tracks the unmasked run kept


def test_clearing_mid_run(api):
    """Cleared before call 3: call 3 still scans image 2 with its mask, call 4 is unmasked; set again before call 5: call 6 is masked."""
    w, h = SIZES["odd"]
    streams, P = streams_of(3, 7, w, h)
    mask = ref.blob_mask(w, h, 9)

    def plan(k, set):
        if k in (0, 5):
            set(mask)
            set(ref.blob_mask(w, h, 10), 2)
        if k == 3:
            set(None)
    paths, _, _ = run_masked(api, w, h, streams, P, plan)
    assert masked_bits(api, paths) == [False, True, True, True, False, False, True]
    L = api._lib
    assert paths[4] & L.PATH_FRONT_FUSED and paths[5] & L.PATH_FRONT_FUSED       # the old launch list again


# ------------------------------------------------------------------------------------------------ 4. no-op guarantees
@pytest.mark.parametrize("n_seq", [1, 10])
def test_all_255_mask_changes_nothing_and_no_mask_sets_no_bit(api, n_seq):
    from test_gpu_rectify import row, same_row
    w, h = SIZES["odd"]
    streams, P = streams_of(n_seq, 4, w, h)
    outs = []
    for masked in (False, True):
        vo = api.BatchVisualOdometry(w, h, n_seq, api.default_config(**OVER))
        vo.initalize_projection_matricies(*P)
        if masked:
            vo.set_detection_mask(np.full((h, w), 255, np.uint8))
            assert vo.detection_mask(0) is not None and vo.detection_mask(0).min() == 255
        else:
            assert vo.detection_mask() is None
        rows, paths = [], []
        for k in range(4):
            ok, T = vo.stereo_callback_batch([s[0][k] for s in streams], [s[1][k] for s in streams])
            rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(n_seq)]); paths.append(vo.last_frame_path())
        outs.append((rows, [snap(vo, i) for i in range(n_seq)], paths))
        vo.close()
    assert not any(masked_bits(api, outs[0][2])) and masked_bits(api, outs[1][2]) == [False, True, True, True]
    for k in range(4):
        for i in range(n_seq):
            assert same_row(outs[0][0][k][i], outs[1][0][k][i]), (k, i)
    assert all(same(a, b) for a, b in zip(outs[0][1], outs[1][1]))


# ------------------------------------------------------------------------------------------------ 5. combinations
def test_bgr8_input_format(api):
    from test_gpu_input_format import coloured
    w, h = SIZES["odd"]
    streams, P = streams_of(3, 4, w, h)
    col, grey = coloured(streams, "bgr8", seed=3)
    paths, _, _ = run_masked(api, w, h, streams, P, lambda k, set: set(ref.blob_mask(w, h, 30 + k)), setup=lambda vo: vo.set_input_format("bgr8"),
                             frames=col, oracle_frames=grey)
    assert all(p & api._lib.PATH_INPUT_CONVERTED for p in paths) and masked_bits(api, paths) == [False, True, True, True]


def test_rectifying_context(api):
    """The mask lives in the rectified geometry: the context's size, not the raw frames'."""
    import rectify_ref
    import test_gpu_rectify as tr
    pair = tr.cam_pair(0)
    mp = tr.maps_of(pair)
    raw = tr.raw_streams(3, 4, 1500)
    rect = [([rectify_ref.remap(a, *mp[0]) for a in L], [rectify_ref.remap(a, *mp[1]) for a in R]) for L, R in raw]
    paths, _, _ = run_masked(api, tr.W, tr.H, rect, tr.projections(pair), lambda k, set: set(ref.blob_mask(tr.W, tr.H, 40)) if k == 0 else None,
                             setup=lambda vo: vo.set_rectification(pair[0], pair[1]), frames=raw)
    assert masked_bits(api, paths) == [False, True, True, True]


def test_ragged_frames_leave_an_idle_sequence_alone(api):
    """Sequence 1 sits out calls 2 and 3 while its own mask is set twice: its features do not move (the driver compares every
    sequence after every frame) and the slot of its last image is not written — when it returns, call 4 scans ITS last image,
    image 1, with the mask set before call 1, and call 5 scans image 4 with the mask set before call 4."""
    w, h = SIZES["odd"]
    streams, P = streams_of(3, 6, w, h)
    act = [None, None, [1, 0, 1], [1, 0, 1], None, None]

    def plan(k, set):
        if k in (2, 3):                                              # sequence 1's: set while it is idle, for an image that never comes
            set(ref.blob_mask(w, h, 60 + k), 0)
            set(ref.blob_mask(w, h, 80 + k), 1)
            return
        for i in range(3):
            set(ref.blob_mask(w, h, 50 + 3 * k + i), i)
    # (the oracle object of an idle sequence is not called, so the mask of its last image stays the one of call 1)
    paths, stats, _ = run_masked(api, w, h, streams, P, plan, active=act)
    assert stats[2][1]["fail_reason"] == 5 and stats[3][1]["fail_reason"] == 5
    assert all(s["fail_reason"] == 0 for s in stats[-1])


def test_graph_mode_runs_masked_frames_from_the_launch_list(api, tmp_path):
    """SVO_GRAPH=1 in a fresh process: unmasked frames replay their graph, masked ones run from the launch list, and the results
    equal this process's launch-list runs."""
    import detect_mask_child as child
    out = tmp_path / "graph.npz"
    env = dict(os.environ, SVO_GRAPH="1")
    p = run_child("detect_mask_child.py", out, env=env)
    assert "detect mask child ok" in p.stdout, p.stdout + p.stderr
    d = np.load(out)
    L = api._lib
    for name, n_seq in child.RUNS:
        T, ok, paths = child.one_run(api, n_seq)
        assert np.array_equal(d[name + "_T"], T) and np.array_equal(d[name + "_ok"], ok), name
        assert [bool(q & L.PATH_DETECT_MASKED) for q in d[name + "_paths"]] == child.MASKED
        assert [bool(q & L.PATH_GRAPH) for q in d[name + "_paths"]] == [not m for m in child.MASKED], d[name + "_paths"]
        assert masked_bits(api, paths) == child.MASKED and ok[-1].all()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_refusals(api):
    w, h = SIZES["even"]
    L = api._lib
    m = np.full((h, w), 255, np.uint8)
    vo = api.BatchVisualOdometry(w, h, 2, api.default_config())
    for bad in (m[:-1], m[:, :-1], m.astype(np.int32), m[None]):
        with pytest.raises(ValueError):
            vo.set_detection_mask(bad)
    assert L.lib.svo_set_detection_mask(vo._h, 0, L.ptr(m), w - 1, 0) == L.SVO_ERR_ARG and b"stride" in L.lib.svo_last_error()
    for seq in (-2, 2):
        assert L.lib.svo_set_detection_mask(vo._h, seq, L.ptr(m), w, 0) == L.SVO_ERR_ARG
        assert L.lib.svo_get_detection_mask(vo._h, seq, None, None) == L.SVO_ERR_ARG
    assert L.lib.svo_set_detection_mask(None, 0, L.ptr(m), w, 0) == L.SVO_ERR_ARG
    vo.clear_detection_mask(); vo.clear_detection_mask(1)             # clearing what was never set is fine
    assert vo.detection_mask() is None and vo.last_frame_path() == 0
    vo.set_detection_mask(m, 1)
    assert vo.detection_mask(0) is None and vo.detection_mask(1).shape == (h, w)
    vo.close()
    for over, word in ((dict(channels=3), b"channels"), (dict(features_per_bucket=2), b"features_per_bucket")):
        vo = api.BatchVisualOdometry(w, h, 1, api.default_config(**over))
        assert L.lib.svo_set_detection_mask(vo._h, -1, L.ptr(m), w, 0) == L.SVO_ERR_ARG and word in L.lib.svo_last_error()
        with pytest.raises(L.SvoError):
            vo.set_detection_mask(m)
        vo.close()
    img = np.zeros((h, w), np.uint8)
    with pytest.raises(ValueError):
        api.featureDetectionFast(img, 20, mask=m[:-1])
    fs = api.FeatureSet()
    with pytest.raises(L.SvoError):
        fs.appendFeaturesFromImage(img, 20, api.default_config(features_per_bucket=2), mask=m)
