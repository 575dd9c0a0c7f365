"""CLAHE in frame ingest on a real GPU (include/svo.h, CLAHE section).

The two kernels are pinned to the numpy restatement (tests/clahe_ref.py) bit for bit through svo_clahe.  A CLAHE context fed the
raw frames must give exactly what a plain context gives when fed clahe_ref of the grey frames — rows, statistics, feature sets and
tracks — on every route into the pyramid (lone-stream fused front, many-sequence launches, build-ahead image stream; host, device
and asynchronous inputs; converting, rectifying, masked and ragged frames).  The setting is host state like the input format:
every frame carries the one it was issued with."""
import ctypes as C

import numpy as np
import pytest

import clahe_ref as ref
import input_format_ref as fmt_ref
import pyramid_ref
import rectify_ref
import scenes
import test_gpu_rectify as tr
from test_gpu_input_format import SIZES, assert_runs_equal, cfg_for, coloured, grey_streams, run, strided
from test_gpu_rectify import row, same_row
from gpu_kit import api, raw_bits, same, snap  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

CLIP, TILES = 2.0, (8, 8)


_eq_cache = {}


def eq(img, clip=CLIP, tiles=TILES):
    """clahe_ref of a frame, computed once per (frame object, setting): the streams repeat their frames across sequences."""
    key = (id(img), clip, tiles)
    if key not in _eq_cache:
        _eq_cache[key] = (img, ref.clahe_ref(img, clip, tiles))       # (the frame is kept alive: its id stays its own)
    return _eq_cache[key][1]


def eq_streams(streams, clip=CLIP, tiles=TILES):
    return [([eq(a, clip, tiles) for a in L], [eq(a, clip, tiles) for a in R]) for L, R in streams]


# ------------------------------------------------------------------------------------------------ 1. the stage alone
STAGE_SIZES = [(320, 160), (323, 163), (320, 163), (37, 21)]          # divisible by 8 x 8; neither dimension; the quirk; tiny
STAGE_TILES = [(8, 8), (1, 1), (3, 2), (16, 16)]
STAGE_CLIPS = [0, 0.01, 2.0, 40.0]
STAGE_FORMATS = ["mono8", "bgr8", "bgra8", "yuv422"]
STAGE_IMAGES = ["noise", "constant", "ramp", "scene"]
STRIDES = [(0, 0), (5, 0), (0, 1), (5, 3)]                            # (slack bytes per row, byte offset of the first row)


def stage_image(name, w, h):
    if name == "noise":
        return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w)).astype(np.uint8)
    if name == "constant":
        return np.full((h, w), 100, np.uint8)
    if name == "ramp":
        return np.ascontiguousarray(np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8), (h, w)))
    return scenes.random_texture(h, w, 5)


@pytest.mark.parametrize("name", STAGE_IMAGES)
@pytest.mark.parametrize("size", STAGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_svo_clahe_equals_numpy(api, size, name):
    L = api._lib
    w, h = size
    scene = stage_image(name, w, h)
    rng = np.random.default_rng(3)
    frames = {f: fmt_ref.colour_of(scene, f, rng) for f in STAGE_FORMATS}      # every format holds the same grey image
    grey = frames["mono8"][1]
    assert all(np.array_equal(frames[f][1], grey) for f in STAGE_FORMATS)
    n_checked = 0
    for it, tiles in enumerate(STAGE_TILES):
        for ic, clip in enumerate(STAGE_CLIPS):
            if ref.geometry(w, h, tiles) is None:
                out = np.zeros((h, w), np.uint8)
                assert L.lib.svo_clahe(0, L.INPUT_MONO8, L.ptr(grey), w, h, w, clip, tiles[0], tiles[1], L.ptr(out)) == L.SVO_ERR_ARG
                continue
            want = ref.clahe_ref(grey, clip, tiles)
            for jf, f in enumerate(STAGE_FORMATS):
                extra, offset = STRIDES[(it + ic + jf) % 4]
                got = api.clahe(strided(frames[f][0], extra, offset), f, clip, tiles)
                assert np.array_equal(got, want), (size, name, tiles, clip, f, extra, offset, int((got != want).sum()))
                n_checked += 1
    assert n_checked == 64                                            # rule 1 accepts every combination of this list


def test_svo_clahe_rejections_and_extension_limits(api):
    L = api._lib
    img = np.random.default_rng(4).integers(0, 256, (40, 40)).astype(np.uint8)
    out = np.zeros_like(img)
    call = lambda w, h, clip, tx, ty, fmt=0, stride=None: L.lib.svo_clahe(0, fmt, L.ptr(img), w, h, stride or w, clip, tx, ty, L.ptr(out))
    for w, h, tiles in [(8, 9, (8, 8)), (9, 8, (8, 8)), (4, 4, (8, 8)), (5, 2, (4, 4)), (16, 17, (16, 16)), (16, 9, (16, 8))]:    # the last: the quirk alone rejects it (a divisible width grows by 16 > w - 1)
        assert ref.geometry(w, h, tiles) is None
        assert call(w, h, 2.0, *tiles) == L.SVO_ERR_ARG, (w, h, tiles)
    for tx, ty in [(0, 8), (8, 0), (17, 8), (8, 17), (-1, 4)]:
        assert call(40, 40, 2.0, tx, ty) == L.SVO_ERR_ARG
    for clip in (float("nan"), float("inf"), -float("inf")):
        assert call(40, 40, clip, 8, 8) == L.SVO_ERR_ARG
    assert call(40, 40, 2.0, 8, 8, fmt=7, stride=40) == L.SVO_ERR_ARG and call(10, 10, 2.0, 2, 2, fmt=L.INPUT_BGR8, stride=29) == L.SVO_ERR_ARG
    # the widest extensions rule 1 accepts: every extension column / row is a reflected one, down to column / row 0
    for w, h, tiles in [(9, 9, (8, 8)), (17, 18, (16, 16)), (17, 9, (16, 8))]:
        assert ref.geometry(w, h, tiles) is not None
        sub = np.ascontiguousarray(img[:h, :w])
        for clip in (0, 1.0):
            assert np.array_equal(api.clahe(sub, "mono8", clip, tiles), ref.clahe_ref(sub, clip, tiles)), (w, h, tiles, clip)
    with pytest.raises(ValueError):
        api.clahe(img, "mono8", 2.0, (0, 8))
    with pytest.raises(ValueError):
        api.clahe(img, "mono8", float("nan"))


# ------------------------------------------------------------------------------------------------ 2. the whole pipeline
def mask_of(w, h):
    m = np.full((h, w), 255, np.uint8)
    m[:, w // 3: w // 2] = 0; m[: h // 5] = 0
    return m


EQUAL = [  # n_seq, entry (host / device: one frame in flight / async: two), size, variant
    (1, "host", "even", "mono8"), (1, "device", "odd", "bgr8"), (1, "async", "odd", "mono8"), (1, "host", "even", "rect"), (1, "host", "odd", "mask"),
    (3, "host", "odd", "bgr8"), (3, "device", "even", "mono8"), (3, "async", "even", "rect"), (3, "async", "even", "mask"),
    (9, "async", "odd", "mono8"), (9, "device", "even", "bgr8"), (9, "host", "even", "rect"), (9, "async", "odd", "mask"), (9, "host", "even", "mono8"),
]


@pytest.mark.parametrize("n_seq,entry,size,variant", EQUAL)
def test_clahe_context_equals_plain_on_equalised_frames(api, n_seq, entry, size, variant):
    L = api._lib
    n = 6
    mode, depth = ("host", 1) if entry == "host" else ("device", 1 if entry == "device" else 2)
    cfg = cfg_for(api)
    on = lambda vo: vo.set_clahe(CLIP, TILES)
    fmt = None
    if variant == "rect":                                             # CLAHE runs on the RAW frame (344 x 180: the padding quirk), then the remap
        pair = tr.cam_pair(0)
        mp = tr.maps_of(pair)
        w, h = tr.W, tr.H
        base = tr.raw_streams(3 if n_seq > 1 else 1, n, 2100)
        P = tr.projections(pair)
        fed = [base[i % len(base)] for i in range(n_seq)]
        plain = [([rectify_ref.remap(a, *mp[0]) for a in Lq], [rectify_ref.remap(a, *mp[1]) for a in Rq]) for Lq, Rq in eq_streams(fed)]
        rect = lambda vo: vo.set_rectification(pair[0], pair[1])
        setup, plain_setup = (lambda vo: (rect(vo), on(vo))), None
    else:
        w, h = SIZES[size]
        base, P = grey_streams(3 if n_seq > 1 else 1, n, 2000, w, h)
        fed = [base[i % len(base)] for i in range(n_seq)]
        setup, plain_setup = on, None
        if variant == "bgr8":
            fmt = "bgr8"
            fed, grey = coloured(fed, "bgr8", seed=90 + n_seq)
            plain = eq_streams(grey)
        else:
            plain = eq_streams(fed)
        if variant == "mask":
            m = mask_of(w, h)
            setup, plain_setup = (lambda vo: (on(vo), vo.set_detection_mask(m))), (lambda vo: vo.set_detection_mask(m))
    got, paths = run(api, w, h, cfg, fed, P, mode, fmt=fmt, setup=setup, depth=depth)
    want, plain_paths = run(api, w, h, cfg, plain, P, mode, setup=plain_setup, depth=depth)
    assert_runs_equal(got, want, "%s %s %s" % (variant, entry, size))
    route = L.PATH_INGEST_AHEAD if n_seq > 8 else (L.PATH_FRONT_FUSED if variant != "mask" else 0)
    assert all(p & L.PATH_CLAHE and (p & route) == route for p in paths), paths
    assert all(bool(p & L.PATH_INPUT_CONVERTED) == (variant == "bgr8") for p in paths), paths
    assert all(not p & (L.PATH_CLAHE | L.PATH_INPUT_CONVERTED) and (p & route) == route for p in plain_paths), plain_paths
    if variant == "mask":
        assert any(p & L.PATH_DETECT_MASKED for p in paths)
    assert any(r[0] for r in got[0][-1]), "no pose in the last frame: the test would not see tracking differences"


@pytest.mark.parametrize("size", ["even", "odd"])
def test_ragged_frames_with_a_reset_mid_run(api, size):
    """A ragged `active` mask (one all-idle frame), sequence 1 reset before frame 3: idle sequences are not touched."""
    w, h = SIZES[size]
    n_seq, n = 9, 6
    base, P = grey_streams(3, n, 2000, w, h)
    fed = [base[i % 3] for i in range(n_seq)]
    rng = np.random.default_rng(17)
    acts = [None] + [(rng.random(n_seq) < 0.6) for _ in range(n - 1)]
    acts[2] = np.zeros(n_seq, bool)
    for a in acts[3:]:
        a[1] = True                                                   # the reset sequence goes on afterwards
    L = api._lib

    def go(streams, clahe):
        vo = api.BatchVisualOdometry(w, h, n_seq, cfg_for(api)); vo.initalize_projection_matricies(*P)
        if clahe:
            vo.set_clahe(CLIP, TILES)
        rows, snaps, paths = [], [], []
        for k in range(n):
            if k == 3:
                vo.reset_sequence(1)
            on = [True] * n_seq if acts[k] is None else [bool(x) for x in acts[k]]
            ok, T = vo.stereo_callback_batch([s[0][k] if o else None for s, o in zip(streams, on)],
                                             [s[1][k] if o else None for s, o in zip(streams, on)], active=acts[k])
            paths.append(vo.last_frame_path())
            rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(n_seq)])
            snaps.append([snap(vo, i) for i in range(n_seq)])
        vo.close()
        return (rows, snaps), paths
    got, paths = go(fed, True)
    want, _ = go(eq_streams(fed), False)
    assert_runs_equal(got, want, "ragged")
    assert paths[2] == 0 and all(p & L.PATH_CLAHE for k, p in enumerate(paths) if k != 2), paths
    assert any(r[2]["fail_reason"] == 5 for fr in got[0] for r in fr) and any(r[0] for r in got[0][-1])


# ------------------------------------------------------------------------------------------------ 3. level 0
@pytest.mark.parametrize("n_seq", [1, 9])
def test_level_0_is_the_equalised_frame(api, n_seq):
    w, h = SIZES["odd"]
    base, P = grey_streams(3, 2, 2200, w, h)
    fed = [base[i % 3] for i in range(n_seq)]
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg_for(api)); vo.initalize_projection_matricies(*P); vo.set_clahe(4.0, (4, 4))
    for k in range(2):
        vo.stereo_callback_batch([s[0][k] for s in fed], [s[1][k] for s in fed])
    for i in range(n_seq):
        for cam in (0, 1):
            got, pad = vo.pyramid(i, "t1", cam, 0)
            assert np.array_equal(got, pyramid_ref.padded(ref.clahe_ref(fed[i][cam][1], 4.0, (4, 4)), pad)), (n_seq, i, cam)
    vo.close()


# ------------------------------------------------------------------------------------------------ 4. switching in flight
@pytest.mark.parametrize("n_seq", [1, 9])
def test_switching_with_frames_in_flight(api, n_seq):
    import torch
    L = api._lib
    w, h = SIZES["even"]
    n, depth = 8, 4
    base, P = grey_streams(3, n, 2300, w, h)
    fed = [base[i % 3] for i in range(n_seq)]
    plan = [None, None, (2.0, (8, 8)), (2.0, (8, 8)), (4.0, (4, 4)), (4.0, (4, 4)), None, None]      # the setting each frame is issued with
    plain = [([a if plan[k] is None else eq(a, *plan[k]) for k, a in enumerate(Lq)], [a if plan[k] is None else eq(a, *plan[k]) for k, a in enumerate(Rq)])
             for Lq, Rq in fed]
    cfg = cfg_for(api)
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg); vo.initalize_projection_matricies(*P)
    dev = [[(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in zip(*s)] for s in fed]
    torch.cuda.synchronize()
    rows, paths, sub, cur = [], [], 0, None
    for k in range(n):
        while sub < n and sub - k < depth:
            if plan[sub] != cur:                                      # the setter runs with up to three frames in flight
                cur = plan[sub]
                if cur is None:
                    vo.clear_clahe()
                else:
                    vo.set_clahe(*cur)
            vo.submit_device([dev[i][sub][0].data_ptr() for i in range(n_seq)], [dev[i][sub][1].data_ptr() for i in range(n_seq)], w)
            paths.append(vo.last_frame_path()); sub += 1
        ok, T = vo.collect()
        rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(n_seq)])
    end = [snap(vo, i) for i in range(n_seq)]
    vo.close(); del dev
    assert [bool(p & L.PATH_CLAHE) for p in paths] == [s is not None for s in plan], paths
    route = L.PATH_INGEST_AHEAD if n_seq > 8 else L.PATH_FRONT_FUSED
    assert all(p & route and not p & L.PATH_INPUT_CONVERTED for p in paths), paths
    (want_rows, want_snaps), _ = run(api, w, h, cfg, plain, P, "device", depth=depth)
    for k in range(n):
        for i in range(n_seq):
            assert same_row(rows[k][i], want_rows[k][i]), (k, i)
    assert all(same(end[i], want_snaps[-1][i]) for i in range(n_seq))
    assert any(r[0] for r in rows[-1])


# ------------------------------------------------------------------------------------------------ 5. off is off
@pytest.mark.parametrize("n_seq,mode", [(1, "host"), (9, "device")])
def test_set_and_cleared_equals_never_called(api, n_seq, mode):
    w, h = SIZES["odd"]
    base, P = grey_streams(3, 4, 2400, w, h)
    fed = [base[i % 3] for i in range(n_seq)]
    cfg = cfg_for(api)
    got, paths = run(api, w, h, cfg, fed, P, mode, setup=lambda vo: (vo.set_clahe(3.0, (4, 2)), vo.clear_clahe()))
    want, plain_paths = run(api, w, h, cfg, fed, P, mode)
    assert_runs_equal(got, want, "off")
    assert paths == plain_paths and not any(p & api._lib.PATH_CLAHE for p in paths), (paths, plain_paths)


# ------------------------------------------------------------------------------------------------ 6. errors and edges
def test_setter_errors(api):
    L = api._lib
    w, h = SIZES["even"]
    bgr = api.BatchVisualOdometry(w, h, 1, cfg_for(api, channels=3))
    assert L.lib.svo_set_clahe(bgr._h, 1, 2.0, 8, 8) == L.SVO_ERR_ARG                  # a channels = 3 context
    assert L.lib.svo_set_clahe(bgr._h, 0, 2.0, 8, 8) == L.SVO_ERR_ARG
    bgr.close()
    assert L.lib.svo_set_clahe(None, 1, 2.0, 8, 8) == L.SVO_ERR_ARG
    vo = api.BatchVisualOdometry(w, h, 1, cfg_for(api))
    for tx, ty in [(0, 8), (8, 0), (17, 8), (8, 17)]:
        assert L.lib.svo_set_clahe(vo._h, 1, 2.0, tx, ty) == L.SVO_ERR_ARG
        with pytest.raises(ValueError):
            vo.set_clahe(2.0, (tx, ty))
    for clip in (float("nan"), float("inf")):
        assert L.lib.svo_set_clahe(vo._h, 1, clip, 8, 8) == L.SVO_ERR_ARG
        with pytest.raises(ValueError):
            vo.set_clahe(clip)
    assert L.lib.svo_set_clahe(vo._h, 0, float("nan"), -5, 99) == L.SVO_OK              # on = 0: the other arguments are not looked at
    vo.close()
    small = api.BatchVisualOdometry(16, 17, 1, cfg_for(api, win_w=5, win_h=5))          # rule 1 rejects 16 x 17 with 16 x 16 tiles
    assert L.lib.svo_set_clahe(small._h, 1, 2.0, 16, 16) == L.SVO_ERR_ARG
    assert L.lib.svo_set_clahe(small._h, 1, 2.0, 4, 4) == L.SVO_OK
    small.close()


def test_raw_size_that_rule_1_rejects_fails_the_submit(api):
    """The setter checks the geometry against the input size it sees; a raw size set later is checked when a frame is submitted."""
    L = api._lib
    w, h = SIZES["even"]
    _, P = grey_streams(1, 2, 2500, w, h)
    vo = api.BatchVisualOdometry(w, h, 1, cfg_for(api)); vo.initalize_projection_matricies(*P)
    vo.set_clahe(2.0, (8, 8))
    m1 = np.zeros((h, w, 2), np.int16); m2 = np.zeros((h, w), np.uint16)
    vo.set_rectification_maps(m1, m2, m1, m2, raw_size=(8, 9))
    raw = np.zeros((9, 8), np.uint8)
    lp = (C.c_void_p * 1)(raw.ctypes.data); rp = (C.c_void_p * 1)(raw.ctypes.data)
    T = np.zeros(16); ok = np.zeros(1, np.int32)
    assert L.lib.svo_process_batch(vo._h, lp, rp, 8, 0, L.ptr(T), L.ptr(ok), None) == L.SVO_ERR_STATE
    assert L.lib.svo_set_clahe(vo._h, 1, 2.0, 8, 8) == L.SVO_ERR_ARG                    # ... and the setter now sees the raw size
    vo.clear_clahe()
    assert L.lib.svo_process_batch(vo._h, lp, rp, 8, 0, L.ptr(T), L.ptr(ok), None) == L.SVO_OK
    vo.close()


def test_setter_before_the_first_frame_and_member_circular_matching(api):
    """VisualOdometry.set_clahe before the context exists is applied at creation; svo_circular_matching equalises its images too."""
    w, h = SIZES["odd"]
    base, P = grey_streams(1, 3, 2600, w, h)
    outs = []
    for streams, clahe in ((base, True), (eq_streams(base, 3.0, (6, 4)), False)):
        (Lq, Rq), = streams
        vo = api.VisualOdometry(cfg=cfg_for(api)); vo.initalize_projection_matricies(*P)
        if clahe:
            with pytest.raises(ValueError):
                vo.set_clahe(2.0, (0, 3))                             # checked at once, not inside the first frame
            vo.set_clahe(3.0, (6, 4))
        ok0, _ = vo.stereo_callback(Lq[0], Rq[0])
        assert bool(vo.last_frame_path() & api._lib.PATH_CLAHE) == clahe
        fs = api.FeatureSet()
        pts = np.stack(np.meshgrid(np.linspace(8, w - 8, 12), np.linspace(8, h - 8, 9)), -1).reshape(-1, 2).astype(np.float32)
        fs.points, fs.ages, fs.strengths = pts.copy(), np.zeros(len(pts), np.int32), np.ones(len(pts), np.int32)
        res = vo.circularMatching(Lq[1], Rq[1], pts, fs)
        ok, T = vo.stereo_callback(Lq[2], Rq[2])
        outs.append([raw_bits(np.ascontiguousarray(a)) for a in res] + [raw_bits(fs.points), np.asarray(T).view(np.uint64), np.array([ok])])
        vo.close()
    assert len(outs[0][0]) > 20 and same(outs[0], outs[1])
