"""Input formats on a real GPU (include/svo.h, input-format section): colour and YUV 4:2:2 frames converted to mono8 inside
frame ingest.

The conversion kernel is pinned to the numpy restatement (tests/input_format_ref.py) bit for bit.  A converting context fed
colour frames must give exactly what a plain context gives when fed the numpy-grey frames — pyramids with their borders, rows,
statistics, feature sets and tracks — on every route into the pyramid (lone-stream fused front, many-sequence launches,
build-ahead image stream, masked frames, the member circularMatching, rectifying contexts, replayed graphs; host, pinned and
device inputs).  The format is stream-ordered like svo_clear_rectification."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_run1
import input_format_ref as ref
import pyramid_ref
import rectify_ref
import test_gpu_rectify as tr
from test_gpu_rectify import assert_runs_equal, row, same_row
from gpu_kit import api, calib, raw_bits, run_child, same, snap, streams  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"even": (320, 160), "odd": (323, 163)}       # the odd one: full and partial tiles at both tile shapes, edge tiles on all four sides


_grey_cache = {}


def grey_streams(n_seq, n_frames, seed0, w, h):
    """n_seq independent synthetic grey sequences of w x h (rendered once per argument set, never written to)."""
    key = (n_seq, n_frames, seed0, w, h)
    if key not in _grey_cache:
        from stereo_visual_odometry_amd import synthetic as syn
        cal = dict(calib(w, h), fx=300.0, fy=300.0)
        _grey_cache[key] = (streams(n_seq, n_frames, seed0, w, h, cal=cal), syn.projection_matrices(cal))
    return _grey_cache[key]


def coloured(streams, fmt, seed=7):
    """-> (the streams in `fmt`, their numpy-grey streams)."""
    rng = np.random.default_rng(seed)
    col, grey = [], []
    for L, R in streams:
        cl, cr = [ref.colour_of(a, fmt, rng) for a in L], [ref.colour_of(a, fmt, rng) for a in R]
        col.append(([c[0] for c in cl], [c[0] for c in cr]))
        grey.append(([c[1] for c in cl], [c[1] for c in cr]))
    return col, grey


def run(api, w, h, cfg, streams, P, mode, fmt=None, setup=None, depth=2, masks=None):
    """A len(streams)-sequence w x h context over every frame -> (rows [frame][seq], snapshots [frame][seq] (device inputs: only
    the last), svo_get_last_frame_path after each frame's issue).  mode: host / pinned / device (submitted `depth` ahead).
    masks: per frame, None or n_seq flags (host mode; an idle sequence's images are passed as None)."""
    B = len(streams)
    vo = api.BatchVisualOdometry(w, h, B, cfg)
    vo.initalize_projection_matricies(*P)
    if setup:
        setup(vo)
    if fmt:
        vo.set_input_format(fmt)
    n = len(streams[0][0])
    rows, snaps, paths = [], [], []
    if mode == "device":
        import torch
        dev = [[(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in zip(*s)] for s in streams]
        torch.cuda.synchronize()
        stride = streams[0][0][0].strides[0]
        sub = 0
        for k in range(n):
            while sub < n and sub - k < depth:
                vo.submit_device([dev[i][sub][0].data_ptr() for i in range(B)], [dev[i][sub][1].data_ptr() for i in range(B)], stride)
                paths.append(vo.last_frame_path()); sub += 1
            ok, T = vo.collect()
            rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(B)])
            snaps.append(None)
        snaps[-1] = [snap(vo, i) for i in range(B)]
        del dev
    else:
        for k in range(n):
            act = masks[k] if masks else None
            on = [True] * B if act is None else [bool(x) for x in act]
            Ls = [s[0][k] if o else None for s, o in zip(streams, on)]; Rs = [s[1][k] if o else None for s, o in zip(streams, on)]
            if mode == "pinned":
                pin = [api.PinnedImage(a.shape) for a in Ls + Rs]
                for p, a in zip(pin, Ls + Rs):
                    p.array[...] = a
                Ls, Rs = [p.array for p in pin[:B]], [p.array for p in pin[B:]]
            ok, T = vo.stereo_callback_batch(Ls, Rs, active=act)
            paths.append(vo.last_frame_path())
            rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(B)])
            snaps.append([snap(vo, i) for i in range(B)])
    vo.close()
    return (rows, snaps), paths


def cfg_for(api, **over):
    return api.default_config(max_translation_norm=2.0, **over)


# ------------------------------------------------------------------------------------------------ 1. the conversion alone
def strided(frame, extra, offset):
    """The frame's bytes inside a larger array: rows `extra` bytes longer than they need to be, starting `offset` bytes in."""
    a = frame if frame.ndim == 3 else frame[..., None]
    h, w, bpp = a.shape
    stride = w * bpp + extra
    buf = np.full(offset + h * stride + 3, 0xA5, np.uint8)
    v = np.ndarray(a.shape, np.uint8, buffer=buf, offset=offset, strides=(stride, bpp, 1))
    v[...] = a
    return v if frame.ndim == 3 else v[..., 0]


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_convert_gray_equals_numpy(api, fmt):
    rng = np.random.default_rng(11)
    for w, h in [(1, 1), (3, 2), (67, 19), (131, 35), (333, 147)]:
        shape = (h, w) if fmt == "mono8" else (h, w, ref.BPP[fmt])
        frame = rng.integers(0, 256, shape).astype(np.uint8)
        frame.reshape(-1)[:3] = 255                                   # a saturated pixel: the sum reaches its maximum
        want = ref.to_grey(frame, fmt)
        for extra, offset in [(0, 0), (5, 0), (0, 1), (5, 3)]:
            got = api.convertGray(strided(frame, extra, offset), fmt)
            assert np.array_equal(got, want), (fmt, w, h, extra, offset)


def test_convert_gray_every_colour_value(api):
    """Every value of every channel against every weight: 256 x 3 single-channel ramps, and a random cube sample."""
    rng = np.random.default_rng(12)
    f = rng.integers(0, 256, (64, 256, 3)).astype(np.uint8)
    for c in range(3):
        f[c, :, :] = 0; f[c, :, c] = np.arange(256); f[3 + c, :, :] = 255; f[3 + c, :, c] = np.arange(256)
    for fmt in ("bgr8", "rgb8"):
        assert np.array_equal(api.convertGray(f, fmt), ref.to_grey(f, fmt)), fmt


# ------------------------------------------------------------------------------------------------ 2. pyramids and borders
@pytest.mark.parametrize("n_seq", [1, 9])
@pytest.mark.parametrize("fmt", ["bgr8", "bgra8", "yuv422"])
def test_pyramids_of_colour_frames(api, fmt, n_seq):
    w, h = SIZES["odd"]
    base, P = grey_streams(3, 2, 500, w, h)
    col, grey = coloured([base[i % 3] for i in range(n_seq)], fmt, seed=20 + n_seq)
    cfg = cfg_for(api)
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg); vo.initalize_projection_matricies(*P); vo.set_input_format(fmt)
    for k in range(2):
        vo.stereo_callback_batch([s[0][k] for s in col], [s[1][k] for s in col])
        assert vo.last_frame_path() & api._lib.PATH_INPUT_CONVERTED
    nl = vo.pyramid_levels()
    assert nl == 4
    for i in range(n_seq):
        for cam in (0, 1):
            want = pyramid_ref.pyramid(grey[i][cam][1], cfg.win_w, cfg.max_level)
            assert len(want) == nl
            for lv in range(nl):
                got, pad = vo.pyramid(i, "t1", cam, lv)
                assert np.array_equal(got, pyramid_ref.padded(want[lv], pad)), (fmt, n_seq, i, cam, lv)
    vo.close()


# ------------------------------------------------------------------------------------------------ 3. the whole pipeline
EQUAL = [  # n_seq, input, size, format
    (1, "host", "even", "bgr8"), (1, "pinned", "odd", "bgra8"), (1, "device", "odd", "yuv422"), (1, "host", "odd", "rgb8"),
    (1, "device", "even", "yuv422_yuy2"), (9, "device", "even", "bgr8"), (9, "device", "odd", "rgba8"), (9, "device", "odd", "yuv422"),
]


@pytest.mark.parametrize("n_seq,mode,size,fmt", EQUAL)
def test_converting_context_equals_plain_on_grey(api, n_seq, mode, size, fmt):
    w, h = SIZES[size]
    base, P = grey_streams(3 if n_seq > 1 else 1, 5, 1000 + n_seq, w, h)
    col, grey = coloured([base[i % len(base)] for i in range(n_seq)], fmt, seed=30 + n_seq)
    cfg = cfg_for(api)
    got, paths = run(api, w, h, cfg, col, P, mode, fmt=fmt)
    want, plain_paths = run(api, w, h, cfg, grey, P, "host" if mode != "device" else "device")
    assert_runs_equal(got, want, "%s %s" % (fmt, mode))
    L = api._lib
    route = L.PATH_INGEST_AHEAD if n_seq > 8 else L.PATH_FRONT_FUSED
    assert all(p & route and p & L.PATH_INPUT_CONVERTED for p in paths), paths
    assert all(p & route and not p & L.PATH_INPUT_CONVERTED for p in plain_paths), plain_paths
    assert any(r[0] for r in got[0][-1]), "no pose in the last frame: the test would not see tracking differences"


def test_masked_frames(api):
    w, h = SIZES["odd"]
    n_seq, n = 9, 5
    base, P = grey_streams(3, n, 1200, w, h)
    col, grey = coloured([base[i % 3] for i in range(n_seq)], "bgr8", seed=41)
    rng = np.random.default_rng(42)
    masks = [None] + [(rng.random(n_seq) < 0.6) for _ in range(n - 1)]
    masks[2] = np.zeros(n_seq, bool)                                  # an all-idle frame
    cfg = cfg_for(api)
    got, paths = run(api, w, h, cfg, col, P, "host", fmt="bgr8", masks=masks)
    want, _ = run(api, w, h, cfg, grey, P, "host", masks=masks)
    assert_runs_equal(got, want, "masked")
    assert paths[2] == 0 and all(p & api._lib.PATH_INPUT_CONVERTED for k, p in enumerate(paths) if k != 2), paths
    assert any(r[2]["fail_reason"] == 5 for fr in got[0] for r in fr) and any(r[0] for r in got[0][-1])


def test_format_switch_with_frames_in_flight(api):
    import torch
    w, h = SIZES["even"]
    n_seq, n, cut = 9, 6, 2
    base, P = grey_streams(3, n, 1300, w, h)
    col, grey = coloured([base[i % 3] for i in range(n_seq)], "bgr8", seed=51)
    cfg = cfg_for(api)
    L = api._lib
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg); vo.initalize_projection_matricies(*P)
    up = lambda streams: [[(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in zip(*s)] for s in streams]
    dg, dc = up(grey), up(col)
    torch.cuda.synchronize()

    def submit(dev, k, bpp):
        vo.submit_device([dev[i][k][0].data_ptr() for i in range(n_seq)], [dev[i][k][1].data_ptr() for i in range(n_seq)], w * bpp)
        return vo.last_frame_path()
    paths = [submit(dg, k, 1) for k in range(cut)]                    # mono8 frames in flight ...
    vo.set_input_format("bgr8")                                      # ... the format changes behind them ...
    paths += [submit(dc, k, 3) for k in range(cut, n - 1)]
    vo.set_input_format("mono8")                                     # ... and back, still with frames in flight
    paths.append(submit(dg, n - 1, 1))
    rows = []
    for k in range(n):
        ok, T = vo.collect()
        rows.append([row(ok[i], T[i], vo.stats[i]) for i in range(n_seq)])
    end = [snap(vo, i) for i in range(n_seq)]
    vo.close(); del dg, dc
    conv = [bool(p & L.PATH_INPUT_CONVERTED) for p in paths]
    assert conv == [False] * cut + [True] * (n - 1 - cut) + [False], paths
    (want_rows, want_snaps), _ = run(api, w, h, cfg, grey, P, "device", depth=n)
    for k in range(n):
        for i in range(n_seq):
            assert same_row(rows[k][i], want_rows[k][i]), (k, i)
    assert all(same(end[i], want_snaps[-1][i]) for i in range(n_seq))
    assert any(r[0] for r in rows[-1])


def test_member_circular_matching_with_a_format(api):
    w, h = SIZES["odd"]
    base, P = grey_streams(1, 3, 1400, w, h)
    col, grey = coloured(base, "bgra8", seed=61)
    outs = []
    for streams, fmt in ((col, "bgra8"), (grey, None)):
        (L, R), = streams
        vo = api.VisualOdometry(cfg=cfg_for(api)); vo.initalize_projection_matricies(*P)
        if fmt:
            vo.set_input_format(fmt)                                  # before the context exists: applied at creation
        vo.stereo_callback(L[0], R[0])
        fs = api.FeatureSet()
        pts = np.stack(np.meshgrid(np.linspace(8, w - 8, 12), np.linspace(8, h - 8, 9)), -1).reshape(-1, 2).astype(np.float32)
        fs.points, fs.ages, fs.strengths = pts.copy(), np.zeros(len(pts), np.int32), np.ones(len(pts), np.int32)
        res = vo.circularMatching(L[1], R[1], pts, fs)
        ok, T = vo.stereo_callback(L[2], R[2])
        outs.append([raw_bits(np.ascontiguousarray(a)) for a in res] + [raw_bits(fs.points), np.asarray(T).view(np.uint64), np.array([ok])])
        if fmt:
            with pytest.raises(ValueError):
                vo.circularMatching(grey[0][0][1], grey[0][1][1], pts, fs)      # a grey frame is not a bgra8 frame
        vo.close()
    assert len(outs[0][0]) > 20 and same(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 4. conversion, then remap
@pytest.mark.parametrize("n_seq,mode", [(1, "host"), (9, "device")])
@pytest.mark.parametrize("fmt", ["bgr8", "yuv422"])
def test_rectifying_converting_context(api, fmt, n_seq, mode):
    pair = tr.cam_pair(0)
    mp = tr.maps_of(pair)
    base = tr.raw_streams(3 if n_seq > 1 else 1, 4, 1500 + n_seq)
    col, grey = coloured([base[i % len(base)] for i in range(n_seq)], fmt, seed=71)
    P = tr.projections(pair)
    cfg = cfg_for(api)
    got, paths = run(api, tr.W, tr.H, cfg, col, P, mode, fmt=fmt, setup=lambda vo: vo.set_rectification(pair[0], pair[1]))
    rect = [([rectify_ref.remap(a, *mp[0]) for a in L], [rectify_ref.remap(a, *mp[1]) for a in R]) for L, R in grey]
    want, _ = run(api, tr.W, tr.H, cfg, rect, P, mode)
    assert_runs_equal(got, want, "rectifying %s" % fmt)
    L = api._lib
    assert all(p & L.PATH_INPUT_CONVERTED and p & (L.PATH_INGEST_AHEAD if n_seq > 8 else L.PATH_FRONT_FUSED) for p in paths), paths
    assert any(r[0] for r in got[0][-1])


# ------------------------------------------------------------------------------------------------ 5. replayed graphs
def test_graph_mode_gives_the_same_results(api, tmp_path):
    """SVO_GRAPH=1 in a fresh process (the variable is read when a context is created): a lone and a 9-sequence converting run
    equal the launch-list runs of this process."""
    import input_format_child as child
    out = tmp_path / "graph.npz"
    env = dict(os.environ, SVO_GRAPH="1")
    p = run_child("input_format_child.py", out, env=env)
    assert "input format child ok" in p.stdout, p.stdout + p.stderr
    d = np.load(out)
    L = api._lib
    for name, n_seq, mode, fmt in child.RUNS:
        (rows, _), paths = child.one_run(api, run, grey_streams, coloured, cfg_for, n_seq, mode, fmt)
        T = np.array([[r[1] for r in fr] for fr in rows]); ok = np.array([[r[0] for r in fr] for fr in rows])
        st = np.array([[list(r[2].values()) for r in fr] for fr in rows])
        assert np.array_equal(d[name + "_T"], T) and np.array_equal(d[name + "_ok"], ok) and np.array_equal(d[name + "_stats"], st), name
        assert all(p & L.PATH_GRAPH and p & L.PATH_INPUT_CONVERTED for p in d[name + "_paths"]), (name, d[name + "_paths"])
        assert not any(p & L.PATH_GRAPH for p in paths)
        assert ok[-1].any()


# ------------------------------------------------------------------------------------------------ 6. the reference's frames
def test_run1_colour_frames_as_bgr8(api):
    from stereo_visual_odometry_amd import synthetic as syn
    left, right = golden_run1.bgr_frames(8)
    d = np.load(os.path.join(ROOT, "tests", "golden", "run1_frames_0_7.npz"))
    P = syn.projection_matrices(syn.RUN1)
    w, h = syn.RUN1["width"], syn.RUN1["height"]
    cfg = api.default_config()                                        # the run1 configuration of test_run1_cli.py: reference defaults
    col = [([left[k] for k in range(8)], [right[k] for k in range(8)])]
    grey = [([d["left"][k] for k in range(8)], [d["right"][k] for k in range(8)])]
    got, paths = run(api, w, h, cfg, col, P, "host", fmt="bgr8")
    want, _ = run(api, w, h, cfg, grey, P, "host")
    assert_runs_equal(got, want, "run1")
    assert all(p & api._lib.PATH_INPUT_CONVERTED for p in paths) and any(r[0][0] for r in got[0])
    vo = api.BatchVisualOdometry(w, h, 1, cfg); vo.initalize_projection_matricies(*P); vo.set_input_format("bgr8")
    vo.stereo_callback_batch([left[7]], [right[7]])
    for cam in (0, 1):
        lv0, pad = vo.pyramid(0, "t1", cam, 0)
        assert np.array_equal(lv0[pad:-pad, pad:-pad], d["right" if cam else "left"][7])
    vo.close()


# ------------------------------------------------------------------------------------------------ 7. edges
def test_setter_and_stride_errors(api):
    L = api._lib
    w, h = SIZES["even"]
    _, P = grey_streams(1, 3, 1400, *SIZES["odd"])
    bgr = api.BatchVisualOdometry(w, h, 1, cfg_for(api, channels=3))
    assert L.lib.svo_set_input_format(bgr._h, L.INPUT_BGR8) == L.SVO_ERR_ARG           # a channels = 3 context has no input format
    assert L.lib.svo_set_input_format(bgr._h, L.INPUT_MONO8) == L.SVO_ERR_ARG
    bgr.close()
    vo = api.BatchVisualOdometry(w, h, 1, cfg_for(api)); vo.initalize_projection_matricies(*P)
    for bad in (7, -1):
        assert L.lib.svo_set_input_format(vo._h, bad) == L.SVO_ERR_ARG
        with pytest.raises(ValueError):
            vo.set_input_format(bad)
    with pytest.raises(ValueError):
        vo.set_input_format("bayer_rggb8")
    vo.set_input_format("bgr8")
    img = np.zeros((h, w, 3), np.uint8)
    lp = (C.c_void_p * 1)(img.ctypes.data); rp = (C.c_void_p * 1)(img.ctypes.data)
    T = np.zeros(16); ok = np.zeros(1, np.int32)
    assert L.lib.svo_process_batch(vo._h, lp, rp, w * 3 - 1, 0, L.ptr(T), L.ptr(ok), None) == L.SVO_ERR_ARG       # one byte short
    assert L.lib.svo_process_batch(vo._h, lp, rp, w * 3, 0, L.ptr(T), L.ptr(ok), None) == L.SVO_OK
    vo.set_input_format("yuv422")
    assert L.lib.svo_process_batch(vo._h, lp, rp, w * 2 - 1, 0, L.ptr(T), L.ptr(ok), None) == L.SVO_ERR_ARG
    with pytest.raises(ValueError):
        vo.stereo_callback_batch([img], [img])                        # three channels where the format has two
    with pytest.raises(ValueError):
        vo.stereo_callback_batch([img[:, :, 0]], [img[:, :, 0]])      # a grey frame where the format has two
    bad = np.zeros((5, 5, 3), np.uint8)
    assert L.lib.svo_convert_gray(0, 7, L.ptr(bad), 5, 5, 15, L.ptr(bad)) == L.SVO_ERR_ARG
    assert L.lib.svo_convert_gray(0, L.INPUT_BGR8, L.ptr(bad), 5, 5, 14, L.ptr(bad)) == L.SVO_ERR_ARG
    with pytest.raises(ValueError):
        api.convertGray(bad, "bgra8")
    vo.close()
    lone = api.VisualOdometry(cfg=cfg_for(api)); lone.initalize_projection_matricies(*P); lone.set_input_format("rgb8")
    with pytest.raises(ValueError):
        lone.stereo_callback(img[:, :, 0], img[:, :, 0])
    lone.close()


# ------------------------------------------------------------------------------------------------ 8. CLI and C++ facade
def test_cli_gray_2_prints_the_rows_of_gray_1(tmp_path):
    from PIL import Image
    from test_run1_cli import build_cli
    left, right = golden_run1.bgr_frames(8)
    folder = tmp_path / "run1"
    (folder / "left").mkdir(parents=True); (folder / "right").mkdir()
    for k in range(8):
        Image.fromarray(left[k][..., ::-1]).save(folder / "left" / ("frame%06d.png" % k))       # RGB PNG files, as in run1/
        Image.fromarray(right[k][..., ::-1]).save(folder / "right" / ("frame%06d.png" % k))
    exe = build_cli()
    text = {}
    for g in ("1", "2"):
        res = tmp_path / ("result%s.csv" % g)
        out = subprocess.run([exe, "400", str(folder), "--gray", g, "--out", str(res)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "processed 8 frame pairs" in out.stdout, out.stdout + out.stderr
        text[g] = (res.read_text(), [ln for ln in out.stdout.split("\n") if ln.startswith("Frame")])
    assert text["1"] == text["2"] and len(text["1"][1]) == 8
    assert any("ok=1" in ln for ln in text["2"][1])


def test_cpp_facade_input_encoding(tmp_path):
    base, P = grey_streams(1, 4, 1600, *SIZES["even"])
    col, grey = coloured(base, "bgra8", seed=81)
    w, h = SIZES["even"]
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([4, h, w], np.int32).tobytes())
        f.write(np.ascontiguousarray(P[0], np.float32).tobytes()); f.write(np.ascontiguousarray(P[1], np.float32).tobytes())
        for k in range(4):
            for a in (grey[0][0][k], grey[0][1][k], col[0][0][k], col[0][1][k]):
                f.write(a.tobytes())
    exe = os.path.join(ROOT, "tests", "cpp", "input_format_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "input_format_test.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "INPUT FORMAT OK" in out.stdout, out.stdout + out.stderr
