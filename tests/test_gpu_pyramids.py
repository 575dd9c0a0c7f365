"""The pyramids the frame pipeline builds, byte for byte, border included (svo_get_pyramid).

Every case builds frames with the library, reads back the T1 pyramids (and lastLeftPyramid's pair) of every sequence, camera,
level and colour plane WITH the stored REFLECT_101 border, and compares every byte with tests/pyramid_ref.py applied to the
frame's own images.  Each case asserts through svo_get_last_frame_path that the route it names really ran:
- fused:  the lone-stream fused front (k_front_a / k_front_b), SVO_PATH_FRONT_FUSED
- pyr1:   a lone stream's k_ingest_pyr1 (2-3 levels, or features_per_bucket > 1), neither bit
- ahead:  the many-sequence build-ahead on the image stream, SVO_PATH_INGEST_AHEAD, 1-3 frames in flight
- many:   the many-sequence k_ingest_pyr1 without build-ahead (a child process with SVO_INGEST_AHEAD=0), neither bit
- one:    a one-level pyramid (k_ingest<1>), neither bit
- bgr:    channels = 3 (k_ingest<3>, one pyramid per plane), neither bit
and each of them rectifying (the RECT = true instantiations; reference = the pyramid of rectify_ref.remap(raw)).
Inputs: host frames packed and with wide rows, pinned frames, device frames with rows 0, 1, 3 and 64 bytes wider than the
image (0xAB in the gap)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pyramid_ref as ref
import rectify_ref
from gpu_kit import api, projections, run_child  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

RAW_W, RAW_H = 344, 180          # raw frames of the rectifying cases (test_gpu_rectify.cam_pair)


def lk_pad_for(win):
    """The border the library stores around every level (svo_kernels_lk.hip lk_pad_for), restated for the coverage check."""
    ppl = next(p for p in range(1, win + 1) if win * -(-win // p) <= 64)
    return (-(-win // ppl) * ppl + 5 + 3) & ~3


# ------------------------------------------------------------------------------------------------------------- the case matrix
# (route, (w, h), win, max_level, n_seq, input, extra): input = host | stride (host, wide rows) | pinned | dev+K (device frames,
# rows K bytes wider; depth = frames kept in flight); extra: rect, fpb (features_per_bucket), depth
CASES = [
    ("fused", (417, 203), 10, 3, 1, "host", {}),
    ("fused", (418, 202), 7, 4, 2, "pinned", {}),
    ("fused", (419, 201), 10, 5, 1, "dev+1", {}),
    ("fused", (420, 200), 5, 5, 3, "stride", {}),
    ("fused", (1241, 376), 21, 4, 1, "host", {}),
    ("fused", (1241, 376), 31, 3, 1, "pinned", {}),
    ("fused", (255, 129), 15, 4, 1, "dev+3", {}),
    ("fused", (130, 66), 7, 3, 1, "dev+64", {}),
    ("fused", (90, 46), 5, 3, 1, "host", {}),
    ("fused", (90, 46), 5, 3, 8, "dev+1", {}),
    ("fused", (322, 161), 10, 3, 1, "host", {"rect": 1}),
    ("fused", (90, 46), 5, 3, 2, "dev+3", {"rect": 1}),
    ("pyr1", (67, 35), 5, 3, 1, "host", {}),
    ("pyr1", (165, 83), 15, 5, 2, "dev+1", {}),
    ("pyr1", (418, 202), 31, 2, 1, "stride", {}),
    ("pyr1", (130, 66), 15, 1, 4, "pinned", {}),
    ("pyr1", (1241, 376), 21, 2, 1, "dev+64", {}),
    ("pyr1", (417, 203), 10, 3, 1, "host", {"fpb": 3}),
    ("pyr1", (90, 46), 5, 3, 1, "dev+3", {"fpb": 3}),
    ("pyr1", (255, 129), 15, 5, 1, "host", {"fpb": 3}),
    ("pyr1", (319, 158), 7, 2, 1, "host", {"rect": 1}),
    ("pyr1", (322, 161), 10, 3, 1, "dev+1", {"rect": 1, "fpb": 3}),
    ("ahead", (417, 203), 10, 3, 9, "host", {}),
    ("ahead", (419, 201), 7, 5, 10, "dev+3", {"depth": 2}),
    ("ahead", (420, 200), 21, 3, 9, "dev+1", {"depth": 3}),
    ("ahead", (90, 46), 5, 3, 12, "pinned", {}),
    ("ahead", (1241, 376), 21, 4, 9, "dev+0", {"depth": 1}),
    ("ahead", (255, 129), 15, 4, 9, "stride", {}),
    ("ahead", (165, 83), 15, 5, 9, "dev+64", {"depth": 2}),
    ("ahead", (67, 35), 5, 3, 10, "dev+1", {"depth": 3}),
    ("ahead", (130, 66), 31, 5, 9, "host", {}),
    ("ahead", (322, 161), 10, 3, 9, "dev+3", {"rect": 1, "depth": 2}),
    ("ahead", (90, 46), 5, 3, 9, "host", {"rect": 1}),
    ("one", (417, 203), 10, 0, 1, "host", {}),
    ("one", (419, 201), 7, 0, 1, "dev+1", {}),
    ("one", (67, 35), 31, 3, 1, "stride", {}),
    ("one", (1241, 376), 21, 0, 9, "dev+3", {"depth": 2}),
    ("one", (90, 46), 31, 3, 10, "pinned", {}),
    ("one", (321, 163), 10, 0, 1, "host", {"rect": 1}),
    ("one", (322, 161), 15, 0, 9, "dev+1", {"rect": 1}),
    ("bgr", (417, 203), 10, 3, 1, "host", {}),
    ("bgr", (90, 46), 5, 3, 1, "dev+1", {}),
    ("bgr", (419, 201), 7, 2, 10, "dev+3", {"depth": 2}),
    ("bgr", (1241, 376), 21, 4, 1, "pinned", {}),
    ("bgr", (67, 35), 5, 0, 10, "stride", {}),
    ("bgr", (165, 83), 15, 5, 10, "host", {}),
    ("bgr", (322, 161), 10, 3, 1, "host", {"rect": 1}),
    ("bgr", (90, 46), 5, 3, 10, "dev+64", {"rect": 1}),
]
# the many-sequence k_ingest_pyr1 without build-ahead: SVO_INGEST_AHEAD is read once per process, so these run in a child
MANY_CASES = [
    ("many", (418, 202), 7, 4, 9, "host", {}),
    ("many", (90, 46), 5, 3, 10, "dev+1", {"depth": 2}),
    ("many", (319, 158), 10, 3, 9, "pinned", {"rect": 1}),
    ("many", (1241, 376), 21, 4, 9, "stride", {}),
    ("many", (165, 83), 15, 5, 9, "dev+3", {}),
]


def case_id(c):
    route, (w, h), win, ml, B, inp, ex = c
    return "%s-%dx%d-w%d-l%d-B%d-%s%s" % (route, w, h, win, ml, B, inp, "".join("-%s%s" % kv for kv in sorted(ex.items())))


def test_case_matrix_covers_the_edges():
    """The level chains of the matrix hold every width residue mod 4, levels narrower and shorter than the pad, and a level no
    wider or taller than (pad + 1) / 2 (where the left / top border folds twice): later edits cannot make the matrix vacuous."""
    residues, narrow, short, fold = set(), False, False, False
    for route, (w, h), win, ml, B, inp, ex in CASES + MANY_CASES:
        pad = lk_pad_for(win)
        sizes = ref.level_sizes(w, h, win, ml)
        if route == "fused":
            assert len(sizes) >= 4
        elif route in ("pyr1", "ahead", "many"):
            assert len(sizes) >= 2 and (route != "pyr1" or len(sizes) <= 3 or ex.get("fpb", 1) > 1)
        elif route == "one":
            assert len(sizes) == 1
        for lw, lh in sizes:
            residues.add(lw % 4)
            narrow |= lw <= pad
            short |= lh <= pad
            fold |= min(lw, lh) <= (pad + 1) // 2
    assert residues == {0, 1, 2, 3} and narrow and short and fold
    routes = {c[0] for c in CASES + MANY_CASES}
    assert routes == {"fused", "pyr1", "ahead", "many", "one", "bgr"}
    assert all(any(c[0] == r and c[6].get("rect") for c in CASES + MANY_CASES) for r in routes)
    assert {c[6].get("depth", 1) for c in CASES if c[0] == "ahead" and c[5].startswith("dev")} == {1, 2, 3}
    assert {c[5] for c in CASES} >= {"host", "stride", "pinned", "dev+0", "dev+1", "dev+3", "dev+64"}


# ------------------------------------------------------------------------------------------------------------------ frames
def texture(w, h, seed, cn=1):
    """Noise over a smooth pattern: FAST finds corners everywhere, and every tap of the 5x5 kernel matters."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(x / (5.0 + seed % 7) + seed) * np.cos(y / 6.0)
    img = np.clip(base + rng.integers(-70, 71, (h, w)), 0, 255).astype(np.uint8)
    if cn == 3:
        img = np.ascontiguousarray(np.stack([img, np.roll(img, 3, 1), 255 - np.roll(img, 2, 0)], -1))
    return img


def make_stream(w, h, n, seed, cn=1, black=()):
    """n stereo pairs; the right view is the left one shifted, the next frame moves a little.  Frames in `black` are all zero."""
    assert n <= 16
    base = texture(w + 2 * n + 6, h + n, seed, cn)
    L, R = [], []
    for k in range(n):
        a = np.ascontiguousarray(base[k:k + h, 2 * k:2 * k + w])
        b = np.ascontiguousarray(base[k:k + h, 2 * k + 6:2 * k + 6 + w])
        if k in black:
            a, b = np.zeros_like(a), np.zeros_like(b)
        L.append(a); R.append(b)
    return L, R


class Ctx:
    """A context of one case plus what the reference needs: the rectification maps and a cache of reference pyramids."""

    def __init__(self, api, w, h, win, ml, B, cn=1, rect=False, fpb=1, facade=False):
        self.api, self.w, self.h, self.win, self.ml, self.B, self.cn = api, w, h, win, ml, B, cn
        cfg = api.default_config(win_w=win, win_h=win, max_level=ml, max_translation_norm=2.0, channels=cn, features_per_bucket=fpb)
        self.maps = None
        if facade:
            self.vo = api.VisualOdometry(w, h, cfg)
        else:
            self.vo = api.BatchVisualOdometry(w, h, B, cfg)
        self.vo.initalize_projection_matricies(*projections(w, h))
        if rect:
            from test_gpu_rectify import cam_pair
            pair = cam_pair(1)
            self.vo.set_rectification(*pair)
            self.maps = [rectify_ref.init_rectify_map(c["K"], c["D"], c["R"], c["P"], w, h) for c in pair]
        self._ref = {}

    def in_size(self):
        return (RAW_W, RAW_H) if self.maps else (self.w, self.h)

    def reference(self, img, cam):
        key = (id(img), cam)
        if key not in self._ref:
            self._ref[key] = (img, ref.pyramids(img, self.win, self.ml, self.maps[cam] if self.maps else None))
        return self._ref[key][1]

    def read(self, seq, which):
        """{(cam, plane, level): padded level} of one stored pyramid pair."""
        n = self.vo.pyramid_levels()
        out = {}
        for cam in range(2):
            for plane in range(self.cn):
                for lv in range(n):
                    out[cam, plane, lv] = self.vo.pyramid(seq, which, cam, lv, plane)
        return out

    def check(self, seq, which, pair, what):
        """Every byte of the stored pyramids `which` of `seq` against the reference pyramids of the stereo pair `pair`."""
        n = self.vo.pyramid_levels()
        for cam, img in enumerate(pair):
            want = self.reference(img, cam)
            assert len(want) == self.cn and len(want[0]) == n, (what, "levels", n, len(want[0]))
            for plane in range(self.cn):
                for lv in range(n):
                    got, pad = self.vo.pyramid(seq, which, cam, lv, plane)
                    assert pad == lk_pad_for(self.win)
                    exp = ref.padded(want[plane][lv], pad)
                    if not np.array_equal(got, exp):
                        ys, xs = np.nonzero(got != exp)
                        lh, lw = want[plane][lv].shape
                        inner = ((ys >= pad) & (ys < pad + lh) & (xs >= pad) & (xs < pad + lw)).sum()
                        pytest.fail("%s: seq %d %s cam %d plane %d level %d (%dx%d, pad %d): %d bytes differ (%d inside the level), "
                                    "first at (x, y) = %s" % (what, seq, which, cam, plane, lv, lw, lh, pad, len(ys), inner,
                                                              list(zip((xs[:6] - pad).tolist(), (ys[:6] - pad).tolist()))))

    def close(self):
        self.vo.close()


def host_strided(api, vo, Ls, Rs, extra, active=None):
    """svo_process_batch(_masked) on host frames whose rows are `extra` bytes wider than the image (0xAB in the gap)."""
    from stereo_visual_odometry_amd import _lib
    B = vo.n_seq
    bufs, stride = [], None
    for a in Ls + Rs:
        if a is None:
            bufs.append(None); continue
        rows = a.reshape(a.shape[0], -1)
        b = np.full((rows.shape[0], rows.shape[1] + extra), 0xAB, np.uint8)
        b[:, :rows.shape[1]] = rows
        bufs.append(b); stride = b.shape[1]
    ptrs = [b.ctypes.data if b is not None else None for b in bufs]
    lp, rp = (C.c_void_p * B)(*ptrs[:B]), (C.c_void_p * B)(*ptrs[B:])
    T = np.zeros((B, 16)); ok = np.zeros(B, np.int32); st = (_lib.SvoFrameStats * B)()
    if active is None:
        _lib.check(_lib.lib.svo_process_batch(vo._h, lp, rp, stride, 0, _lib.ptr(T), _lib.ptr(ok), st))
    else:
        act = np.ascontiguousarray(np.asarray(active, bool), np.uint8)
        _lib.check(_lib.lib.svo_process_batch_masked(vo._h, lp, rp, stride, 0, _lib.ptr(act), _lib.ptr(T), _lib.ptr(ok), st))
    vo.stats = list(st)


def device_frames(frames, extra):
    """torch device copies of the frames with rows `extra` bytes wider than the image, 0xAB in the gap -> (tensors, stride)."""
    import torch
    out, stride = [], None
    for a in frames:
        rows = a.reshape(a.shape[0], -1)
        t = torch.full((rows.shape[0], rows.shape[1] + extra), 0xAB, dtype=torch.uint8, device="cuda")
        t[:, :rows.shape[1]] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        out.append(t); stride = t.shape[1]
    torch.cuda.synchronize()
    return out, stride


def assert_route(api, vo, route, what):
    from stereo_visual_odometry_amd import _lib
    p = vo.last_frame_path()
    fused, ahead = bool(p & _lib.PATH_FRONT_FUSED), bool(p & _lib.PATH_INGEST_AHEAD)
    want = {"fused": (True, False), "ahead": (False, True)}.get(route, (False, False))
    assert (fused, ahead) == want, (what, route, p)


class LastLeft:
    """lastLeftPyramid's frame per sequence, from the frames' stats: it moves to a frame that is the sequence's first one (since
    creation or reset) or that had points to match (n_into_lk > 0); vo.cpp:50-53, 179-181, 231-232."""

    def __init__(self, B):
        self.frame = [None] * B
        self.first = [True] * B

    def update(self, seq, frame, stats):
        if self.first[seq] or stats.n_into_lk > 0:
            self.frame[seq] = frame
        self.first[seq] = False

    def reset(self, seq):
        self.first[seq] = True


def run_case(api, case):
    """Two or three frames of a case; every frame's T1 and lastLeftPyramid pyramids checked whenever no frame is in flight."""
    route, (w, h), win, ml, B, inp, ex = case
    what = case_id(case)
    cn = 3 if route == "bgr" else 1
    ctx = Ctx(api, w, h, win, ml, B, cn=cn, rect=bool(ex.get("rect")), fpb=ex.get("fpb", 1))
    vo = ctx.vo
    depth = ex.get("depth", 1)
    n = 2 + depth
    iw, ih = ctx.in_size()
    # sequence 0 gets a black second frame: a frame with nothing to track may leave lastLeftPyramid behind T1
    streams = [make_stream(iw, ih, n, 1000 * win + 17 * i + w, cn, black=(1,) if i == 0 else ()) for i in range(B)]
    ll = LastLeft(B)
    if inp.startswith("dev"):
        extra = int(inp[4:])
        dev = [[device_frames([s[0][k], s[1][k]], extra) for k in range(n)] for s in streams]
        stride = dev[0][0][1]
        sub = 0
        for k in range(n):
            while sub < n and sub - k < depth:
                vo.submit_device([dev[i][sub][0][0].data_ptr() for i in range(B)], [dev[i][sub][0][1].data_ptr() for i in range(B)], stride)
                assert_route(api, vo, route, (what, sub))
                sub += 1
            vo.collect()
            for i in range(B):
                ll.update(i, k, vo.stats[i])
            if sub == k + 1:
                for i in range(B):
                    ctx.check(i, "t1", (streams[i][0][k], streams[i][1][k]), (what, k))
                    j = ll.frame[i]
                    ctx.check(i, "last_left", (streams[i][0][j], streams[i][1][j]), (what, k, "last_left", j))
        del dev
    else:
        for k in range(n):
            Ls, Rs = [s[0][k] for s in streams], [s[1][k] for s in streams]
            if inp == "stride":
                host_strided(api, vo, Ls, Rs, 13)
            else:
                if inp == "pinned":
                    pin = [api.PinnedImage(a.shape) for a in Ls + Rs]
                    for p, a in zip(pin, Ls + Rs):
                        p.array[...] = a
                    Ls, Rs = [p.array for p in pin[:B]], [p.array for p in pin[B:]]
                vo.stereo_callback_batch(Ls, Rs)
            assert_route(api, vo, route, (what, k))
            for i in range(B):
                ll.update(i, k, vo.stats[i])
                ctx.check(i, "t1", (streams[i][0][k], streams[i][1][k]), (what, k))
                j = ll.frame[i]
                ctx.check(i, "last_left", (streams[i][0][j], streams[i][1][j]), (what, k, "last_left", j))
    ctx.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_frame_pyramids_byte_exact(api, case):
    run_case(api, case)


def test_many_sequences_without_build_ahead():
    """The many-sequence k_ingest_pyr1 on the frame's own stream (SVO_INGEST_AHEAD=0, read once per process): a fresh child."""
    env = dict(os.environ, SVO_INGEST_AHEAD="0")
    r = run_child("pyramid_child.py", json.dumps(MANY_CASES), env=env, timeout=600)
    assert "pyramid child ok: %d cases" % len(MANY_CASES) in r.stdout


# ------------------------------------------------------------------------------------------------------------ member call
@pytest.mark.parametrize("shape,win,ml,cn,rect", [((90, 46), 5, 3, 1, False), ((417, 203), 10, 3, 3, False), ((322, 161), 10, 3, 1, True)])
def test_member_circular_matching_caches_its_t1_pair(api, shape, win, ml, cn, rect):
    """VisualOdometry.circularMatching after a stereo_callback builds its own T1 pyramids (svo_circular_matching's ingest) and
    makes them lastLeftPyramid / lastRightPyramid (vo.cpp:231-232); imageLeftT0_ / imageRightT0_ (the T1 read-out) stay the last
    stereo_callback's.  The next stereo_callback then replaces T1 and, having points, lastLeftPyramid."""
    w, h = shape
    ctx = Ctx(api, w, h, win, ml, 1, cn=cn, rect=rect, facade=True)
    vo = ctx.vo
    iw, ih = ctx.in_size()
    L, R = make_stream(iw, ih, 3, 77 + w, cn)
    vo.stereo_callback(L[0], R[0])
    ctx.check(0, "t1", (L[0], R[0]), "callback 0")
    ctx.check(0, "last_left", (L[0], R[0]), "callback 0")
    fs = api.FeatureSet()
    pts = np.stack(np.meshgrid(np.linspace(-4, w + 4, 9), np.linspace(-4, h + 4, 7)), -1).reshape(-1, 2).astype(np.float32)
    fs.points, fs.ages, fs.strengths = pts.copy(), np.zeros(len(pts), np.int32), np.ones(len(pts), np.int32)
    vo.circularMatching(L[1], R[1], pts, fs)
    ctx.check(0, "t1", (L[0], R[0]), "after the member call")
    ctx.check(0, "last_left", (L[1], R[1]), "after the member call")
    vo.stereo_callback(L[2], R[2])
    assert vo.stats.n_into_lk > 0
    ctx.check(0, "t1", (L[2], R[2]), "callback 2")
    ctx.check(0, "last_left", (L[2], R[2]), "callback 2")
    ctx.close()


# -------------------------------------------------------------------------------------------------------------- lifecycle
def snapshot(ctx, seq):
    return {which: ctx.read(seq, which) for which in ("t1", "last_left")}


def same_snapshot(a, b):
    return all(a[w].keys() == b[w].keys() and all(np.array_equal(a[w][k][0], b[w][k][0]) for k in a[w]) for w in a)


@pytest.mark.parametrize("B,route", [(3, "fused"), (10, "ahead")])
def test_idle_sequences_keep_their_pyramids_and_reset_refuses(api, B, route):
    """Ragged frames: an idle sequence's T1 and lastLeftPyramid stay byte-identical across the frames it sits out; after
    svo_reset_sequence the read-out refuses (SVO_ERR_STATE) until the sequence's next active frame, whose images T1 then holds;
    black frames spliced in leave lastLeftPyramid on the last frame that was a first frame or had points to match."""
    from stereo_visual_odometry_amd import _lib
    w, h, win, ml = 130, 66, 7, 3
    ctx = Ctx(api, w, h, win, ml, B)
    vo = ctx.vo
    n_steps = 9
    rng = np.random.default_rng(B)
    act = rng.random((n_steps, B)) < 0.6
    act[0] = True                                                # every sequence starts
    act[:, 0] = [1, 1, 0, 1, 1, 0, 1, 1, 1]                      # sequence 0: reset after step 4, idle at step 5, a new stream from step 6
    act[:, 1] = True                                             # sequence 1: black frames at its stream frames 2, 5, 6
    reset_seq, reset_after = 0, 4
    streams = [make_stream(w, h, n_steps, 500 + 31 * i, black=(2, 5, 6) if i == 1 else ()) for i in range(B)]
    new_stream = make_stream(w, h, n_steps, 4242)
    nxt = [0] * B
    shown = [None] * B                                           # stream frame index in T1 (None: nothing readable)
    ll = LastLeft(B)
    out = np.zeros(1 << 16, np.uint8)

    def refuses(seq):
        return all(_lib.lib.svo_get_pyramid(vo._h, seq, which, 0, 0, 0, _lib.ptr(out), out.size, None, None, None, None)
                   == _lib.SVO_ERR_STATE for which in (_lib.PYR_T1, _lib.PYR_LAST_LEFT))

    saw_lag = refused_idle = False
    for k in range(n_steps):
        a = act[k]
        before = {i: snapshot(ctx, i) for i in range(B) if not a[i] and shown[i] is not None}
        Ls = [streams[i][0][nxt[i]] if a[i] else None for i in range(B)]
        Rs = [streams[i][1][nxt[i]] if a[i] else None for i in range(B)]
        vo.stereo_callback_batch(Ls, Rs, active=a)
        assert_route(api, vo, route, ("step", k))
        for i in range(B):
            if a[i]:
                ll.update(i, nxt[i], vo.stats[i])
                shown[i] = nxt[i]; nxt[i] += 1
                ctx.check(i, "t1", (streams[i][0][shown[i]], streams[i][1][shown[i]]), ("step", k))
                j = ll.frame[i]
                ctx.check(i, "last_left", (streams[i][0][j], streams[i][1][j]), ("step", k, "last_left", j))
                saw_lag |= j != shown[i]
            elif shown[i] is not None:
                assert same_snapshot(before[i], snapshot(ctx, i)), ("idle sequence changed", k, i)
            else:
                assert refuses(i), ("a reset sequence's read-out must refuse until its next active frame", k, i)
                refused_idle = True
        if k == reset_after:
            vo.reset_sequence(reset_seq)
            ll.reset(reset_seq); shown[reset_seq] = None
            streams[reset_seq] = new_stream; nxt[reset_seq] = 0
            assert refuses(reset_seq)
    assert refused_idle and shown[reset_seq] is not None
    assert saw_lag, "no black frame left lastLeftPyramid behind: the rule went untested"
    ctx.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_build_ahead_in_flight_then_drain(api, depth):
    """Build-ahead with 2-3 frames in flight and black frames spliced in: after the drain, T1 is the last frame and
    lastLeftPyramid the frame the stats name — an ahead build that landed in a slot still in use would show here."""
    B, w, h, win, ml = 9, 255, 129, 10, 3
    ctx = Ctx(api, w, h, win, ml, B)
    vo = ctx.vo
    n = 7
    streams = [make_stream(w, h, n, 40 + 7 * i, black=((2,), (1, 2), (4,), (5,), ())[i % 5]) for i in range(B)]
    dev = [[device_frames([s[0][k], s[1][k]], 3) for k in range(n)] for s in streams]
    stride = dev[0][0][1]
    ll = LastLeft(B)
    lag = False
    sub = 0
    for burst_end in (4, n):                                     # drain twice: mid-run and at the end
        start = sub
        for k in range(start, burst_end):
            while sub < burst_end and sub - k < depth:
                vo.submit_device([dev[i][sub][0][0].data_ptr() for i in range(B)], [dev[i][sub][0][1].data_ptr() for i in range(B)], stride)
                assert_route(api, vo, "ahead", sub)
                sub += 1
            vo.collect()
            for i in range(B):
                ll.update(i, k, vo.stats[i])
        last = burst_end - 1
        for i in range(B):
            ctx.check(i, "t1", (streams[i][0][last], streams[i][1][last]), ("drained at", last))
            j = ll.frame[i]
            lag |= j != last
            ctx.check(i, "last_left", (streams[i][0][j], streams[i][1][j]), ("drained at", last, "last_left", j))
    assert lag, "every lastLeftPyramid was T1: the in-flight slots went untested"
    del dev
    ctx.close()


def test_read_out_refusals(api):
    """Bad indices: SVO_ERR_ARG; before the first frame, with frames in flight: SVO_ERR_STATE; out == NULL: sizes only."""
    from stereo_visual_odometry_amd import _lib
    lib = _lib.lib
    ctx = Ctx(api, 90, 46, 5, 3, 2)
    vo = ctx.vo
    out = np.zeros(1 << 16, np.uint8)
    w, h, pad, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.svo_get_pyramid(vo._h, 0, 0, 0, 0, 3, None, 0, C.byref(w), C.byref(h), C.byref(pad), C.byref(nl)) == 0
    assert (w.value, h.value, pad.value, nl.value) == (12, 6, 12, 4)
    assert lib.svo_get_pyramid(vo._h, 0, 0, 0, 0, 0, _lib.ptr(out), out.size, None, None, None, None) == _lib.SVO_ERR_STATE
    for args in ((2, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 4), (0, 0, 0, 0, -1)):
        assert lib.svo_get_pyramid(vo._h, *args, _lib.ptr(out), out.size, None, None, None, None) == _lib.SVO_ERR_ARG, args
    L, R = make_stream(90, 46, 2, 3)
    vo.stereo_callback_batch([L[0]] * 2, [R[0]] * 2)
    assert lib.svo_get_pyramid(vo._h, 0, 0, 0, 0, 0, _lib.ptr(out), (90 + 24) * (46 + 24) - 1, None, None, None, None) == _lib.SVO_ERR_ARG
    dev, stride = device_frames([L[1], R[1]], 0)
    vo.submit_device([dev[0].data_ptr()] * 2, [dev[1].data_ptr()] * 2, stride)
    assert lib.svo_get_pyramid(vo._h, 1, 0, 1, 0, 0, _lib.ptr(out), out.size, None, None, None, None) == _lib.SVO_ERR_STATE
    vo.collect()
    ctx.check(1, "t1", (L[1], R[1]), "after collect")
    del dev
    ctx.close()
