"""The derivative planes the LK kernel loads at the pyramid levels >= 1, sample for sample, border included (svo_get_derivatives).

Many-sequence grey contexts in the exact-sums mode keep, beside every pyramid, the Scharr images of its levels >= 1 (k_deriv_levels,
svo_internal.hpp).  Every case runs such a context over a short stream and, after every frame at which nothing is in flight, reads
back both planes of every sequence, camera, level >= 1 and of both T1 and lastLeftPyramid's pair WITH the stored border, and compares
every sample with tests/deriv_ref.py applied to the reference pyramid (tests/pyramid_ref.py) of the frame's own images: 4 x the
Scharr value of the level on its REFLECT_101 border inside the level, zero outside it.  Integers: no tolerance anywhere.  Every frame
must report SVO_PATH_INGEST_AHEAD.  The matrix (deriv_ref.CASES; guarded on the CPU by tests/test_deriv_ref.py) spreads over its rows:
host, pinned and device frames with 1-3 frames in flight (every slot gets rewritten: a stale sample or a store into the border
shows); a black second frame of sequence 0 (lastLeftPyramid lags T1); a masked frame a third of the sequences sit out (their planes
stay byte-identical); a reset sequence (refused until its next frame); a rectifying, a bgr8 and a CLAHE context (other ingest kernels
in front of the same planes); the bench shape."""
import ctypes as C
import os

import numpy as np
import pytest

import deriv_ref
import pyramid_ref as ref
import test_gpu_pyramids as tp
from test_gpu_pyramids import LastLeft, assert_route, device_frames, make_stream
from gpu_kit import api, run_child  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

CLAHE = (2.0, (8, 8))


class Planes(tp.Ctx):
    """A context of one case: tp.Ctx's reference pyramids, and the planes checked against deriv_ref of their levels."""

    def __init__(self, api, case):
        (w, h), win, ml, B, inp, ex, chain = case
        super().__init__(api, w, h, win, ml, B, rect=bool(ex.get("rect")))
        self.chain = chain
        self._planes = {}
        if ex.get("fmt"):
            self.vo.set_input_format(ex["fmt"])
        if ex.get("clahe"):
            self.vo.set_clahe(*CLAHE)

    def want(self, img, cam, lv):
        """(ix, iy, the reference level) of level lv of the grey frame `img` as the library stores them"""
        key = (id(img), cam, lv)
        if key not in self._planes:
            level = self.reference(img, cam)[0][lv]
            self._planes[key] = deriv_ref.planes(level, tp.lk_pad_for(self.win)) + (level,)
        return self._planes[key]

    def read(self, seq, which):
        """{(cam, level): (ix, iy)} of one stored pair of pyramids"""
        return {(cam, lv): self.vo.derivatives(seq, which, cam, lv)[:2] for cam in range(2) for lv in range(1, self.vo.pyramid_levels())}

    def check(self, seq, which, pair, what):
        """Every sample of the planes `which` of `seq` against the reference planes of the grey stereo pair `pair`."""
        n = self.vo.pyramid_levels()
        assert n == 1 + len(self.chain), (what, "levels", n)
        for cam, img in enumerate(pair):
            for lv in range(1, n):
                wx, wy, level = self.want(img, cam, lv)
                gx, gy, pad = self.vo.derivatives(seq, which, cam, lv)
                assert pad == tp.lk_pad_for(self.win) and level.shape[::-1] == self.chain[lv - 1]
                for name, got, exp in (("Ix", gx, wx), ("Iy", gy, wy)):
                    assert got.dtype == np.int16 and got.shape == exp.shape, (what, name, got.shape, exp.shape)
                    if not np.array_equal(got, exp):
                        self.report(seq, which, cam, lv, name, got, exp, level, pad, what)

    def report(self, seq, which, cam, lv, name, got, exp, level, pad, what):
        ys, xs = np.nonzero(got != exp)
        lh, lw = level.shape
        inner = int(((ys >= pad) & (ys < pad + lh) & (xs >= pad) & (xs < pad + lw)).sum())
        stored, _ = self.vo.pyramid(seq, which, cam, lv)
        pyr_ok = np.array_equal(stored, ref.padded(level, pad))
        pytest.fail("%s: seq %d %s cam %d level %d (%dx%d, pad %d) %s: %d samples differ, %d inside the level and %d in the border; first at "
                    "(x, y) = %s; the stored pyramid level %s its reference (%s)"
                    % (what, seq, which, cam, lv, lw, lh, pad, name, len(ys), inner, len(ys) - inner,
                       list(zip((xs[:6] - pad).tolist(), (ys[:6] - pad).tolist())),
                       "equals" if pyr_ok else "DIFFERS from", "a derivative fault" if pyr_ok else "a pyramid fault"))


def refuses(vo, seq):
    from stereo_visual_odometry_amd import _lib
    buf = np.zeros((vo.height + 80) * (vo.width + 80), np.int16)
    return all(_lib.lib.svo_get_derivatives(vo._h, seq, which, cam, 1, _lib.ptr(buf), None, buf.size, None, None, None, None) == _lib.SVO_ERR_STATE
               for which in (_lib.PYR_T1, _lib.PYR_LAST_LEFT) for cam in (0, 1))


def fed_streams(case, n):
    """Per sequence ([fed left], [fed right], [grey left], [grey right]): what the library is given and the grey frames its pyramids are
    of (before rectification, which tp.Ctx.reference applies).  One spare stream at the end for the sequence that is reset."""
    (w, h), win, ml, B, inp, ex, chain = case
    size = (tp.RAW_W, tp.RAW_H) if ex.get("rect") else (w, h)
    out = []
    rng = np.random.default_rng(w)
    for i in range(B + 1):
        # sequence 0 gets a black second frame: a frame with nothing to track leaves lastLeftPyramid behind T1 one frame later
        L, R = make_stream(size[0], size[1], n, 1000 * win + 17 * i + w, black=(1,) if i == 0 else ())
        fedL, fedR = L, R
        if ex.get("fmt"):
            import input_format_ref
            cl, cr = [input_format_ref.colour_of(a, ex["fmt"], rng) for a in L], [input_format_ref.colour_of(a, ex["fmt"], rng) for a in R]
            fedL, fedR, L, R = [c[0] for c in cl], [c[0] for c in cr], [c[1] for c in cl], [c[1] for c in cr]
        if ex.get("clahe"):
            import clahe_ref
            L, R = [clahe_ref.clahe_ref(a, *CLAHE) for a in L], [clahe_ref.clahe_ref(a, *CLAHE) for a in R]
        out.append((fedL, fedR, L, R))
    return out


def run_case(api, case):
    (w, h), win, ml, B, inp, ex, chain = case
    what = deriv_ref.case_id(case)
    n = ex["frames"]
    ctx = Planes(api, case)
    vo = ctx.vo
    assert vo.has_derivatives(), what
    streams = fed_streams(case, n)
    spare = streams.pop()
    mask_at, reset_before = ex.get("mask"), ex.get("mask") if "reset" in ex else None
    reset_seq = ex.get("reset")
    assert reset_seq is None or reset_seq % 3 == 1                # it sits the masked frame out
    nxt, shown = [0] * B, [None] * B                              # per sequence: its next stream frame, the one T1 holds (None: refused)
    ll = LastLeft(B)
    depth = ex.get("depth", 1) if inp.startswith("dev") else 1
    dev = {}
    lag = refused = idle_kept = False

    def active(k):
        return [not (k == mask_at and i % 3 == 1) for i in range(B)]

    def verify(k, before):
        nonlocal lag, refused, idle_kept
        for i in range(B):
            if shown[i] is None:
                assert refuses(vo, i), (what, k, i, "a reset sequence's read-out must refuse until its next active frame")
                refused = True
                continue
            j = ll.frame[i]
            s = streams[i]
            ctx.check(i, "t1", (s[2][shown[i]], s[3][shown[i]]), (what, k))
            ctx.check(i, "last_left", (s[2][j], s[3][j]), (what, k, "last_left", j))
            lag |= j != shown[i]
            if i in before:
                now = {wh: ctx.read(i, wh) for wh in ("t1", "last_left")}
                assert all(a.tobytes() == b.tobytes() for wh in now for key in now[wh] for a, b in zip(before[i][wh][key], now[wh][key])), \
                    (what, k, i, "the planes of a sequence that sat the frame out changed")
                idle_kept = True

    k = 0
    while k < n:
        burst = range(k, min(k + depth, n))
        if mask_at in burst:                                      # the masked frame runs alone: nothing in flight before or after it
            burst = range(k, k + 1) if k == mask_at else range(k, mask_at)
        before, acts, stats, fed = {}, {}, {}, {}
        for f in burst:
            if f == reset_before:
                assert f == k, "a reset needs nothing in flight here"
                vo.reset_sequence(reset_seq)
                ll.reset(reset_seq); shown[reset_seq] = None
                streams[reset_seq] = spare; nxt[reset_seq] = 0
                assert refuses(vo, reset_seq), (what, "just after the reset")
            acts[f] = act = active(f)
            if f == mask_at:                                      # what the idle sequences hold now must survive the frame
                before = {i: {wh: ctx.read(i, wh) for wh in ("t1", "last_left")} for i in range(B) if not act[i] and shown[i] is not None}
            masked = None if all(act) else act
            Ls = [streams[i][0][nxt[i]] if act[i] else None for i in range(B)]
            Rs = [streams[i][1][nxt[i]] if act[i] else None for i in range(B)]
            fed[f] = list(nxt)                                    # the stream frame each active sequence is given
            for i in range(B):
                nxt[i] += act[i]
            if inp.startswith("dev"):
                on = [a for a in Ls + Rs if a is not None]
                t, stride = device_frames(on, int(inp[4:]))
                dev[f] = t
                it = iter(t)
                ptrs = [next(it).data_ptr() if a is not None else None for a in Ls + Rs]
                vo.submit_device(ptrs[:B], ptrs[B:], stride, active=masked)
            else:
                if inp == "pinned":
                    pin = [api.PinnedImage(a.shape) if a is not None else None for a in Ls + Rs]
                    for p, a in zip(pin, Ls + Rs):
                        if a is not None:
                            p.array[...] = a
                    Ls, Rs = [p.array if p is not None else None for p in pin[:B]], [p.array if p is not None else None for p in pin[B:]]
                vo.stereo_callback_batch(Ls, Rs, active=masked)
            assert_route(api, vo, "ahead", (what, f))
            if not inp.startswith("dev"):
                stats[f] = vo.stats
        for f in burst:
            if inp.startswith("dev"):
                vo.collect()
                stats[f] = vo.stats
            for i in range(B):
                if acts[f][i]:
                    ll.update(i, fed[f][i], stats[f][i])
                    shown[i] = fed[f][i]
        k = burst[-1] + 1
        verify(k - 1, before)                                     # nothing is in flight
    dev.clear()
    assert lag or n < 3, (what, "no black frame left lastLeftPyramid behind T1: the rule went untested")
    assert refused or reset_seq is None, what
    assert idle_kept or mask_at is None, what
    ctx.close()


@pytest.mark.parametrize("case", deriv_ref.CASES, ids=deriv_ref.case_id)
def test_derivative_planes_sample_exact(api, case):
    run_case(api, case)


# --------------------------------------------------------------------------------------------------------------- refusals
def test_read_out_refusals(api):
    """Bad indices: SVO_ERR_ARG (level 0 has no planes); before the first frame and with frames in flight: SVO_ERR_STATE; both arrays
    NULL: sizes only; either array alone is filled."""
    from stereo_visual_odometry_amd import _lib
    lib = _lib.lib
    case = ((134, 70), 5, 3, 9, "host", {"frames": 2}, [(67, 35), (34, 18), (17, 9)])
    ctx = Planes(api, case)
    vo = ctx.vo
    buf = np.zeros(1 << 16, np.int16)
    w, h, pad, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.svo_get_derivatives(vo._h, 0, 0, 0, 3, None, None, 0, C.byref(w), C.byref(h), C.byref(pad), C.byref(nl)) == 0
    assert (w.value, h.value, pad.value, nl.value) == (17, 9, 12, 4)
    assert vo.has_derivatives()
    assert lib.svo_get_derivatives(vo._h, 0, 0, 0, 1, _lib.ptr(buf), _lib.ptr(buf), buf.size, None, None, None, None) == _lib.SVO_ERR_STATE   # no frame yet
    #            seq which cam level
    for args in ((0, 0, 0, 0), (0, 0, 0, 4), (0, 0, 0, -1), (0, 0, 2, 1), (0, 0, -1, 1), (0, 2, 0, 1), (0, -1, 0, 1), (9, 0, 0, 1), (-1, 0, 0, 1)):
        assert lib.svo_get_derivatives(vo._h, *args, _lib.ptr(buf), _lib.ptr(buf), buf.size, None, None, None, None) == _lib.SVO_ERR_ARG, args
        assert lib.svo_get_derivatives(vo._h, *args, None, None, 0, None, None, None, None) == _lib.SVO_ERR_ARG, args
    L, R = make_stream(134, 70, 2, 3)
    vo.stereo_callback_batch([L[0]] * 9, [R[0]] * 9)
    need = (67 + 24) * (35 + 24)
    assert lib.svo_get_derivatives(vo._h, 0, 0, 0, 1, _lib.ptr(buf), _lib.ptr(buf), need - 1, None, None, None, None) == _lib.SVO_ERR_ARG
    assert lib.svo_get_derivatives(vo._h, 0, 0, 0, 1, _lib.ptr(buf), None, need, None, None, None, None) == _lib.SVO_OK
    wx, wy, _ = ctx.want(L[0], 0, 1)
    assert np.array_equal(buf[:need].reshape(wx.shape), wx) and not buf[need:].any()
    assert lib.svo_get_derivatives(vo._h, 0, 0, 0, 1, None, _lib.ptr(buf), need, None, None, None, None) == _lib.SVO_OK
    assert np.array_equal(buf[:need].reshape(wy.shape), wy) and not buf[need:].any()
    dev, stride = device_frames([L[1], R[1]], 0)
    vo.submit_device([dev[0].data_ptr()] * 9, [dev[1].data_ptr()] * 9, stride)
    assert lib.svo_get_derivatives(vo._h, 1, 0, 1, 1, _lib.ptr(buf), _lib.ptr(buf), buf.size, None, None, None, None) == _lib.SVO_ERR_STATE
    assert "in flight" in lib.svo_last_error().decode()
    vo.collect()
    ctx.check(1, "t1", (L[1], R[1]), "after collect")
    del dev
    ctx.close()


@pytest.mark.parametrize("n_seq,over", [(8, {}), (9, {"channels": 3}), (9, {"lk_float_sums": 1}), (9, {"max_level": 0})],
                         ids=["8-sequences", "channels-3", "float-sums", "one-level"])
def test_contexts_without_planes_say_so(api, n_seq, over):
    """A context that keeps no planes answers SVO_ERR_STATE with "no planes", with or without arrays, before and after a frame."""
    from stereo_visual_odometry_amd import _lib
    w, h = 134, 70
    cfg = api.default_config(**dict(dict(win_w=5, win_h=5, max_level=3, max_translation_norm=2.0), **over))
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg)
    vo.initalize_projection_matricies(*tp.projections(w, h))
    buf = np.zeros(1 << 16, np.int16)
    cn = over.get("channels", 1)
    L, R = make_stream(w, h, 1, 5, cn)

    def asked():
        assert not vo.has_derivatives()
        for level in (0, 1):
            for a in (None, _lib.ptr(buf)):
                assert _lib.lib.svo_get_derivatives(vo._h, 0, 0, 0, level, a, a, buf.size, None, None, None, None) == _lib.SVO_ERR_STATE
                assert "no planes" in _lib.lib.svo_last_error().decode()
        with pytest.raises(_lib.SvoError, match="no planes"):
            vo.derivatives(0, "t1", 0, 1)

    asked()
    vo.stereo_callback_batch([L[0]] * n_seq, [R[0]] * n_seq)
    asked()
    vo.close()


@pytest.mark.parametrize("var", ["SVO_LK_DERIV", "SVO_INGEST_AHEAD"])
def test_switched_off_in_the_environment(var):
    """SVO_LK_DERIV=0 (no planes) and SVO_INGEST_AHEAD=0 (no build-ahead, hence none) are read once per process: a fresh child each."""
    r = run_child("deriv_planes_child.py", var, env=dict(os.environ, **{var: "0"}))
    assert "deriv planes child ok: no planes under %s=0" % var in r.stdout
