"""The many-sequence front at batch speed (k_fast_batch, k_deriv_levels, k_pad_pyramid) against the references, at the sizes the
kernels' tiles make special (tests/front_batch_cases.py; tests/test_front_batch_cases.py guards the matrix on the CPU).

Every case is a plain grey context of 9 .. 12 sequences — the smallest that take the many-sequence path: every frame must report
SVO_PATH_INGEST_AHEAD — fed three host frames.  After every frame, for every sequence:
- the T1 pyramids and lastLeftPyramid's pair, borders included, equal tests/pyramid_ref.py byte for byte;
- the derivative planes of both, borders included, equal tests/deriv_ref.py sample for sample;
- the flags, every svo_frame_stats field and the feature set equal the CPU oracle's exactly, the pose within 1e-6
  (tests/test_gpu_parity.py's tolerance).
The streams put corners on the three-pixel image margin and on both sides of the FAST tile seams (dots), more candidates into one
tile than its block has threads (dense), and a frame that needs the second detection pass (black)."""
import numpy as np
import pytest

import deriv_ref
import front_batch_cases as fb
import oracle_lib as orc
import pyramid_ref as ref
from gpu_kit import api, f32_bits as bits  # noqa: F401  (the fixture is found by name)
from test_gpu_parity import POSE_TOL_R, POSE_TOL_T, rot_angle
from test_gpu_pyramids import LastLeft, assert_route

pytestmark = pytest.mark.gpu


def oracle_run(case, L, R):
    """Per frame (ok, T, stats, features) of the CPU oracle on one stream."""
    from stereo_visual_odometry_amd import synthetic as syn
    (w, h), win, ml, B, kinds = case
    Pl, Pr = syn.projection_matrices(fb.calib(w, h))
    o = orc.VisualOdometry(orc.default_config(win_w=win, win_h=win, max_level=ml, max_translation_norm=2.0))
    o.initalize_projection_matricies(Pl, Pr)
    out = []
    for k in range(len(L)):
        ok, T = o.stereo_callback(L[k], R[k])
        out.append((ok, T.copy(), {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, [a.copy() for a in o.features()]))
    return out


class Stored:
    """The reference pyramids and planes of a stream's frames, computed once per (stream, frame, camera)."""

    def __init__(self, vo, win, ml):
        self.vo, self.win, self.ml, self.pad = vo, win, ml, fb.lk_pad_for(win)
        self._ref = {}

    def want(self, key, img):
        if key not in self._ref:
            levels = ref.pyramid(img, self.win, self.ml)
            self._ref[key] = ([ref.padded(lv, self.pad) for lv in levels], [deriv_ref.planes(lv, self.pad) for lv in levels[1:]])
        return self._ref[key]

    def check(self, seq, which, keys, pair, what):
        n = self.vo.pyramid_levels()
        for cam, img in enumerate(pair):
            pyr, planes = self.want(keys + (cam,), img)
            assert len(pyr) == n, (what, "levels", n, len(pyr))
            for lv in range(n):
                got, pad = self.vo.pyramid(seq, which, cam, lv)
                assert pad == self.pad and got.shape == pyr[lv].shape, (what, which, cam, lv, pad, got.shape)
                bad = np.argwhere(got != pyr[lv])
                assert not len(bad), "%s: seq %d %s cam %d level %d: %d bytes differ, first (y, x) %s (border %d)" % (what, seq, which, cam, lv, len(bad), bad[:4].tolist(), pad)
            for lv in range(1, n):
                gx, gy, pad = self.vo.derivatives(seq, which, cam, lv)
                for name, got, exp in (("Ix", gx, planes[lv - 1][0]), ("Iy", gy, planes[lv - 1][1])):
                    assert got.dtype == np.int16 and got.shape == exp.shape, (what, name, got.shape, exp.shape)
                    bad = np.argwhere(got != exp)
                    assert not len(bad), "%s: seq %d %s cam %d level %d %s: %d samples differ, first (y, x) %s (border %d)" % (what, seq, which, cam, lv, name, len(bad), bad[:4].tolist(), pad)


@pytest.mark.parametrize("case", fb.CASES, ids=fb.case_id)
def test_batch_front_matches_the_references(api, case):
    from stereo_visual_odometry_amd import synthetic as syn
    (w, h), win, ml, B, kinds = case
    what = fb.case_id(case)
    assert 9 <= B <= 12
    streams = [fb.stream(kind, w, h, 1000 * win + 31 * j + w) for j, kind in enumerate(kinds)]
    want = [oracle_run(case, L, R) for L, R in streams]
    if "black" in kinds:
        assert any(fr[2]["second_pass"] == 1 for fr in want[kinds.index("black")]), (what, "no frame needed the second detection pass")
    if "dots" in kinds or "dense" in kinds:
        assert any(fr[2]["n_after_detect"] > 0 for j, k in enumerate(kinds) if k in ("dots", "dense") for fr in want[j]), (what, "no features detected")
    vo = api.BatchVisualOdometry(w, h, B, api.default_config(win_w=win, win_h=win, max_level=ml, max_translation_norm=2.0))
    vo.initalize_projection_matricies(*syn.projection_matrices(fb.calib(w, h)))
    assert vo.has_derivatives(), what
    stored = Stored(vo, win, ml)
    ll = LastLeft(B)
    for k in range(fb.N_FRAMES):
        ok, T = vo.stereo_callback_batch([streams[i % len(kinds)][0][k] for i in range(B)], [streams[i % len(kinds)][1][k] for i in range(B)])
        assert_route(api, vo, "ahead", (what, k))
        for i in range(B):
            j = i % len(kinds)
            o_ok, o_T, o_stats, o_feat = want[j][k]
            sg = vo.stats[i].as_dict()
            assert bool(ok[i]) == o_ok and sg == o_stats, (what, k, i, sg, o_stats)
            f = vo.features(i)
            assert np.array_equal(bits(f[0]), bits(o_feat[0])) and np.array_equal(f[1], o_feat[1]) and np.array_equal(f[2], o_feat[2]), (what, k, i, "feature set")
            assert np.abs(T[i][:3, 3] - o_T[:3, 3]).max() < POSE_TOL_T and rot_angle(T[i][:3, :3], o_T[:3, :3]) < POSE_TOL_R, (what, k, i, "pose")
            ll.update(i, k, vo.stats[i])
            L, R = streams[j]
            stored.check(i, "t1", (j, k), (L[k], R[k]), (what, k))
            m = ll.frame[i]
            stored.check(i, "last_left", (j, m), (L[m], R[m]), (what, k, "last_left", m))
    vo.close()
