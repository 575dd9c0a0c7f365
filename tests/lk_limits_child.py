"""Frame-pipeline runs of tests/test_gpu_lk_limits.py over maximum-contrast frames: the synthetic stereo stream of the smallest
four-level frame (tests/lk_deriv_child.py, scene four_levels: 200 x 169, w = 21, max_level = 3), every frame binarised at its median to
0 / 255.  Imported by the tests for the frames, the oracle's results and the default runs; run as a script in a fresh process with
SVO_LK_DERIV=0 (the switch is read once per process) it repeats the many-sequence run without the derivative planes and writes what
the frames returned to the .npz named on the command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lk_deriv_child as ldc                # noqa: E402
import lk_limits_scenes as lim              # noqa: E402
import oracle_lib as orc                    # noqa: E402

NAME, B, N_FRAMES = "four_levels", ldc.B, 3
STAT_NAMES = sorted(f[0] for f in orc.OrcFrameStats._fields_)


def frames():
    """[stream][frame] (left, right), binarised"""
    return [[(lim.binarised(s.left[k]), lim.binarised(s.right[k])) for k in range(N_FRAMES)] for s in ldc.streams(NAME, n_frames=N_FRAMES)]


def config_over(float_sums=0):
    return dict(ldc.config_over(NAME), lk_float_sums=float_sums)


def oracle_frames(float_sums=0):
    """[stream][frame] dict(ok, T, stats, xy, age, strength, tracks) of a fresh oracle per stream"""
    out = []
    for s in frames():
        o = orc.VisualOdometry(orc.default_config(**config_over(float_sums))); o.initalize_projection_matricies(*ldc.projections(NAME))
        per = []
        for L, R in s:
            ok, T = o.stereo_callback(L, R)
            f = o.features()
            per.append(dict(ok=ok, T=T.reshape(16).copy(), stats=np.array([getattr(o.stats, n) for n in STAT_NAMES], np.int64),
                            xy=f[0].view(np.uint32).copy(), age=f[1].copy(), strength=f[2].copy(),
                            tracks={k: v.copy() for k, v in o.last_tracks().items()} if o.stats.n_into_lk else None))
        out.append(per)
    return out


def run_batch(api):
    """A B-sequence context (sequence i plays stream i % 2) -> flat {"k/i/field": array} and "paths" """
    w, h = ldc.SCENES[NAME][:2]
    fr = frames()
    vo = api.BatchVisualOdometry(w, h, B, api.default_config(**config_over())); vo.initalize_projection_matricies(*ldc.projections(NAME))
    out, paths = {}, []
    for k in range(N_FRAMES):
        ok, T = vo.stereo_callback_batch([fr[i % 2][k][0] for i in range(B)], [fr[i % 2][k][1] for i in range(B)])
        for i in range(B):
            ldc.flatten("%d/%d" % (k, i), ldc.record(vo, ok, T, i), out)
        paths.append(vo.last_frame_path())
    vo.close()
    out["paths"] = np.array(paths, np.int64)
    return out


def main():
    assert os.environ.get("SVO_LK_DERIV") == "0", "run with SVO_LK_DERIV=0"
    from stereo_visual_odometry_amd import api
    np.savez(sys.argv[1], **run_batch(api))
    print("lk limits child ok")


if __name__ == "__main__":
    main()
