"""The nine-sequence run of tests/test_gpu_lk_epoch_reach.py: a small, fast-moving occlusion-edge scene through a many-sequence
context, so that the image stream builds the derivative planes and the LK kernel reads them at the levels >= 1.  Imported by the
test for the default run; run as a script in a fresh process with SVO_LK_DERIV=0 (the switch is read once per process) it repeats
the run with the kernel differentiating in registers and writes what the frames returned to the .npz named on the command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lk_deriv_child as ldc  # noqa: E402

B, N_FRAMES = ldc.B, 3
W_IMG, H_IMG = 160, 120                   # w = 21 has three levels here: 160 x 120, 80 x 60, 40 x 30
OVER = dict(win_w=21, win_h=21, max_level=2, bucket_start_row=0, max_translation_norm=5.0)
SEQ = dict(step=0.9, yaw_amp_deg=1.2, movers=0.5)


def streams():
    from stereo_visual_odometry_amd import synthetic as syn
    return [syn.StereoSequence(cal=ldc.calib(W_IMG, H_IMG), n_frames=N_FRAMES, seed=4100 + 17 * s, **SEQ) for s in range(2)]


def projections():
    from stereo_visual_odometry_amd import synthetic as syn
    return syn.projection_matrices(ldc.calib(W_IMG, H_IMG))


def run(api):
    """sequence i plays stream i % 2 -> one flat {name: array}"""
    sq = streams()
    vo = api.BatchVisualOdometry(W_IMG, H_IMG, B, api.default_config(**OVER)); vo.initalize_projection_matricies(*projections())
    out, paths = {}, []
    for k in range(N_FRAMES):
        ok, T = vo.stereo_callback_batch([sq[i % 2].left[k] for i in range(B)], [sq[i % 2].right[k] for i in range(B)])
        for i in range(B):
            ldc.flatten("%d/%d" % (k, i), ldc.record(vo, ok, T, i), out)
        paths.append(vo.last_frame_path())
    vo.close()
    out["paths"] = np.array(paths, np.int64)
    return out


def main():
    assert os.environ.get("SVO_LK_DERIV") == "0", "run with SVO_LK_DERIV=0"
    from stereo_visual_odometry_amd import api
    np.savez(sys.argv[1], **run(api))
    print("lk epoch child ok")


if __name__ == "__main__":
    main()
