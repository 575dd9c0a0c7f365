"""The scenes of tests/test_gpu_lk_deriv_levels.py and the many-sequence runs over them.  Imported by that test for the default
runs; run as a script in a fresh process with SVO_LK_DERIV=0 (the switch is read once per process) it repeats every run without the
derivative pyramid and writes what the frames returned to the .npz named on the command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from gpu_kit import calib  # noqa: E402

B = 9                    # the smallest many-sequence context: from nine sequences on the image stream builds the pyramids ahead
N_FRAMES = 3

# name -> (width, height, config overrides, StereoSequence arguments).
#  four_levels  w = 21 needs every level larger than the window: level 3 of a frame is ceil(size / 8), so 169 is the smallest side
#               with four levels (169 -> 85 -> 43 -> 22).  The height is that; the width keeps 200 so that the stereo disparity (up to
#               17 px) leaves tracks.  Level 3 is 25 x 22: every window there crosses the edge.
#  small_window w = 5 on 64 x 48: four levels down to 8 x 6, narrower than the border.
#  odd          203 x 187: level sizes 102 x 94, 51 x 47, 26 x 24 — odd and even widths, every row-tail shape of the differentiation.
#  borders      the four-level frame with the bucket grid from row 0 and a fast, yawing camera: features sit within w of every
#               border and corner, and tracks leave the frame.
SCENES = {
    "four_levels": (200, 169, dict(win_w=21, win_h=21, max_level=3), dict(step=0.3)),
    "small_window": (64, 48, dict(win_w=5, win_h=5, max_level=3, bucket_start_row=0), dict(step=0.15, cell_px=5.0, depth=(60.0, 140.0))),
    "odd": (203, 187, dict(win_w=21, win_h=21, max_level=3), dict(step=0.3)),
    "borders": (200, 169, dict(win_w=21, win_h=21, max_level=3, bucket_start_row=0), dict(step=0.9, yaw_amp_deg=1.2)),
}


def config_over(name):
    return dict(SCENES[name][2], max_translation_norm=5.0)


def streams(name, n=2, n_frames=N_FRAMES):
    """n distinct sequences of the scene -> [StereoSequence]"""
    from stereo_visual_odometry_amd import synthetic as syn
    w, h, _, kw = SCENES[name]
    return [syn.StereoSequence(cal=calib(w, h), n_frames=n_frames, seed=9000 + 131 * len(name) + 17 * s, **kw) for s in range(n)]


def projections(name):
    from stereo_visual_odometry_amd import synthetic as syn
    w, h = SCENES[name][:2]
    return syn.projection_matrices(calib(w, h))


def record(vo, ok, T, i):
    """everything frame pipeline reports for sequence i, as arrays"""
    st = vo.stats[i].as_dict()
    f = vo.features(i)
    return dict(ok=np.array([bool(ok[i])]), T=np.asarray(T[i], np.float64).reshape(16).copy(), stats=np.array([st[k] for k in sorted(st)], np.int64),
                xy=f[0].view(np.uint32).copy(), age=f[1].copy(), strength=f[2].copy())


def run_scene(api, name):
    """A B-sequence context over the scene (sequence i plays stream i % 2) -> ([frame][sequence] record, [frame] path bits)"""
    w, h = SCENES[name][:2]
    sq = streams(name)
    vo = api.BatchVisualOdometry(w, h, B, api.default_config(**config_over(name))); vo.initalize_projection_matricies(*projections(name))
    out, paths = [], []
    for k in range(N_FRAMES):
        ok, T = vo.stereo_callback_batch([sq[i % 2].left[k] for i in range(B)], [sq[i % 2].right[k] for i in range(B)])
        out.append([record(vo, ok, T, i) for i in range(B)])
        paths.append(vo.last_frame_path())
    vo.close()
    return out, paths


# ---- frames in flight: device images, three frames submitted ahead, an idle mask on two frames and a reset between two others
FL_NAME, FL_B, FL_FRAMES, FL_RESET_SEQ, FL_RESET_BEFORE = "four_levels", 10, 7, 3, 4


def flight_plan():
    """[frame] mask (None: every sequence), and per sequence the index of its stream's frame it is fed (None: idle)"""
    masks = [None] * FL_FRAMES
    m = np.ones(FL_B, bool); m[[1, 4, 7]] = False; masks[2] = m
    m = np.ones(FL_B, bool); m[[0, 4, 9]] = False; masks[5] = m
    nxt = [0] * FL_B
    fed = []
    for k in range(FL_FRAMES):
        a = np.ones(FL_B, bool) if masks[k] is None else masks[k]
        fed.append([nxt[i] if a[i] else None for i in range(FL_B)])
        for i in range(FL_B):
            nxt[i] += int(a[i])
    return masks, fed


def run_flight(api):
    """-> ([frame][sequence] (ok, T, stats) rows, [sequence] feature sets at the end)"""
    import torch
    w, h = SCENES[FL_NAME][:2]
    sq = streams(FL_NAME, n=2, n_frames=FL_FRAMES)
    dev = [[(torch.from_numpy(np.ascontiguousarray(s.left[k])).cuda(), torch.from_numpy(np.ascontiguousarray(s.right[k])).cuda()) for k in range(FL_FRAMES)] for s in sq]
    torch.cuda.synchronize()
    masks, fed = flight_plan()
    vo = api.BatchVisualOdometry(w, h, FL_B, api.default_config(**config_over(FL_NAME))); vo.initalize_projection_matricies(*projections(FL_NAME))

    def submit(k):
        if k == FL_RESET_BEFORE:
            vo.reset_sequence(FL_RESET_SEQ)                          # stream-ordered: lands between frames k - 1 and k, three frames in flight
        lp = [dev[i % 2][j][0].data_ptr() if j is not None else None for i, j in enumerate(fed[k])]
        rp = [dev[i % 2][j][1].data_ptr() if j is not None else None for i, j in enumerate(fed[k])]
        vo.submit_device(lp, rp, w, active=masks[k])

    rows = []
    for k in range(3):
        submit(k)
    for k in range(FL_FRAMES):
        ok, T = vo.collect()
        rows.append([dict(ok=np.array([bool(ok[i])]), T=np.asarray(T[i], np.float64).reshape(16).copy(),
                          stats=np.array([v for _, v in sorted(vo.stats[i].as_dict().items())], np.int64)) for i in range(FL_B)])
        if k + 3 < FL_FRAMES:
            submit(k + 3)
    end = []
    for i in range(FL_B):
        f = vo.features(i)
        end.append(dict(xy=f[0].view(np.uint32).copy(), age=f[1].copy(), strength=f[2].copy()))
    vo.close()
    return rows, end


def flatten(prefix, recs, into):
    for key, v in recs.items():
        into["%s/%s" % (prefix, key)] = v


def everything(api):
    """every run of this module as one flat {name: array}"""
    out = {}
    for name in SCENES:
        frames, paths = run_scene(api, name)
        out["%s/paths" % name] = np.array(paths, np.int64)
        for k, per in enumerate(frames):
            for i, r in enumerate(per):
                flatten("%s/%d/%d" % (name, k, i), r, out)
    rows, end = run_flight(api)
    for k, per in enumerate(rows):
        for i, r in enumerate(per):
            flatten("flight/%d/%d" % (k, i), r, out)
    for i, r in enumerate(end):
        flatten("flight/end/%d" % i, r, out)
    return out


def main():
    assert os.environ.get("SVO_LK_DERIV") == "0", "run with SVO_LK_DERIV=0"
    from stereo_visual_odometry_amd import api
    np.savez(sys.argv[1], **everything(api))
    print("lk deriv child ok")


if __name__ == "__main__":
    main()
