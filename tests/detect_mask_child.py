"""Run in a fresh process with SVO_GRAPH=1 (test_gpu_detect_mask.py::test_graph_mode_runs_masked_frames_from_the_launch_list): the
runs listed in RUNS, written to the .npz named on the command line for the parent to compare with its own launch-list runs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

RUNS = [("lone", 1), ("many", 9)]                     # name, sequences
MASKED = [False, True, True, False, False]            # set before call 0, cleared before call 2: calls 1 and 2 scan masked images
W, H = 323, 163


def one_run(api, n_seq):
    """-> (T [frame][seq], ok [frame][seq], svo_get_last_frame_path per frame)"""
    import detect_mask_ref as ref
    base = [ref.stream(5, 900 + 31 * i, W, H) for i in range(min(n_seq, 3))]
    vo = api.BatchVisualOdometry(W, H, n_seq, api.default_config(max_translation_norm=2.0))
    vo.initalize_projection_matricies(*base[0][1])
    Ts, oks, paths = [], [], []
    for k in range(5):
        if k == 0:
            vo.set_detection_mask(ref.blob_mask(W, H, 5))
            if n_seq > 1:
                vo.set_detection_mask(ref.blob_mask(W, H, 6), 1)
        if k == 2:
            vo.clear_detection_mask()
        ok, T = vo.stereo_callback_batch([base[i % len(base)][0][0][k] for i in range(n_seq)], [base[i % len(base)][0][1][k] for i in range(n_seq)])
        Ts.append(T); oks.append(ok); paths.append(vo.last_frame_path())
    vo.close()
    return np.array(Ts), np.array(oks), paths


def main():
    assert os.environ.get("SVO_GRAPH") == "1", "run with SVO_GRAPH=1"
    from stereo_visual_odometry_amd import api
    out = {}
    for name, n_seq in RUNS:
        T, ok, paths = one_run(api, n_seq)
        out[name + "_T"], out[name + "_ok"], out[name + "_paths"] = T, ok, np.array(paths)
    np.savez(sys.argv[1], **out)
    print("detect mask child ok")


if __name__ == "__main__":
    main()
