"""Run in a fresh process with SVO_GRAPH=1 (test_gpu_input_format.py::test_graph_mode_gives_the_same_results): the converting
runs listed in RUNS, every frame a replayed graph, written to the .npz named on the command line for the parent to compare with
its own launch-list runs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

RUNS = [("lone", 1, "host", "bgr8"), ("many", 9, "device", "yuv422")]   # name, sequences, input, format


def one_run(api, run, grey_streams, coloured, cfg_for, n_seq, mode, fmt):
    w, h = 323, 163
    base, P = grey_streams(3 if n_seq > 1 else 1, 5, 1700 + n_seq, w, h)
    col, _ = coloured([base[i % len(base)] for i in range(n_seq)], fmt, seed=90 + n_seq)
    return run(api, w, h, cfg_for(api), col, P, mode, fmt=fmt)


def main():
    assert os.environ.get("SVO_GRAPH") == "1", "run with SVO_GRAPH=1"
    import test_gpu_input_format as t
    from stereo_visual_odometry_amd import api
    out = {}
    for name, n_seq, mode, fmt in RUNS:
        (rows, _), paths = one_run(api, t.run, t.grey_streams, t.coloured, t.cfg_for, n_seq, mode, fmt)
        out[name + "_T"] = np.array([[r[1] for r in fr] for fr in rows])
        out[name + "_ok"] = np.array([[r[0] for r in fr] for fr in rows])
        out[name + "_stats"] = np.array([[list(r[2].values()) for r in fr] for fr in rows])
        out[name + "_paths"] = np.array(paths)
    np.savez(sys.argv[1], **out)
    print("input format child ok")


if __name__ == "__main__":
    main()
