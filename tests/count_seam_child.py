"""Runs one case of tests/count_seam_cases.py on the GPU and records everything a frame leaves behind; tests/test_gpu_count_seams.py
compares the records with the references.  Imported by that test for the cases it runs itself, and started as a fresh process for
the one that needs SVO_FORCE_LEAN=1 (read once per process).
Usage: count_seam_child.py CASE OUT.pkl"""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import count_seam_cases as cs  # noqa: E402


def state(vo, i, tracks_on):
    """The synchronising reads of sequence i: feature set, compacted tracks, feature ids."""
    out = dict(feats=vo.features(i), tracks=vo.last_tracks(i))
    if tracks_on:
        out["ids"] = vo.feature_ids(i)
    return out


def rows_of(vo, i, ok, T, tracks_on):
    out = dict(ok=bool(ok[i]), T=np.array(T[i], np.float64).reshape(4, 4), stats=vo.stats[i].as_dict())
    if tracks_on:
        out["obs"], out["n_tracks"] = vo.last_track_obs(i, with_count=True)
    return out


def run_case(case):
    """-> per call dict(path, seqs): seqs[i] holds ok, T, stats, (obs, n_tracks) and — where no later frame is in flight — feats,
    tracks, (ids).  SVO_GRAPH / SVO_FORCE_LEAN are the caller's to set."""
    from stereo_visual_odometry_amd import api
    B, on = case.B, case.track_rows is not None
    vo = api.BatchVisualOdometry(cs.W, cs.H, B, api.default_config(**cs.OVER))
    vo.initalize_projection_matricies(*cs.projections())
    if on:
        vo.set_track_output(case.track_rows)
    F = [cs.frames(s) for s in case.streams]
    plan, out = case.plan(), []
    pick = lambda k, cam: [F[i][cam][j] if j is not None else None for i, j in enumerate(plan[k])]
    if case.mode != "inflight":
        for k, act in enumerate(case.steps):
            ok, T = vo.stereo_callback_batch(pick(k, 0), pick(k, 1), active=act)
            out.append(dict(path=vo.last_frame_path(), seqs=[dict(rows_of(vo, i, ok, T, on), **state(vo, i, on)) for i in range(B)]))
    else:
        import torch
        dev = {}
        for i, s in enumerate(case.streams):                          # sequences that share a stream share its device frames
            if s not in dev:
                dev[s] = [[torch.from_numpy(np.array(a)).cuda() for a in cam] for cam in F[i]]
        torch.cuda.synchronize()

        def submit(k):
            ptrs = lambda cam: [dev[case.streams[i]][cam][j].data_ptr() if j is not None else None for i, j in enumerate(plan[k])]
            vo.submit_device(ptrs(0), ptrs(1), cs.W, active=case.steps[k])
            return vo.last_frame_path()

        paths = [submit(0)]
        for k in range(len(plan)):
            if k + 1 < len(plan):
                paths.append(submit(k + 1))                           # two frames in flight
            ok, T = vo.collect()
            out.append(dict(path=paths[k], seqs=[rows_of(vo, i, ok, T, on) for i in range(B)]))
        for i in range(B):
            out[-1]["seqs"][i].update(state(vo, i, on))
        del dev
    vo.close()
    return out


if __name__ == "__main__":
    with open(sys.argv[2], "wb") as f:
        pickle.dump(run_case(cs.BY_NAME[sys.argv[1]]), f)
    print("count seam child ok")
