"""The GPU side of tests/test_gpu_auto_prior.py, in a fresh process: the frame runs of the predicted-prior tests (include/svo.h,
SVO_PRIOR_LAST_ROTATION) on the scenes of tests/lk_prior_cases.py, written as one flat {name: array} .npz in the record layout of
tests/motion_prior_child.py.  Nothing is judged here.

usage: auto_prior_child.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lk_prior_cases as pc  # noqa: E402
from motion_prior_child import bits, put_records, prior_or_zeros, B_MANY  # noqa: E402

FAILS = 4                                        # the sequence of the nine that gets no prior at frame 1 in the "seed" run
EXPLICIT = 2                                     # the sequence that gets an explicit identity before frame 2 there
IDLE = 1                                         # the sequence that sits out the first submit of frame 2 in the "idle" run


def last_prior(vo, seq):
    """svo_get_last_motion_prior -> [source], and H, Hi as bits (zeros without a prior)"""
    p = vo.last_motion_prior(seq)
    if p is None:
        return np.array([0], np.int64), np.zeros((2, 9), np.uint32)
    return np.array([p[2]], np.int64), np.stack([bits(p[0]).reshape(9), bits(p[1]).reshape(9)])


def put_last_priors(out, key, vo):
    for i in range(vo.n_seq):
        out["%s/%d/source" % (key, i)], out["%s/%d/used" % (key, i)] = last_prior(vo, i)


def new_vo(api, w, h, win, n_seq, auto):
    vo = api.BatchVisualOdometry(w, h, n_seq, api.default_config(**pc.over(win)))
    vo.initalize_projection_matricies(*pc.projections(w, h))
    if auto:
        vo.set_motion_prior_mode("last_rotation")
    return vo


def frame_run(api, out, w, h, win, n_seq, mode):
    """three frames, one call each.  Every mode but "none" bootstraps frame 1 with the ground-truth rotation prior.
    "auto": the mode on, nothing before frame 2.  "host": the mode off, before frame 2 the host restatement of the rule — every
    sequence whose frame 1 returned ok gets set_rotation_prior(T[:3, :3].T).  "plain": the mode off, nothing before frame 2.
    "none": no prior at all.  "seed": the mode on; sequence FAILS gets no prior at frame 1, EXPLICIT an identity before frame 2.
    "off": the mode on for frames 0 and 1, switched off before frame 2."""
    sc = pc.scene(w, h)
    key = "f/%dx%d/%d/%s" % (w, h, n_seq, mode)
    vo = new_vo(api, w, h, win, n_seq, mode in ("auto", "seed", "off"))
    paths = []
    ok = T = None
    for k in range(pc.N_FRAMES):
        if k == 1 and mode == "seed":
            H, Hi = api.motion_prior_from_rotation(pc.projections(w, h)[0], pc.rotation(w, h, 1))
            vo.set_motion_priors(np.stack([H] * n_seq), has=[i != FAILS for i in range(n_seq)], His=np.stack([Hi] * n_seq))
        elif k == 1 and mode != "none":
            vo.set_rotation_prior(pc.rotation(w, h, 1))
        if k == 2 and mode == "host":
            for i in range(n_seq):
                if ok[i]:
                    vo.set_rotation_prior(np.asarray(T[i], np.float64).reshape(4, 4)[:3, :3].T, seq=i)
        if k == 2 and mode == "seed":
            vo.set_motion_prior(np.eye(3, dtype=np.float32), seq=EXPLICIT)
        if k == 2 and mode == "off":
            vo.set_motion_prior_mode("explicit")
        for i in range(n_seq):
            out["%s/%d/%d/pending" % (key, k, i)] = prior_or_zeros(vo, i)      # svo_get_motion_prior before the submit
        ok, T = vo.stereo_callback_batch([sc.left[k]] * n_seq, [sc.right[k]] * n_seq)
        paths.append(vo.last_frame_path())
        put_records(out, "%s/%d" % (key, k), vo, ok, T)
        put_last_priors(out, "%s/%d" % (key, k), vo)
    out[key + "/paths"] = np.array(paths, np.int64)
    out[key + "/mode"] = np.array([vo.motion_prior_mode() == "last_rotation"], np.int64)
    vo.close()


def stats_row(vo, i):
    st = vo.stats[i].as_dict()
    return np.array([st[n] for n in sorted(st)], np.int64)


def in_flight(api, out, dev, w, h, win, n_seq):
    """submit 0, collect, the explicit prior, submit 1, submit 2, collect, collect: frame 2 is enqueued before the host has frame 1's pose"""
    key = "o/flight/%d" % n_seq
    vo = new_vo(api, w, h, win, n_seq, True)
    sub = lambda k, active=None: vo.submit_device([dev[k][0].data_ptr()] * n_seq, [dev[k][1].data_ptr()] * n_seq, w, active=active)
    sub(0); vo.collect()
    vo.set_rotation_prior(pc.rotation(w, h, 1))
    paths = []
    sub(1); paths.append(vo.last_frame_path())
    sub(2); paths.append(vo.last_frame_path())
    for k in (1, 2):
        ok, T = vo.collect()
        for i in range(n_seq):
            out["%s/%d/%d/stats" % (key, k, i)], out["%s/%d/%d/T" % (key, k, i)] = stats_row(vo, i), np.asarray(T[i], np.float64).reshape(16)
        put_last_priors(out, "%s/%d" % (key, k), vo)
    put_records(out, key + "/2", vo, ok, T)
    out[key + "/paths"] = np.array(paths, np.int64)
    vo.close()


def idle_and_reset(api, out, dev, w, h, win, n_seq):
    """sequence IDLE sits out the first submit of frame 2 and takes it at the next one; then it is reset and plays frames 0 and 1 again"""
    key = "o/idle"
    vo = new_vo(api, w, h, win, n_seq, True)
    sub = lambda k, active=None: vo.submit_device([dev[k][0].data_ptr()] * n_seq, [dev[k][1].data_ptr()] * n_seq, w, active=active)
    sub(0); vo.collect()
    vo.set_rotation_prior(pc.rotation(w, h, 1))
    sub(1); vo.collect()
    others, only = [int(i != IDLE) for i in range(n_seq)], [int(i == IDLE) for i in range(n_seq)]
    paths = []
    sub(2, others); paths.append(vo.last_frame_path()); ok, T = vo.collect()
    put_records(out, key + "/first", vo, ok, T); put_last_priors(out, key + "/first", vo)
    sub(2, only); paths.append(vo.last_frame_path()); ok, T = vo.collect()
    put_records(out, key + "/second", vo, ok, T); put_last_priors(out, key + "/second", vo)
    # a frame nobody takes launches nothing
    sub(2, [0] * n_seq); paths.append(vo.last_frame_path()); vo.collect()
    put_last_priors(out, key + "/nobody", vo)
    vo.reset_sequence(IDLE)
    for k in (0, 1):                             # the reset sequence's frames 0 and 1: its first tracked frame is the second
        sub(k, only); paths.append(vo.last_frame_path()); ok, T = vo.collect()
        put_last_priors(out, "%s/reset%d" % (key, k), vo)
        out["%s/reset%d/stats" % (key, k)] = stats_row(vo, IDLE)
    out[key + "/paths"] = np.array(paths, np.int64)
    vo.close()


def errors(api, out, w, h, win):
    from stereo_visual_odometry_amd import _lib
    import ctypes as C
    lib = _lib.lib
    codes = {}
    bgr = api.BatchVisualOdometry(w, h, 1, api.default_config(channels=3, **pc.over(win)))
    codes["bgr"] = lib.svo_set_motion_prior_mode(bgr._h, _lib.PRIOR_LAST_ROTATION); bgr.close()
    fs = api.BatchVisualOdometry(w, h, 1, api.default_config(lk_float_sums=1, **pc.over(win)))
    codes["float_sums"] = lib.svo_set_motion_prior_mode(fs._h, _lib.PRIOR_LAST_ROTATION); fs.close()
    vo = new_vo(api, w, h, win, 1, False)
    codes["unknown_mode"] = lib.svo_set_motion_prior_mode(vo._h, 2)
    codes["negative_mode"] = lib.svo_set_motion_prior_mode(vo._h, -1)
    codes["mode_after_errors"] = int(vo.motion_prior_mode() == "last_rotation")
    src = C.c_int(-7)
    codes["getter_before_collect"] = lib.svo_get_last_motion_prior(vo._h, 0, None, None, C.byref(src))
    sc = pc.scene(w, h)
    vo.stereo_callback_batch([sc.left[0]], [sc.right[0]])
    codes["getter_without_buffers"] = lib.svo_get_last_motion_prior(vo._h, 0, None, None, C.byref(src))
    codes["source_without_buffers"] = src.value
    codes["getter_seq_range"] = lib.svo_get_last_motion_prior(vo._h, 1, None, None, C.byref(src))
    codes["getter_null_source"] = lib.svo_get_last_motion_prior(vo._h, 0, None, None, None)
    codes["set_on"] = lib.svo_set_motion_prior_mode(vo._h, _lib.PRIOR_LAST_ROTATION)
    codes["set_off"] = lib.svo_set_motion_prior_mode(vo._h, _lib.PRIOR_EXPLICIT)
    vo.close()
    for k, v in codes.items():
        out["o/code/" + k] = np.array([v], np.int64)


def main():
    import torch
    from stereo_visual_odometry_amd import api
    assert api._lib.device_count() >= 1, "no HIP device"
    out = {}
    for w, h, win in pc.FRAME_CASES:
        for n_seq in (1, B_MANY):
            for mode in ("auto", "host", "plain"):
                frame_run(api, out, w, h, win, n_seq, mode)
    w, h, win = pc.FRAME_CASES[0]
    for n_seq in (1, B_MANY):
        frame_run(api, out, w, h, win, n_seq, "none")
        frame_run(api, out, w, h, win, n_seq, "off")
    frame_run(api, out, w, h, win, B_MANY, "seed")
    sc = pc.scene(w, h)
    dev = [(torch.from_numpy(sc.left[k]).cuda(), torch.from_numpy(sc.right[k]).cuda()) for k in range(pc.N_FRAMES)]
    torch.cuda.synchronize()
    for n_seq in (1, B_MANY):
        in_flight(api, out, dev, w, h, win, n_seq)
    idle_and_reset(api, out, dev, w, h, win, B_MANY)
    errors(api, out, w, h, win)
    np.savez(sys.argv[1], **out)
    print("auto prior child ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
