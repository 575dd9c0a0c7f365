"""The GPU side of tests/test_gpu_motion_prior.py, in a fresh process: every stage call and frame run of the motion-prior tests on the
inputs of tests/lk_prior_cases.py, written as one flat {name: array} .npz that the test holds to the numpy reference.  Nothing is
judged here.

usage: motion_prior_child.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lk_prior_cases as pc  # noqa: E402

MIXED = (0, 3, 8)                                # the sequences of the nine that get a prior in the mixed batch
B_MANY = 9


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def put_circ(out, key, res):
    for name, a in zip(("pl1", "pr1", "pr0", "plc"), res[:4]):
        out[key + "/" + name] = bits(a)
    out[key + "/ok"] = res[4]


def stage(api, out):
    for w, h, win in pc.STAGE_CASES:
        sc = pc.scene(w, h)
        key = "s/%dx%d/%d" % (w, h, win)
        P, G, _ = pc.track_case(w, h, win)
        for name, g in (("guess", G), ("same", P), ("plain", None)):
            nxt, st = api.lk_track(sc.left[0], sc.left[1], P, win, pc.MAX_LEVEL, guess=g)
            out[key + "/%s/next" % name], out[key + "/%s/status" % name] = bits(nxt), st
        cfg = api.default_config(**pc.over(win))
        pts = pc.fast_points(w, h, pc.N_CIRC)
        for j, (k0, k1, H, Hi) in enumerate(pc.circular_cases(w, h)):
            put_circ(out, key + "/circ%d" % j, api.circular_match_prior(cfg, sc.left[k0], sc.right[k0], sc.left[k1], sc.right[k1], pts, H, Hi))
        # the identity, inverted by the library, against the call without a prior
        put_circ(out, key + "/identity", api.circular_match_prior(cfg, sc.left[0], sc.right[0], sc.left[1], sc.right[1], pts, np.eye(3, dtype=np.float32)))
        put_circ(out, key + "/noprior", api.circularMatching(cfg, sc.left[0], sc.right[0], sc.left[1], sc.right[1], pts))
    # the append the frame test's LK input is compared with, per frame shape
    for w, h, win in pc.FRAME_CASES:
        cfg = api.default_config(**pc.over(win))
        fs = api.FeatureSet()
        fs.appendFeaturesFromImage(pc.scene(w, h).left[0], cfg.fast_threshold, cfg)
        if fs.size() < cfg.pre_matching_feature_threshold:
            fs.appendFeaturesFromImage(pc.scene(w, h).left[0], cfg.fast_threshold // 4, cfg)
        out["append/%dx%d/%d" % (w, h, win)] = bits(fs.points)


def record(vo, ok, T, i):
    f, t = vo.features(i), vo.last_tracks(i)
    st = vo.stats[i].as_dict()
    r = dict(ok=np.array([int(ok[i])]), T=np.asarray(T[i], np.float64).reshape(16), stats=np.array([st[n] for n in sorted(st)], np.int64),
             xy=bits(f[0]), age=f[1], strength=f[2], inlier=t["inlier"])
    for k in ("pl0", "pr0", "pl1", "pr1", "world"):
        r[k] = bits(t[k])
    return r


def put_records(out, key, vo, ok, T):
    for i in range(vo.n_seq):
        for name, a in record(vo, ok, T, i).items():
            out["%s/%d/%s" % (key, i, name)] = a


def prior_or_zeros(vo, seq):
    p = vo.motion_prior(seq)
    return np.zeros((2, 9), np.uint32) if p is None else np.stack([bits(p[0]).reshape(9), bits(p[1]).reshape(9)])


def frame_run(api, out, w, h, win, n_seq, mode):
    """three frames of the scene on every sequence; mode: "none", "prior" (the ground-truth rotation before each tracked frame, through
    svo_motion_prior_from_rotation), "identity", "mixed" (the rotation for the sequences MIXED before frame 1 only)"""
    sc = pc.scene(w, h)
    key = "f/%dx%d/%d/%s" % (w, h, n_seq, mode)
    vo = api.BatchVisualOdometry(w, h, n_seq, api.default_config(**pc.over(win)))
    vo.initalize_projection_matricies(*pc.projections(w, h))
    paths, pending = [], []
    for k in range(pc.N_FRAMES):
        if k >= 1 and mode == "prior":
            vo.set_rotation_prior(pc.rotation(w, h, k))
        elif k >= 1 and mode == "identity":
            vo.set_motion_prior(np.eye(3, dtype=np.float32))
        elif k == 1 and mode == "mixed":
            H, Hi = api.motion_prior_from_rotation(pc.projections(w, h)[0], pc.rotation(w, h, k))     # the "prior" run's bits, inverse included
            vo.set_motion_priors(np.stack([H] * n_seq), has=[i in MIXED for i in range(n_seq)], His=np.stack([Hi] * n_seq))
        before = [vo.motion_prior(i) is not None for i in range(n_seq)]
        out["%s/%d/prior" % (key, k)] = prior_or_zeros(vo, 0)              # H, Hi as the frame will use them
        ok, T = vo.stereo_callback_batch([sc.left[k]] * n_seq, [sc.right[k]] * n_seq)
        after = [vo.motion_prior(i) is not None for i in range(n_seq)]
        paths.append(vo.last_frame_path()); pending.append([before, after])
        put_records(out, "%s/%d" % (key, k), vo, ok, T)
    out[key + "/paths"] = np.array(paths, np.int64)
    out[key + "/pending"] = np.array(pending, np.int64)                  # [frame][before | after][sequence]
    vo.close()


def ordering(api, out):
    """the prior's scope on a lone stream and on a pair: frames in flight, an idle frame, a reset"""
    import torch
    from stereo_visual_odometry_amd import _lib
    w, h, win = pc.FRAME_CASES[0]
    sc = pc.scene(w, h)
    dev = [(torch.from_numpy(sc.left[k]).cuda(), torch.from_numpy(sc.right[k]).cuda()) for k in range(pc.N_FRAMES)]
    torch.cuda.synchronize()
    Pl, Pr = pc.projections(w, h)
    R2 = pc.rotation(w, h, 2)
    # two frames in flight, then the prior, then the third: submit, submit, set, submit, collect x 3
    vo = api.BatchVisualOdometry(w, h, 1, api.default_config(**pc.over(win))); vo.initalize_projection_matricies(Pl, Pr)
    sub = lambda v, k, n=1, active=None: v.submit_device([dev[k][0].data_ptr()] * n, [dev[k][1].data_ptr()] * n, w, active=active)
    paths, pend = [], []
    sub(vo, 0); paths.append(vo.last_frame_path())
    sub(vo, 1); paths.append(vo.last_frame_path())
    vo.set_rotation_prior(R2); pend.append(vo.motion_prior(0) is not None)
    sub(vo, 2); paths.append(vo.last_frame_path()); pend.append(vo.motion_prior(0) is not None)
    for k in range(3):
        ok, T = vo.collect()
        out["o/flight/%d/stats" % k] = np.array([vo.stats[0].as_dict()[n] for n in sorted(vo.stats[0].as_dict())], np.int64)
        out["o/flight/%d/T" % k] = T.reshape(16)
    put_records(out, "o/flight/2", vo, ok, T)
    out["o/flight/paths"], out["o/flight/pending"] = np.array(paths, np.int64), np.array(pend, np.int64)
    vo.close()
    # the same three frames one at a time: what the third frame must be
    vo = api.BatchVisualOdometry(w, h, 1, api.default_config(**pc.over(win))); vo.initalize_projection_matricies(Pl, Pr)
    for k in range(3):
        if k == 2:
            vo.set_rotation_prior(R2)
        ok, T = vo.process_device([dev[k][0].data_ptr()], [dev[k][1].data_ptr()], w)
        out["o/sync/%d/stats" % k] = np.array([vo.stats[0].as_dict()[n] for n in sorted(vo.stats[0].as_dict())], np.int64)
        out["o/sync/%d/T" % k] = T.reshape(16)
    put_records(out, "o/sync/2", vo, ok, T)
    vo.close()
    # an idle frame does not consume: sequence 1 of two gets the prior, idles one frame, then takes frame 1
    vo = api.BatchVisualOdometry(w, h, 2, api.default_config(**pc.over(win))); vo.initalize_projection_matricies(Pl, Pr)
    paths, pend = [], []
    sub(vo, 0, 2); vo.collect()
    vo.set_rotation_prior(pc.rotation(w, h, 1), seq=1)
    pend.append([vo.motion_prior(i) is not None for i in range(2)])
    sub(vo, 1, 2, active=[1, 0]); paths.append(vo.last_frame_path()); vo.collect()
    pend.append([vo.motion_prior(i) is not None for i in range(2)])
    sub(vo, 1, 2, active=[0, 1]); paths.append(vo.last_frame_path()); ok, T = vo.collect()
    pend.append([vo.motion_prior(i) is not None for i in range(2)])
    put_records(out, "o/idle", vo, ok, T)
    # svo_reset_sequence drops a pending prior; a clear does; seq = -1 sets every sequence
    vo.set_rotation_prior(pc.rotation(w, h, 1))
    pend.append([vo.motion_prior(i) is not None for i in range(2)])
    vo.reset_sequence(0)
    pend.append([vo.motion_prior(i) is not None for i in range(2)])
    vo.set_motion_prior(None, seq=1)
    pend.append([vo.motion_prior(i) is not None for i in range(2)])
    out["o/idle/paths"], out["o/idle/pending"] = np.array(paths, np.int64), np.array(pend, np.int64)
    vo.close()
    # errors, as status codes
    lib, ptr = _lib.lib, _lib.ptr
    eye = np.eye(3, dtype=np.float32).reshape(9)
    codes = {}
    bgr = api.BatchVisualOdometry(w, h, 1, api.default_config(channels=3, **pc.over(win)))
    codes["bgr"] = lib.svo_set_motion_prior(bgr._h, -1, ptr(eye), None); bgr.close()
    fs = api.BatchVisualOdometry(w, h, 1, api.default_config(lk_float_sums=1, **pc.over(win)))
    codes["float_sums"] = lib.svo_set_motion_prior(fs._h, -1, ptr(eye), None); fs.close()
    vo = api.VisualOdometry(w, h, api.default_config(**pc.over(win))); vo.initalize_projection_matricies(Pl, Pr)
    sing = np.array([1, 2, 3, 2, 4, 6, 0, 0, 1], np.float32)
    nonf = eye.copy(); nonf[4] = np.inf
    nan_i = eye.copy(); nan_i[0] = np.nan
    codes["singular"] = lib.svo_set_motion_prior(vo._h, 0, ptr(sing), None)
    codes["singular_with_inverse"] = lib.svo_set_motion_prior(vo._h, 0, ptr(sing), ptr(eye))     # the caller's Hi is taken as given
    lib.svo_set_motion_prior(vo._h, 0, None, None)
    codes["non_finite"] = lib.svo_set_motion_prior(vo._h, 0, ptr(nonf), None)
    codes["non_finite_inverse"] = lib.svo_set_motion_prior(vo._h, 0, ptr(eye), ptr(nan_i))
    codes["seq_range"] = lib.svo_set_motion_prior(vo._h, 1, ptr(eye), None)
    codes["pending_after_errors"] = int(vo.motion_prior(0) is not None)
    vo.stereo_callback(sc.left[0], sc.right[0])
    vo.set_motion_prior(eye)
    n = 4
    p0 = np.array([[50, 60], [100, 80], [150, 90], [200, 100]], np.float32)
    o4 = [np.zeros((n, 2), np.float32) for _ in range(4)]; okm = np.zeros(n, np.uint8)
    codes["member_with_pending"] = lib.svo_circular_matching(vo._h, ptr(sc.left[1]), ptr(sc.right[1]), w, n, ptr(p0), ptr(o4[0]), ptr(o4[1]), ptr(o4[2]), ptr(o4[3]), ptr(okm))
    vo.set_motion_prior(None)
    codes["member_after_clear"] = lib.svo_circular_matching(vo._h, ptr(sc.left[1]), ptr(sc.right[1]), w, n, ptr(p0), ptr(o4[0]), ptr(o4[1]), ptr(o4[2]), ptr(o4[3]), ptr(okm))
    vo.close()
    for k, v in codes.items():
        out["o/code/" + k] = np.array([v], np.int64)


def main():
    from stereo_visual_odometry_amd import api
    assert api._lib.device_count() >= 1, "no HIP device"
    out = {}
    stage(api, out)
    for w, h, win in pc.FRAME_CASES:
        for n_seq in (1, B_MANY):
            for mode in ("none", "prior", "identity"):
                frame_run(api, out, w, h, win, n_seq, mode)
    frame_run(api, out, *pc.FRAME_CASES[0], B_MANY, "mixed")
    ordering(api, out)
    np.savez(sys.argv[1], **out)
    print("motion prior child ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
