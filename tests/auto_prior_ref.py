"""The CPU side of the predicted-prior tests (include/svo.h, SVO_PRIOR_LAST_ROTATION): the frame pipeline of oracle/orc_vo.c restated
over the oracle's own pieces, with lk_prior_ref.circular — the numpy reference that takes a prior — where orc_vo.c runs its circular
matching, so that a sequence of frames can be played with a prior per frame.  Used for one thing: the state before frame 2 of the
lk_prior_cases scene (after frame 1 ran with the ground-truth rotation prior, which is how every GPU run of
tests/test_gpu_auto_prior.py bootstraps) and what frame pair (1, 2) keeps with no prior, with frame 1's own rotation (the stale,
predicted prior) and with the true one."""
import functools

import numpy as np

import oracle_lib as orc
import lk_prior_cases as pc
import lk_prior_ref as ref


def frame(w, h, win, k, state, H, Hi):
    """stereo_callback of frame k >= 1 (orc_vo.c:169-267) on `state` = dict(xy, age, st, R, t), with the prior (H, Hi) or None ->
    (ok, the new state, dict(n_into_lk, n_after_circular, n_after_bounds, fail_reason))"""
    cfg = orc.default_config(**pc.over(win))
    img = pc.scene(w, h).left[k - 1]
    xy, age, st = pc.append_features(img, cfg, state["xy"], state["age"], state["st"])
    if len(xy) < cfg.pre_matching_feature_threshold:
        xy, age, st = pc.append_features(img, cfg, xy, age, st, cfg.fast_threshold // 4)
    c = pc.circular_cached(w, h, win, k, xy, H, Hi, cfg)
    keep = c["ok"].astype(bool) & c["inb"]
    stats = dict(n_into_lk=len(xy), n_after_circular=int(c["ok"].sum()), n_after_bounds=int(keep.sum()), fail_reason=0)
    new = dict(xy=xy[keep], age=age[keep] + 1, st=st[keep], R=state["R"], t=state["t"])
    if keep.sum() <= max(4, cfg.features_threshold):
        stats["fail_reason"] = 2
        return False, new, stats
    Pl, Pr = pc.projections(w, h)
    world, _ = orc.triangulate(Pl, Pr, xy[keep], c["pr0"][keep])
    ok, R, t, inl, _ = orc.camera_to_world(Pl.reshape(3, 4)[:, :3], c["pl1"][keep], world, state["R"], state["t"], cfg.ransac_iterations,
                                           cfg.ransac_reprojection_error, cfg.ransac_confidence)
    new["R"], new["t"] = R, t
    if len(inl) < cfg.features_threshold or not ok:
        stats["fail_reason"] = 3
        return False, new, stats
    m = np.zeros(int(keep.sum()), bool); m[inl] = True
    new.update(xy=c["pl1"][keep][m], age=new["age"][m], st=new["st"][m])
    tn, angle = np.linalg.norm(t), np.linalg.norm(orc.rodrigues_to_vector(R))
    if tn > cfg.max_translation_norm or angle > cfg.max_rotation_norm:
        stats["fail_reason"] = 4
        return False, new, stats
    return True, new, stats


@functools.lru_cache(maxsize=None)
def after_frame_one(w, h, win):
    """(ok, state, stats) of frame 1 with the ground-truth rotation prior, from an empty feature set"""
    empty = dict(xy=None, age=None, st=None, R=np.eye(3), t=np.zeros(3))
    return frame(w, h, win, 1, empty, *pc.homography(w, h, 1))


@functools.lru_cache(maxsize=None)
def frame_two(w, h, win):
    """{"none" | "stale" | "true": stats of frame 2}, and the angle in degrees of the stale and of the true rotation"""
    ok, state, _ = after_frame_one(w, h, win)
    assert ok
    Pl, _ = pc.projections(w, h)
    priors = dict(none=(None, None), stale=ref.rotation_homography(Pl, state["R"]), true=pc.homography(w, h, 2))
    deg = lambda R: float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))
    return {k: frame(w, h, win, 2, state, *p)[2] for k, p in priors.items()}, deg(state["R"]), deg(pc.rotation(w, h, 2))
