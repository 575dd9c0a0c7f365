"""Reference for track ids and observation rows (include/svo.h, "Track ids and per-frame stereo observations"): numpy plus the
oracle's stage calls (tests/oracle_lib.py).

IdOracleVO is VisualOdometry::stereo_callback composed from the oracle's stages exactly as tests/detect_mask_ref.py's
MaskedOracleVO is, with the identity rule carried through; with the ids ignored it must reproduce MaskedOracleVO(mask=None) bit
for bit (tests/test_track_ids_ref.py pins that on the CPU).

The identity rule, restated.  Per sequence a counter next_id (int64), 0 at creation and after a reset.
 1. Detection pass (each of the two).  The pass publishes n_out entries in bucket-raster order.  An entry that came from the
    existing list (rank < n_old in the pass's input list: the tracks come first, so a track that ties with a fresh FAST hit wins as
    first-come) keeps its id; a fresh FAST hit at output position p gets next_id + p; then next_id += n_out.  The second pass applies
    the same rule to the first pass's output, so a first-pass newcomer displaced in the second pass burns its id.
 2. Circular + bounds compaction (stable): the id of feature i goes with it; features beyond max_features drop out with their ids.
 3. Inlier compaction (fail_reason 0 or 4 only): new feature pos takes the id of the pos-th inlier track.  On fail_reason 2 and 3
    the feature set, and so its ids, is step 2's output.
 4. Observation row i of a frame is track i: its id, pl0 / pr0 / pl1 / pr1, world[i], inlier[i] and the age after this frame's
    increment.  fail_reason 2: no triangulation — xyz 0 0 0, HAS_XYZ clear.  INLIER only where the inlier vector was built
    (fail_reason 0 or 4).
"""
import numpy as np

import oracle_lib as orc
from fast_ref import bucket_index, bucket_score

OBS_INLIER, OBS_HAS_XYZ = 1, 2
# svo_track_obs (include/svo.h), 64 bytes
OBS_DTYPE = np.dtype([("id", "<i8"), ("l0", "<f4", 2), ("r0", "<f4", 2), ("l1", "<f4", 2), ("r1", "<f4", 2),
                      ("xyz", "<f4", 3), ("age", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert OBS_DTYPE.itemsize == 64


def bucket_filter_idx(w, h, xy, ages, strengths, bah, baw, start_row, per_bucket, age_thr, fast_thr):
    """tests/fast_ref.py's bucket_filter (FeatureSet::filterByBucketLocationInternal as written) with the source indices returned:
    -> (xy, ages, strengths, idx) in bucket-raster order, idx[p] = the rank in the input list of output entry p."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    bucket_h, bucket_w = -(-h // bah), -(-w // baw)
    buckets = [[] for _ in range(bah * baw)]
    for i in range(len(xy)):
        bh, bw = bucket_index(xy[i, 1], bucket_h), bucket_index(xy[i, 0], bucket_w)
        if bh < 0 or bh >= bah or bw < 0 or bw >= baw:
            continue
        cap = per_bucket if bh >= start_row else 0
        age, st = int(ages[i]), int(strengths[i])
        if cap == 0 or age >= age_thr:
            continue
        b = buckets[bh * baw + bw]
        if len(b) < cap:
            b.append((i, age, st))
            continue
        scores = [bucket_score(a, s, fast_thr) for _, a, s in b]
        lowest = scores.index(min(scores))
        if bucket_score(age, st, fast_thr) > scores[lowest]:
            b[lowest] = (i, age, st)
    flat = [e for b in buckets for e in b]
    idx = np.array([e[0] for e in flat], np.int64).reshape(-1)
    return (xy[idx].reshape(-1, 2).copy(), np.array([e[1] for e in flat], np.int32).reshape(-1),
            np.array([e[2] for e in flat], np.int32).reshape(-1), idx)


def append_with_ids(img, feats, ids, next_id, cfg, threshold):
    """One detection pass (rule 1) -> (features, ids, next_id)."""
    h, w = img.shape
    xy, resp = orc.fast_detect(img, threshold)
    n_old = len(ids)
    all_xy = np.concatenate([np.asarray(feats[0], np.float32).reshape(-1, 2), xy])
    ages = np.concatenate([np.asarray(feats[1], np.int32), np.zeros(len(xy), np.int32)])
    strs = np.concatenate([np.asarray(feats[2], np.int32), resp.astype(np.int32)])
    oxy, oages, ostrs, idx = bucket_filter_idx(w, h, all_xy, ages, strs, cfg.buckets_along_height, cfg.buckets_along_width,
                                               cfg.bucket_start_row, cfg.features_per_bucket, cfg.age_threshold, cfg.fast_threshold)
    n_out = len(idx)
    old = idx < n_old
    new_ids = next_id + np.arange(n_out, dtype=np.int64)
    new_ids[old] = ids[idx[old]]
    return (oxy, oages, ostrs), new_ids, next_id + n_out


class IdOracleVO:
    """stereo_callback from the oracle's stages with ids.  features() / last_tracks() as MaskedOracleVO's; feature_ids(), obs()."""

    def __init__(self, cfg=None):
        self.cfg = cfg if cfg is not None else orc.default_config()
        assert self.cfg.channels in (0, 1) and not self.cfg.lk_float_sums and self.cfg.features_per_bucket == 1
        self.reset()

    def reset(self):
        """svo_reset_sequence: the constructor's state, the projection matrices kept."""
        self.frame_id = 0
        self.feats = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        self.ids = np.zeros(0, np.int64)
        self.next_id = 0
        self.next_id_before_detect = 0
        self.R, self.t, self.last_T = np.eye(3), np.zeros(3), np.eye(4)
        self.tracks = None
        self.track_ids = np.zeros(0, np.int64)
        self.track_ages = np.zeros(0, np.int32)
        self.second_pass = False
        self.fail_reason = 0

    def assign_ids(self):
        """svo_set_track_output switching on: the features held now get next_id + index."""
        n = len(self.feats[1])
        self.ids = self.next_id + np.arange(n, dtype=np.int64)
        self.next_id += n

    def initalize_projection_matricies(self, Pl, Pr):
        self.Pl = np.ascontiguousarray(Pl, np.float32).reshape(3, 4)
        self.Pr = np.ascontiguousarray(Pr, np.float32).reshape(3, 4)
        self.K = self.Pl[:, :3].copy()

    def _pyr(self, img):
        c = self.cfg
        return orc.Pyramid(img, (c.win_w, c.win_h), c.max_level)

    def _compact(self, ok):
        ok = np.asarray(ok, bool)
        self.feats = tuple(a[ok] for a in self.feats)
        self.ids = self.ids[ok]

    def _tracks(self, pl0, pr0, pl1, pr1, world=None, inlier=None):
        n = len(pl0)
        self.tracks = dict(pl0=pl0, pr0=pr0, pl1=pl1, pr1=pr1, world=np.zeros((n, 3), np.float32) if world is None else world,
                           inlier=np.zeros(n, np.uint8) if inlier is None else inlier)

    def stereo_callback(self, left, right):
        c = self.cfg
        left, right = orc.u8img(left).copy(), orc.u8img(right).copy()
        T_fail = self.last_T.copy()
        h, w = left.shape
        if self.frame_id == 0:
            self.imgL0, self.imgR0 = left, right
            self.pyrL0, self.pyrR0 = self._pyr(left), self._pyr(right)
            self.frame_id = 1
            self.fail_reason = 1
            self.tracks = None
            self.track_ids = np.zeros(0, np.int64); self.track_ages = np.zeros(0, np.int32)
            return False, T_fail
        self.frame_id += 1
        self.next_id_before_detect = self.next_id
        self.feats, self.ids, self.next_id = append_with_ids(self.imgL0, self.feats, self.ids, self.next_id, c, c.fast_threshold)   # rule 1
        self.second_pass = len(self.ids) < c.pre_matching_feature_threshold
        if self.second_pass:
            self.feats, self.ids, self.next_id = append_with_ids(self.imgL0, self.feats, self.ids, self.next_id, c, int(c.fast_threshold / 4))
        if c.max_features > 0 and len(self.ids) > c.max_features:                                        # rule 2: the rest drop out with their ids
            self.feats = tuple(a[:c.max_features] for a in self.feats); self.ids = self.ids[:c.max_features]
        n = len(self.ids)
        pl0 = self.feats[0].copy()
        e = np.zeros((0, 2), np.float32)
        pl1 = pr1 = pr0 = e
        if n > 0:
            l1, r1 = self._pyr(left), self._pyr(right)
            pl1, pr1, pr0, _, ok = orc.circular_match(self.pyrL0, self.pyrR0, l1, r1, pl0, c)
            self.pyrL0, self.pyrR0 = l1, r1
            ok = ok.astype(bool)
            self._compact(ok)                                                                            # rule 2
            pl0, pl1, pr1, pr0 = pl0[ok], pl1[ok], pr1[ok], pr0[ok]
            good = np.ones(len(pl0), bool)
            for p in (pl0, pl1, pr0, pr1):
                good &= ~((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 1] >= h) | (p[:, 0] >= w))
            self._compact(good)
            pl0, pl1, pr1, pr0 = pl0[good], pl1[good], pr1[good], pr0[good]
        nt = len(pl0)
        self.feats = (self.feats[0], self.feats[1] + 1, self.feats[2])
        self.track_ids, self.track_ages = self.ids.copy(), self.feats[1].copy()                          # rule 4: the row's id and age
        self.imgL0, self.imgR0 = left, right
        self._tracks(pl0, pr0, pl1, pr1)
        if nt <= max(4, c.features_threshold):
            self.fail_reason = 2
            return False, T_fail
        world, _ = orc.triangulate(self.Pl, self.Pr, pl0, pr0)
        success, self.R, self.t, inl, _ = orc.camera_to_world(self.K, pl1, world, self.R, self.t, c.ransac_iterations,
                                                              c.ransac_reprojection_error, c.ransac_confidence)
        self._tracks(pl0, pr0, pl1, pr1, world)
        if len(inl) < c.features_threshold or not success:
            self.fail_reason = 3
            return False, T_fail
        is_ok = np.zeros(nt, np.uint8); is_ok[inl] = 1
        self._tracks(pl0, pr0, pl1, pr1, world, is_ok)
        self.feats = (pl1.copy(), self.feats[1], self.feats[2])
        self._compact(is_ok)                                                                             # rule 3
        tn = np.sqrt(self.t[0] * self.t[0] + self.t[1] * self.t[1] + self.t[2] * self.t[2])
        rv = orc.rodrigues_to_vector(self.R)
        angle = np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
        if tn > c.max_translation_norm or angle > c.max_rotation_norm:
            self.fail_reason = 4
            return False, T_fail
        self.last_T = orc.inverse_transform(self.R, self.t)
        self.fail_reason = 0
        return True, self.last_T.copy()

    def features(self):
        return self.feats

    def feature_ids(self):
        return self.ids

    def last_tracks(self):
        return self.tracks

    def obs(self):
        """The rows of the last frame this sequence took (rule 4), all of them, as svo_track_obs."""
        t = self.tracks
        n = 0 if t is None or self.fail_reason == 1 else len(t["pl0"])
        rows = np.zeros(n, OBS_DTYPE)
        if n == 0:
            return rows
        fr = self.fail_reason
        has_xyz, has_inl = fr in (0, 3, 4), fr in (0, 4)
        rows["id"] = self.track_ids
        rows["l0"], rows["r0"], rows["l1"], rows["r1"] = t["pl0"], t["pr0"], t["pl1"], t["pr1"]
        if has_xyz:
            rows["xyz"] = t["world"]
        rows["age"] = self.track_ages
        rows["flags"] = (t["inlier"].astype(np.int32) * OBS_INLIER if has_inl else 0) + (OBS_HAS_XYZ if has_xyz else 0)
        return rows


# ------------------------------------------------------------------------------------------------ streams for the tests
_streams = {}


def stream(n_frames, seed, w, h, blank=(), movers=0.0):
    """One synthetic w x h stereo stream with detect_mask_ref.stream's calibration (fx = fy = 300, step 0.3) -> ((lefts, rights),
    (Pl, Pr)), rendered once per argument set and never written to.  movers: the fraction of the pixels an independently moving
    foreground layer covers (its tracks are RANSAC's outliers).  blank: frames that are flat grey."""
    key = (n_frames, seed, w, h, tuple(blank), float(movers))
    if key not in _streams:
        from stereo_visual_odometry_amd import synthetic as syn
        cal = dict(syn.KITTI00, width=w, height=h, fx=300.0, fy=300.0, cx=w / 2.0, cy=h / 2.0)
        s = syn.StereoSequence(cal=cal, n_frames=n_frames, seed=seed, step=0.3, movers=movers)
        L, R = [np.ascontiguousarray(a) for a in s.left], [np.ascontiguousarray(a) for a in s.right]
        for k in blank:
            L[k] = np.full((h, w), 128, np.uint8); R[k] = np.full((h, w), 128, np.uint8)
        _streams[key] = ((L, R), syn.projection_matrices(cal))
    return _streams[key]
