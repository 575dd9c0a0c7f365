"""Reference for detection masks (include/svo.h, "Detection masks"): numpy plus the oracle's stage calls (tests/oracle_lib.py).

mask_filter is the rule as definition.  masked_append is FeatureSet::appendFeaturesFromImage with the filter between the
concatenation and the bucket grid.  MaskedOracleVO is VisualOdometry::stereo_callback composed from the oracle's stage functions
(oracle/orc_vo.c is the same composition in C, without a mask), with masked_append as its detection stage: with no mask, or an
all-255 one, it must reproduce orc_vo_stereo_callback bit for bit (tests/test_detect_mask_ref.py pins that on the CPU).

A mask belongs to a left image: the one passed with a frame is kept beside imageLeftT0_ and applied when that image is scanned, in
the following call.  Single-channel, lk_float_sums = 0 only.
"""
import numpy as np

import oracle_lib as orc


def mask_filter(xy, mask):
    """KeyPointsFilter::runByPixelsMask: an entry at (x, y) stays iff mask[min((int)(y + 0.5f), H-1)][min((int)(x + 0.5f), W-1)] != 0.
    The sum is an f32 sum and the conversion truncates toward zero.  (A coordinate below -0.5 would index before the image; the
    frame pipeline's tracks are never negative — vo.cpp:341-359 — and the kernels clamp such a load to 0, so does this.)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    h, w = mask.shape
    half = np.float32(0.5)
    ix = np.clip((xy[:, 0] + half).astype(np.int32), 0, w - 1)
    iy = np.clip((xy[:, 1] + half).astype(np.int32), 0, h - 1)
    return mask[iy, ix] != 0


def masked_detect(img, threshold, mask):
    """cv::FAST with non-max suppression, then the mask on the survivors -> (xy, response)."""
    xy, resp = orc.fast_detect(img, threshold)
    if mask is None:
        return xy, resp
    keep = mask_filter(xy, mask)
    return xy[keep], resp[keep]


def masked_append(img, feats, mask, cfg, threshold=None):
    """appendFeaturesFromImage(img, threshold) on the feature set feats = (xy, ages, strengths) with a mask over the whole list
    (the existing tracks, then the FAST hits in raster order) -> the new set.  One pass; see masked_detection for the second."""
    h, w = img.shape
    threshold = cfg.fast_threshold if threshold is None else threshold
    xy, resp = orc.fast_detect(img, threshold)
    all_xy = np.concatenate([np.asarray(feats[0], np.float32).reshape(-1, 2), xy])
    ages = np.concatenate([np.asarray(feats[1], np.int32), np.zeros(len(xy), np.int32)])                 # feature_set.cpp:84
    strs = np.concatenate([np.asarray(feats[2], np.int32), resp.astype(np.int32)])                       # :86-87 float -> int
    if mask is not None:
        keep = mask_filter(all_xy, mask)
        all_xy, ages, strs = all_xy[keep], ages[keep], strs[keep]
    return orc.bucket_filter(w, h, all_xy, ages, strs, cfg.buckets_along_height, cfg.buckets_along_width, cfg.bucket_start_row,
                             cfg.features_per_bucket, cfg.age_threshold, cfg.fast_threshold)


def masked_detection(img, feats, mask, cfg):
    """vo.cpp:325-332: the pass at fast_threshold, and the second at a quarter of it when fewer than
    pre_matching_feature_threshold features remain -> (features, second_pass)."""
    feats = masked_append(img, feats, mask, cfg, cfg.fast_threshold)
    if len(feats[1]) < cfg.pre_matching_feature_threshold:
        return masked_append(img, feats, mask, cfg, int(cfg.fast_threshold / 4)), True
    return feats, False


class MaskedOracleVO:
    """stereo_callback from the oracle's stages.  stereo_callback(left, right, mask): `mask` (or None) describes `left`."""

    def __init__(self, cfg=None):
        self.cfg = cfg if cfg is not None else orc.default_config()
        assert self.cfg.channels in (0, 1) and not self.cfg.lk_float_sums
        self.frame_id = 0
        self.feats = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        self.R, self.t, self.last_T = np.eye(3), np.zeros(3), np.eye(4)
        self.tracks = None
        self.second_pass = False
        self.fail_reason = 0
        self.scanned_mask = None                  # the mask the last call's detection applied

    def initalize_projection_matricies(self, Pl, Pr):
        self.Pl = np.ascontiguousarray(Pl, np.float32).reshape(3, 4)
        self.Pr = np.ascontiguousarray(Pr, np.float32).reshape(3, 4)
        self.K = self.Pl[:, :3].copy()                                                                   # vo.cpp:16-25

    def _pyr(self, img):
        c = self.cfg
        return orc.Pyramid(img, (c.win_w, c.win_h), c.max_level)

    def _compact(self, ok):
        ok = np.asarray(ok, bool)
        self.feats = tuple(a[ok] for a in self.feats)

    def _tracks(self, pl0, pr0, pl1, pr1, world=None, inlier=None):
        n = len(pl0)
        self.tracks = dict(pl0=pl0, pr0=pr0, pl1=pl1, pr1=pr1, world=np.zeros((n, 3), np.float32) if world is None else world,
                           inlier=np.zeros(n, np.uint8) if inlier is None else inlier)

    def stereo_callback(self, left, right, mask=None):
        c = self.cfg
        left, right = orc.u8img(left).copy(), orc.u8img(right).copy()
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).copy()
        T_fail = self.last_T.copy()                                                                      # vo.cpp:43-44
        h, w = left.shape
        if self.frame_id == 0:                                                                           # :47-56
            self.imgL0, self.imgR0, self.maskL0 = left, right, mask
            self.pyrL0, self.pyrR0 = self._pyr(left), self._pyr(right)
            self.frame_id = 1
            self.fail_reason = 1
            return False, T_fail
        self.frame_id += 1
        self.scanned_mask = self.maskL0
        self.feats, self.second_pass = masked_detection(self.imgL0, self.feats, self.maskL0, c)         # :325-332, on the PREVIOUS left image
        if c.max_features > 0 and len(self.feats[1]) > c.max_features:
            self.feats = tuple(a[:c.max_features] for a in self.feats)
        n = len(self.feats[1])
        pl0 = self.feats[0].copy()                                                                       # :338
        e = np.zeros((0, 2), np.float32)
        pl1 = pr1 = pr0 = e
        if n > 0:                                                                                        # circularMatching :179-181 (else: the stale pyramids stay)
            l1, r1 = self._pyr(left), self._pyr(right)                                                   # :200-201
            pl1, pr1, pr0, _, ok = orc.circular_match(self.pyrL0, self.pyrR0, l1, r1, pl0, c)            # :203-230
            self.pyrL0, self.pyrR0 = l1, r1                                                              # :231-232
            ok = ok.astype(bool)
            self._compact(ok)                                                                            # :233
            pl0, pl1, pr1, pr0 = pl0[ok], pl1[ok], pr1[ok], pr0[ok]                                      # :234-238
            good = np.ones(len(pl0), bool)
            for p in (pl0, pl1, pr0, pr1):                                                               # :341-359
                good &= ~((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 1] >= h) | (p[:, 0] >= w))
            self._compact(good)                                                                          # :360
            pl0, pl1, pr1, pr0 = pl0[good], pl1[good], pr1[good], pr0[good]
        nt = len(pl0)
        self.feats = (self.feats[0], self.feats[1] + 1, self.feats[2])                                   # :70-72
        self.imgL0, self.imgR0, self.maskL0 = left, right, mask                                          # :74-75, and the image's mask with it
        self._tracks(pl0, pr0, pl1, pr1)
        if nt <= max(4, c.features_threshold):                                                           # :82-84
            self.fail_reason = 2
            return False, T_fail
        world, _ = orc.triangulate(self.Pl, self.Pr, pl0, pr0)                                           # :89-94
        success, self.R, self.t, inl, _ = orc.camera_to_world(self.K, pl1, world, self.R, self.t, c.ransac_iterations,
                                                              c.ransac_reprojection_error, c.ransac_confidence)   # :101-104
        self._tracks(pl0, pr0, pl1, pr1, world)
        if len(inl) < c.features_threshold or not success:                                               # :106-113
            self.fail_reason = 3
            return False, T_fail
        is_ok = np.zeros(nt, np.uint8); is_ok[inl] = 1                                                   # :115-119
        self._tracks(pl0, pr0, pl1, pr1, world, is_ok)
        self.feats = (pl1.copy(), self.feats[1], self.feats[2])                                          # :120
        self._compact(is_ok)                                                                             # :121
        tn = np.sqrt(self.t[0] * self.t[0] + self.t[1] * self.t[1] + self.t[2] * self.t[2])             # :124
        rv = orc.rodrigues_to_vector(self.R)                                                             # :125
        angle = np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])                                   # :126
        if tn > c.max_translation_norm or angle > c.max_rotation_norm:                                   # :129-132
            self.fail_reason = 4
            return False, T_fail
        self.last_T = orc.inverse_transform(self.R, self.t)                                              # :133-135
        self.fail_reason = 0
        return True, self.last_T.copy()

    def features(self):
        return self.feats

    def last_tracks(self):
        return self.tracks


# ------------------------------------------------------------------------------------------------ streams and masks for the tests
_streams = {}


def stream(n_frames, seed, w, h, blank=()):
    """One synthetic w x h stereo stream -> ((lefts, rights), (Pl, Pr)), rendered once per argument set and never written to.
    The frames listed in `blank` are flat grey: the call that receives one loses its tracks (fail_reason 2), the next one finds
    nothing to detect in it, takes the second pass and returns before circularMatching builds pyramids (vo.cpp:179-181)."""
    key = (n_frames, seed, w, h, tuple(blank))
    if key not in _streams:
        from stereo_visual_odometry_amd import synthetic as syn
        cal = dict(syn.KITTI00, width=w, height=h, fx=300.0, fy=300.0, cx=w / 2.0, cy=h / 2.0)
        s = syn.StereoSequence(cal=cal, n_frames=n_frames, seed=seed, step=0.3)
        L, R = [np.ascontiguousarray(a) for a in s.left], [np.ascontiguousarray(a) for a in s.right]
        for k in blank:
            L[k] = np.full((h, w), 128, np.uint8); R[k] = np.full((h, w), 128, np.uint8)
        _streams[key] = ((L, R), syn.projection_matrices(cal))
    return _streams[key]


def band_mask(w, h, x0, x1):
    """everything allowed but the columns [x0, x1)"""
    m = np.full((h, w), 255, np.uint8)
    m[:, max(x0, 0):max(x1, 0)] = 0
    return m


def blob_mask(w, h, seed, n=6):
    """everything allowed but n random rectangles ("cars"); non-zero values vary: any non-zero byte allows"""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    for _ in range(n):
        x, y = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
        m[y:y + int(rng.integers(8, h // 2)), x:x + int(rng.integers(8, w // 3))] = 0
    return m
