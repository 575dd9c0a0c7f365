"""The detection front written from its definition, in numpy and plain Python: FAST-9/16 scores, strict 3x3 non-max
suppression, the bucket grid and the two-pass detection chain of a frame.

TEST INFRASTRUCTURE ONLY.  Nothing here restates cv::FAST's cornerScore arithmetic (which both the HIP kernel and
oracle/orc_fast.c follow): a pixel is a corner at t iff 9 contiguous pixels of its 16-pixel circle are all brighter than
v + t or all darker than v - t, and its score is the largest t at which that still holds.  The bucket filter is a sequential
list-of-lists restatement of Bucket::add_feature / filterByBucketLocationInternal.  No ctypes, no oracle.
"""
import numpy as np

# Bresenham circle of radius 3, (dx, dy), consecutive entries adjacent on the circle
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
ARC = 9


def clamp_threshold(th):
    return min(max(int(th), 0), 255)


def _arc_strength(img):
    """(h, w) int32: for every tested pixel (rows 3..h-4, cols 3..w-4) the largest m such that some 9 contiguous circle pixels
    all differ from the centre by at least m on the same side (brighter, or darker); 0 elsewhere and where no arc is one-sided."""
    img = np.asarray(img)
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    a = img.astype(np.int32)
    v = a[3:h - 3, 3:w - 3]
    diff = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in CIRCLE])    # p_k - v, (16, h-6, w-6)
    best = np.zeros_like(v)
    for k in range(16):
        arc = diff[[(k + j) % 16 for j in range(ARC)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))       # all brighter by >= m / all darker by >= m
    out[3:h - 3, 3:w - 3] = best
    return out


def _nms(raw, corner):
    """strictly greater than all eight neighbours of the raw score map (zeros outside the tested band)"""
    h, w = raw.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = raw
    keep = corner.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= raw > p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    return keep


def fast_scores(img, th, nonmax=True):
    """-> (score u8 map, kept bool map).  Without nonmax: every corner with its score.  With it: the corners that beat all eight
    neighbours, the score map zero elsewhere.  `kept` is separate from `score` because a corner can score 0 at th = 0."""
    th = clamp_threshold(th)
    m = _arc_strength(img)
    corner = m > th                                   # an arc all > v + th, or all < v - th
    raw = np.where(corner, m - 1, 0)                  # still a corner at t' iff m > t': the largest such t' is m - 1
    kept = _nms(raw, corner) if nonmax else corner
    return np.where(kept, raw, 0).astype(np.uint8), kept


def literal_max_threshold(img):
    """By the letter, for small images: the corner predicate tested at every t in 0..255 -> (h, w) int32 of the largest t that
    passes, -1 where none does."""
    img = np.asarray(img)
    h, w = img.shape
    out = np.full((h, w), -1, np.int32)

    def is_corner(x, y, t):
        v = int(img[y, x])
        ring = [int(img[y + dy, x + dx]) for dx, dy in CIRCLE]
        for side in (lambda p: p > v + t, lambda p: p < v - t):
            flags = [side(p) for p in ring]
            if any(all(flags[(k + j) % 16] for j in range(ARC)) for k in range(16)):
                return True
        return False

    for y in range(3, h - 3):
        for x in range(3, w - 3):
            out[y, x] = max([t for t in range(256) if is_corner(x, y, t)], default=-1)
    return out


def fast_scores_literal(img, th, nonmax=True, max_t=None):
    """fast_scores from literal_max_threshold (pass it as max_t to reuse it across thresholds)"""
    th = clamp_threshold(th)
    max_t = literal_max_threshold(img) if max_t is None else max_t
    corner = max_t >= th                              # the predicate is monotone in t
    raw = np.where(corner, max_t, 0)
    kept = _nms(raw, corner) if nonmax else corner
    return np.where(kept, raw, 0).astype(np.uint8), kept


def fast_keypoints(img, th, nonmax=True):
    """kept pixels in raster order -> ((n, 2) f32 of (x, y), (n,) f32 responses)"""
    score, kept = fast_scores(img, th, nonmax)
    ys, xs = np.nonzero(kept)                         # row-major: raster order
    return np.stack([xs, ys], 1).astype(np.float32).reshape(-1, 2), score[ys, xs].astype(np.float32)


# ---------------------------------------------------------------------------- bucket grid
def _cdiv(a, b):
    """C integer division: truncation toward zero (Python's // floors)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def bucket_score(age, strength, fast_thr):
    return int(age) + _cdiv(int(strength) - int(fast_thr), 20)


def bucket_index(coord, size):
    """f32 division, then truncation toward zero"""
    return int(np.float32(coord) / np.float32(size))


def bucket_filter(w, h, xy, ages, strengths, bah, baw, start_row, per_bucket, age_thr, fast_thr, trace=None):
    """-> (xy (m, 2) f32, ages (m,) i32, strengths (m,) i32) in bucket-raster order.
    trace: a dict that receives how many offers to a full bucket were decided by a tie — "tie_kept" (the newcomer equals the
    minimum and stays out) and "tie_first_min" (it replaces the first of several equal minima)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    bucket_h, bucket_w = -(-h // bah), -(-w // baw)                  # ceiling division
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
        lowest = scores.index(min(scores))                           # the first minimum
        new = bucket_score(age, st, fast_thr)
        if trace is not None:
            trace["tie_kept"] = trace.get("tie_kept", 0) + (new == scores[lowest])
            trace["tie_first_min"] = trace.get("tie_first_min", 0) + (new > scores[lowest] and scores.count(scores[lowest]) > 1)
        if new > scores[lowest]:                                     # strictly better
            b[lowest] = (i, age, st)
    flat = [e for b in buckets for e in b]
    idx = [e[0] for e in flat]
    return (xy[idx].reshape(-1, 2).copy(), np.array([e[1] for e in flat], np.int32).reshape(-1),
            np.array([e[2] for e in flat], np.int32).reshape(-1))


def append_features(img, th, xy, ages, strengths, bah, baw, start_row, per_bucket, age_thr, fast_thr):
    """existing tracks, then the image's keypoints with age 0 and strength = response, through the bucket filter"""
    h, w = np.asarray(img).shape
    kxy, resp = fast_keypoints(img, th)
    xy = np.concatenate([np.asarray(xy, np.float32).reshape(-1, 2), kxy])
    ages = np.concatenate([np.asarray(ages, np.int32).reshape(-1), np.zeros(len(kxy), np.int32)])
    strengths = np.concatenate([np.asarray(strengths, np.int32).reshape(-1), resp.astype(np.int32)])
    return bucket_filter(w, h, xy, ages, strengths, bah, baw, start_row, per_bucket, age_thr, fast_thr)


def detect_for_frame(img, cfg, existing=None):
    """Detection of one frame -> (xy, ages, strengths, second_pass): a pass at fast_threshold and, if fewer than
    pre_matching_feature_threshold features survive, a second at fast_threshold / 4 with the survivors as existing tracks (the
    bucket score keeps using fast_threshold).  existing: the feature set the frame starts from as (xy, ages, strengths); None is
    the empty set.  cfg: any object with the configuration's field names."""
    grid = (cfg.buckets_along_height, cfg.buckets_along_width, cfg.bucket_start_row, cfg.features_per_bucket,
            cfg.age_threshold, cfg.fast_threshold)
    none = np.zeros(0, np.int32)
    existing = (np.zeros((0, 2), np.float32), none, none) if existing is None else existing
    out = append_features(img, cfg.fast_threshold, existing[0], existing[1], existing[2], *grid)
    second = len(out[1]) < cfg.pre_matching_feature_threshold
    if second:
        out = append_features(img, _cdiv(cfg.fast_threshold, 4), out[0], out[1], out[2], *grid)
    return out[0], out[1], out[2], second


# ---------------------------------------------------------------------------- fixture images
SIZES = [(7, 7), (7, 64), (8, 9), (19, 67), (20, 68), (35, 131), (36, 132), (37, 133), (40, 200)]     # (h, w)
FAMILIES = ("rand", "sat", "blk")
THRESHOLDS = [-3, 0, 1, 5, 20, 127, 128, 253, 254, 255, 300]
SEAM_SHAPE = (40, 136)
_SEED = 1


def noise(rng, h, w):
    return rng.integers(0, 256, (h, w)).astype(np.uint8)


def saturated(rng, h, w):
    return rng.choice(np.array([0, 1, 254, 255], np.uint8), size=(h, w), p=[.45, .05, .05, .45])


def blocks(rng, h, w):
    """2x2 block-replicated noise: plateaus of equal score"""
    return np.repeat(np.repeat(noise(rng, (h + 1) // 2, (w + 1) // 2), 2, 0), 2, 1)[:h, :w].copy()


def seam_image(rng=None):
    """40x136: columns 64..127 mirror columns 63..0 and rows 16..31 mirror rows 15..0, the rest is noise.  The circle is
    mirror-symmetric, so raw scores are equal across columns 63|64 and rows 15|16 — the seams of a 64x16 tile grid."""
    rng = rng if rng is not None else np.random.default_rng([_SEED, 99])
    img = noise(rng, *SEAM_SHAPE)
    img[:, 64:128] = img[:, 63::-1]
    img[16:32, :] = img[15::-1, :]
    return img


def cases():
    """[(name, image)]: every family at every size, then the seam image.  Seeded, the same on every call."""
    make = dict(rand=noise, sat=saturated, blk=blocks)
    out = []
    for fi, fam in enumerate(FAMILIES):
        for h, w in SIZES:
            out.append(("%s%dx%d" % (fam, h, w), make[fam](np.random.default_rng([_SEED, fi, h, w]), h, w)))
    out.append(("seam", seam_image()))
    return out


_cache = {}


def case_image(name):
    if "images" not in _cache:
        _cache["images"] = dict(cases())
        for a in _cache["images"].values():
            a.setflags(write=False)
    return _cache["images"][name]


def case_scores(name, th, nonmax=True):
    """fast_scores of a fixture image, computed once per process and shared read-only between the tests"""
    key = (name, clamp_threshold(th), bool(nonmax))
    if key not in _cache:
        _cache[key] = fast_scores(case_image(name), th, nonmax)
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


def case_names():
    return [n for n, _ in cases()]


# the issue's negative-coordinate inputs (image 64x32, grid 4x8, start row 0, capacity 1: the filter keeps (-0.5, 3))
NEGATIVE_TRACKS = [(-0.5, 3.0), (5.0, -0.25), (-8.0, 3.0), (2.0, 2.0)]


def track_fixture(w, h, bah, baw, seed, n=400, age_thr=20):
    """Existing tracks that sit where the bucket index can go wrong -> (xy f32, ages i32, strengths i32), shuffled:
    random points (a third on whole pixels), bucket edges and the last f32 below them, w - 1 and h - 1, coordinates in
    (-bucket, 0), at and below -bucket, -0.0, beyond the grid; ages up to and above age_thr; strengths 0..255 (below the FAST
    threshold truncation and floor differ); runs of equal scores inside one bucket."""
    rng = np.random.default_rng([seed, w, h, bah, baw])
    bh, bw = -(-h // bah), -(-w // baw)
    f = np.float32
    xy = np.stack([rng.uniform(0, w - 0.01, n), rng.uniform(0, h - 0.01, n)], 1).astype(f)
    xy[::3] = np.floor(xy[::3])
    rx = lambda: f(rng.uniform(0, w - 0.01))
    ry = lambda: f(rng.uniform(0, h - 0.01))
    sp = [(w - 1, h - 1), (w - 1, 0), (0, h - 1), (0, 0)]
    for _ in range(12):
        ex, ey = f(bw * rng.integers(1, baw + 1)), f(bh * rng.integers(1, bah + 1))
        sp += [(ex, ry()), (np.nextafter(ex, f(0)), ry()), (rx(), ey), (rx(), np.nextafter(ey, f(0))), (ex, ey)]
    for _ in range(4):
        sp += [(-0.5, ry()), (-bw + 0.25, ry()), (rx(), -0.25), (rx(), -bh + 0.25),               # in (-bucket, 0)
               (-bw, ry()), (-bw - 3.5, ry()), (rx(), -bh), (rx(), -bh - 3.5),                    # at and below -bucket
               (-0.0, ry()), (rx(), -0.0), (-0.0, -0.0),
               (baw * bw, ry()), (baw * bw + 7.5, ry()), (rx(), bah * bh), (rx(), bah * bh + 7.5)]   # beyond the grid
    sp += NEGATIVE_TRACKS
    cx, cy = f(bw * (baw // 2) + 0.5 * bw), f(bh * (bah - 1) + 0.5 * bh)                          # one bucket of the last row
    run = [(cx, cy)] * 60
    xy = np.concatenate([xy, np.array(sp, f), np.array(run, f)])
    m = len(xy)
    ages = rng.integers(0, age_thr + 5, m).astype(np.int32)
    st = rng.integers(0, 256, m).astype(np.int32)
    ages[-60:] = np.repeat(rng.integers(0, 3, 6), 10)                # equal (age, strength) ten at a time ...
    st[-60:] = np.repeat(rng.integers(0, 256, 6), 10)
    st[-60::2] += rng.integers(0, 3, 30).astype(np.int32)            # ... or equal score at different strengths
    ages[m - 60 - len(NEGATIVE_TRACKS):m - 60] = 0
    st[m - 60 - len(NEGATIVE_TRACKS):m - 60] = 40
    order = rng.permutation(m)
    return xy[order].copy(), ages[order].copy(), np.clip(st[order], 0, 255).astype(np.int32)
