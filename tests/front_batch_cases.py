"""The case matrix of tests/test_gpu_front_batch.py and what builds its frames: the many-sequence front at batch speed (k_fast_batch,
k_deriv_levels, k_pad_pyramid; svo_kernels_img.hip).  tests/test_front_batch_cases.py guards on the CPU that the matrix holds the
sizes the kernels' tiles make special.

The tile constants, restated:
- FAST_TW x FAST_TH: the tile of k_fast_batch (level 0), staged with a 4-pixel halo; a block has FAST_THREADS threads.
- PLANE_V: consecutive samples of a row a thread of k_deriv_levels owns (one 16-byte store per plane); its vectors start at
  x = PLANE_V k - (pad & 7), so a row holds ceil((w + (pad & 7)) / PLANE_V) of them; PLANE_ROWS: rows a thread walks down.

A case is ((w, h), win, max_level, n_seq, streams): a grey context of 9 .. 12 sequences in the exact-sums mode, host frames, three
frames; sequence i replays stream i % len(streams).  Stream kinds:
- scene:  a rendered stereo scene (synthetic.StereoSequence): tracks, poses, inliers
- dots:   isolated bright pixels of random heights on a quiet background, forced onto the three-pixel image margin (both sides of
          it) and onto both sides of every tile seam, and neighbours across a seam that NMS must decide between
- dense:  full-range noise: one FAST tile queues more candidates than its block has threads
- black:  a black first frame in front of a scene: the frame after it finds no features and needs the second detection pass"""
import numpy as np

import pyramid_ref

FAST_TW, FAST_TH, FAST_THREADS = 64, 32, 256
PLANE_V, PLANE_ROWS = 8, 8
N_FRAMES = 3


def lk_pad_for(win):
    """The border the library stores around every level (svo_kernels_lk.hip lk_pad_for)."""
    ppl = next(p for p in range(1, win + 1) if win * -(-win // p) <= 64)
    return (-(-win // ppl) * ppl + 5 + 3) & ~3


CASES = [
    ((385, 161), 10, 3, 9, ("scene", "dots")),       # k T + 1 both ways; levels 193x81 97x41 49x21
    ((384, 160), 21, 2, 10, ("scene", "black")),     # k T; levels 192x80 96x40 (pad 28: the vectors start at x = -4)
    ((383, 159), 15, 3, 9, ("dense", "scene")),      # k T - 1; levels 192x80 96x40 48x20 (pad 24)
    ((129, 97), 5, 5, 12, ("dots", "dense")),        # levels 65x49 33x25 17x13 9x7: one shorter than PLANE_ROWS, narrower than the pad
    ((100, 207), 5, 5, 9, ("dense", "dots")),        # levels 50x104 25x52 13x26 7x13: one narrower than a vector
    ((255, 64), 7, 4, 11, ("dots", "black")),        # levels 128x32 64x16 32x8
    ((243, 95), 10, 2, 9, ("scene", "dense")),       # levels 122x48 61x24
    ((118, 110), 7, 3, 9, ("dots", "scene")),        # levels 59x55 30x28 15x14
    ((142, 78), 5, 4, 10, ("black", "dots")),        # levels 71x39 36x20 18x10 9x5 -> stops at 18x10
]


def case_id(c):
    (w, h), win, ml, B, kinds = c
    return "%dx%d-w%d-l%d-B%d-%s" % (w, h, win, ml, B, "+".join(kinds))


def levels_of(case):
    (w, h), win, ml, B, kinds = case
    return pyramid_ref.level_sizes(w, h, win, ml)


# ------------------------------------------------------------------------------------------------------------------ frames
def special_columns(n, tile):
    """Both sides of the three-pixel margin and of every tile seam of an axis of n pixels."""
    xs = {2, 3, n - 4, n - 3}
    for s in range(tile, n, tile):
        xs |= {s - 1, s}
    return sorted(x for x in xs if 0 <= x < n)


def dots_image(w, h, seed):
    rng = np.random.default_rng(seed)
    img = (100 + rng.integers(-4, 5, (h, w))).astype(np.uint8)
    xs, ys = special_columns(w, FAST_TW), special_columns(h, FAST_TH)
    for y in ys:                                                     # along every special row and column, every 7th pixel
        for x in range(3 + (y % 5), w - 3, 7):
            img[y, x] = rng.integers(160, 256)
    for x in xs:
        for y in range(3 + (x % 5), h - 3, 7):
            img[y, x] = rng.integers(160, 256)
    for y in ys:                                                     # the crossings themselves, and a diagonal neighbour across the seam
        for x in xs:
            img[y, x] = rng.integers(160, 256)
            if y + 1 < h and x + 1 < w:
                img[y + 1, x + 1] = rng.integers(160, 256)
    n = max(8, w * h // 60)
    img[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.integers(150, 256, n)
    return img


def shifted_pairs(base, w, h, n):
    """n stereo pairs cut from a wider image: the right view is the left one shifted, the next frame moves a little."""
    L = [np.ascontiguousarray(base[k:k + h, 2 * k:2 * k + w]) for k in range(n)]
    R = [np.ascontiguousarray(base[k:k + h, 2 * k + 6:2 * k + 6 + w]) for k in range(n)]
    return L, R


def scene(w, h, n, seed):
    from stereo_visual_odometry_amd import synthetic as syn
    s = syn.StereoSequence(cal=calib(w, h), n_frames=n, seed=seed, step=0.3)
    return list(s.left)[:n], list(s.right)[:n]


def calib(w, h):
    from stereo_visual_odometry_amd import synthetic as syn
    return dict(syn.KITTI00, width=w, height=h, cx=w / 2.0, cy=h / 2.0)


def stream(kind, w, h, seed, n=N_FRAMES):
    """(lefts, rights) of one stream of n frames."""
    if kind == "scene":
        return scene(w, h, n, seed)
    if kind == "black":
        L, R = scene(w, h, n - 1, seed)
        z = np.zeros((h, w), np.uint8)
        return [z] + L, [z.copy()] + R
    if kind == "dots":                                               # the first frame IS the dots image: its margins and seams are the image's
        L, R = shifted_pairs(np.pad(dots_image(w, h, seed), ((0, n), (0, 2 * n + 6)), mode="reflect"), w, h, n)
        return L, R
    if kind == "dense":
        rng = np.random.default_rng(seed)
        return shifted_pairs(rng.integers(0, 256, (h + n, w + 2 * n + 6)).astype(np.uint8), w, h, n)
    raise ValueError(kind)


def screen_count_max(img, th=20):
    """The largest number of pixels FAST's screening test queues in one tile of k_fast_batch: the tile with its one-pixel ring, the
    pixels at least 3 from the image edge, a darker (or a brighter) member in each of the circle's pairs (0, 8) and (4, 12)."""
    a = np.asarray(img, np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    up, dn, lf, rt = a[0:h - 6, 3:w - 3], a[6:h, 3:w - 3], a[3:h - 3, 0:w - 6], a[3:h - 3, 6:w]
    dark = ((dn < v - th) | (up < v - th)) & ((rt < v - th) | (lf < v - th))
    bright = ((dn > v + th) | (up > v + th)) & ((rt > v + th) | (lf > v + th))
    p = np.zeros((h, w), bool)
    p[3:h - 3, 3:w - 3] = dark | bright
    best = 0
    for y0 in range(0, h, FAST_TH):
        for x0 in range(0, w, FAST_TW):
            best = max(best, int(p[max(y0 - 1, 0):y0 + FAST_TH + 1, max(x0 - 1, 0):x0 + FAST_TW + 1].sum()))
    return best
