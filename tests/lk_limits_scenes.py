"""Maximum-contrast inputs for the LK kernel's wide-sum paths, and the proof — from the oracle's own derivative images, in int64
numpy — that a case must take them.  Nothing here reads the kernel.

The kernel sums the 2x2 normal matrix A and the mismatch vector b of a window over the 64 lanes of a wave.  A lane whose partial
of sum Ix^2 or sum Iy^2 (or |partial| of a mismatch sum) reaches 2^25 sends the wave to the "wide" reduction, which splits every
partial into 16-bit halves after PRE doublings; otherwise the reduction stays in int32 ("narrow").  The proofs below rest on the
pigeonhole argument alone: 64 lanes each below 2^25 cannot sum to 2^31, so a window total at or above 2^31 cannot have been summed
by the narrow form — and whatever threshold the kernel uses, an int32 cannot hold such a total, so a kernel that took the narrow
form anyway cannot return the oracle's bits.  (With the lane threshold at 2^27 instead of 2^25, every lane of a w = 21 window —
seven pixels, at most 7 * 4080^2 = 1.17e8 < 2^27 — would pass as narrow; every w = 21 case below totals 2^31 or more and would
overflow.  The proof does not lean on the threshold it tests.)

Points.  Every case places N_POINTS points whose window origin pt - (w - 1) / 2 is an integer (k + 0.5 coordinates for even w) and
whose window, with the one extra row and column of the bilinear stencil, lies inside the image.  At max_level = 0 the template is
then sampled with weights (2^14, 0, 0, 0) and the first Newton step starts from the same origin, so with Ix, Iy = Pyramid.deriv(0)
of the first image, exactly:
    A11 = sum Ix^2, A22 = sum Iy^2, A12 = sum Ix Iy            (the oracle's iA11 .. at level 0)
    b1 = sum 32 (J - I) Ix, b2 = sum 32 (J - I) Iy              (its ib1, ib2 of step 0)
over the w x w window and, for three channels, over the channels: the kernel's per-lane partial spans the channels (CN_fold).

Windows.  Scharr of u8 is at most 4080 in magnitude.
  w <= 10      one lane holds one or two pixels: 2 * 4080^2 = 3.3e7 < 2^25.  No lane can reach the bound, the wide form is
               unreachable, there is nothing to test.
  w = 11       three pixels per lane can reach 2^25 (3 * 4080^2 = 5.0e7), so the wide form can run, but the window total stays below
               121 * 4080^2 < 2^31: both forms are exact there and no total can prove which one ran.  Not a case.
  w = 12 .. 16 (PRE = 4 grey: three or four pixels per lane).  Random blocks cannot reach 2^31 (w = 15 tops out at 0.94 * 2^31), but
               vertical stripes two pixels wide have |Ix| = 4080 in every column: sum Ix^2 = w^2 * 4080^2 >= 2^31 from w = 12 on.
               `stripes` breaks them with sparse row bands of opposite polarity so that sum Iy^2 > 0 and the min-eigenvalue test passes.
  w = 17 .. 21 (PRE = 3 grey, PRE = 1 BGR), w = 22 .. 31 (PRE = 2 grey; BGR is not built above 21): random 2 x 2 blocks of 0 / 255.
  BGR w = 12 .. 16 is PRE = 2 (nine to twelve pixel-channels per lane).
"""
import numpy as np

import oracle_lib as orc
import scenes

H, W_IMG, N_POINTS = 120, 160, 150
TWO31 = 1 << 31


def binary(h, w, blk, seed):
    """random blocks of blk x blk pixels, each 0 or 255"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, ((h + blk - 1) // blk, (w + blk - 1) // blk)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(cells, np.ones((blk, blk), np.uint8))[:h, :w])


def stripes(h, w, seed, band=(4, 9)):
    """vertical stripes two pixels wide (|Ix| = 4080 in every column); row bands of random height band[0] .. band[1] - 1 alternate
    the polarity, which gives the rows at a band's edge a vertical derivative (|Iy| = 2550) at the cost of |Ix| = 2550 there"""
    rng = np.random.default_rng(seed)
    col = ((np.arange(w) // 2) % 2).astype(np.uint8)
    pol = np.zeros(h, np.uint8)
    y, p = 0, 0
    while y < h:
        n = int(rng.integers(band[0], band[1]))
        pol[y:y + n] = p
        y += n; p ^= 1
    return np.ascontiguousarray((col[None, :] ^ pol[:, None]) * np.uint8(255))


def lk_layout(win):
    """(PPL, LPR) of the kernel's LkLayout<win>: PPL = smallest p with win * ceil(win / p) <= 64"""
    for p in range(1, win + 1):
        if win * ((win + p - 1) // p) <= 64:
            return p, (win + p - 1) // p
    return win, 1


def presplit_steps(win, cn):
    """PRE of the kernel (lk_presplit_steps(PPL * CN)): doublings a lane's largest partial survives in int32, at most 4"""
    m, k = lk_layout(win)[0] * cn * 8160 * 4080, 0
    while k < 4 and m * 2 <= 2147483647:
        m *= 2; k += 1
    return k


def window_points(h, w, win, n, seed):
    """n points with an integer window origin, window and bilinear stencil inside the image: origin in [1, size - win - 2]"""
    rng = np.random.default_rng(seed)
    ox = rng.integers(1, w - win - 1, n)
    oy = rng.integers(1, h - win - 1, n)
    return (np.stack([ox, oy], 1) + (win - 1) / 2.0).astype(np.float32)


class Case:
    """planes_a, planes_b: lists of (h, w) u8 planes (one for grey, three for BGR); pts: the N_POINTS proof points"""

    def __init__(self, name, planes_a, planes_b, win, seed=3, pts=None):
        self.name, self.win = name, win
        self.planes_a = [np.ascontiguousarray(p, np.uint8) for p in planes_a]
        self.planes_b = [np.ascontiguousarray(p, np.uint8) for p in planes_b]
        self.h, self.w = self.planes_a[0].shape
        self.cn = len(self.planes_a)
        self.pts = window_points(self.h, self.w, win, N_POINTS, seed) if pts is None else np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        self._sums = None

    @property
    def a(self):
        return self.planes_a[0] if self.cn == 1 else np.ascontiguousarray(np.stack(self.planes_a, -1))

    @property
    def b(self):
        return self.planes_b[0] if self.cn == 1 else np.ascontiguousarray(np.stack(self.planes_b, -1))

    def origins(self, pts=None):
        o = (self.pts if pts is None else np.asarray(pts)).astype(np.float64) - (self.win - 1) / 2.0
        assert np.array_equal(o, np.floor(o)), "a window origin is not an integer"
        assert (o >= 0).all() and (o[:, 0] + self.win < self.w).all() and (o[:, 1] + self.win < self.h).all(), "a window leaves the image"
        return o.astype(np.int64)

    def inside(self, pts):
        """which of pts have an integer window origin and the window with its bilinear stencil inside the image"""
        o = np.asarray(pts).astype(np.float64) - (self.win - 1) / 2.0
        return (o == np.floor(o)).all(1) & (o >= 0).all(1) & (o[:, 0] + self.win < self.w) & (o[:, 1] + self.win < self.h)


def _box(img, org, win):
    """sum of img over the win x win window at every origin (x, y), exact in int64"""
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    s[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    x, y = org[:, 0], org[:, 1]
    return s[y + win, x + win] - s[y, x + win] - s[y + win, x] + s[y, x]


def first_step_sums(case, pts=None):
    """per point (the case's own, or pts), summed over the channels, int64: dict A11, A12, A22 (level 0) and b1, b2 (first Newton
    step at max_level = 0)"""
    if pts is not None:
        return first_step_sums(Case(case.name, case.planes_a, case.planes_b, case.win, pts=pts))
    if case._sums is None:
        org = case.origins()
        out = {k: np.zeros(len(org), np.int64) for k in ("A11", "A12", "A22", "b1", "b2")}
        for pa, pb in zip(case.planes_a, case.planes_b):
            d = orc.Pyramid(pa, (case.win, case.win), 0).deriv(0).astype(np.int64)
            ix, iy = d[:, :, 0], d[:, :, 1]
            diff = 32 * (pb.astype(np.int64) - pa.astype(np.int64))
            for k, v in (("A11", ix * ix), ("A12", ix * iy), ("A22", iy * iy), ("b1", diff * ix), ("b2", diff * iy)):
                out[k] += _box(v, org, case.win)
        case._sums = out
    return case._sums


def provably_wide_A(case, pts=None):
    """per point: max(A11, A22) >= 2^31 over the channels — some lane's partial is then at or above 2^25"""
    s = first_step_sums(case, pts)
    return np.maximum(s["A11"], s["A22"]) >= TWO31


def provably_wide_b(case, pts=None):
    """per point: max(|b1|, |b2|) of the first step >= 2^31 over the channels"""
    s = first_step_sums(case, pts)
    return np.maximum(np.abs(s["b1"]), np.abs(s["b2"])) >= TWO31


def oracle_track(case, max_level=0, pts=None):
    """(next, status) of the oracle on the case's grey images"""
    assert case.cn == 1
    win = case.win
    pa, pb = orc.Pyramid(case.a, (win, win), max_level), orc.Pyramid(case.b, (win, win), max_level)
    return orc.lk_track(pa, pb, case.pts if pts is None else pts, (win, win), max_level)


# ---------------------------------------------------------------- the cases
BIN = dict(h=H, w=W_IMG, blk=2, seed=5)
STRIPE_WIN, STRIPE_SEED = 16, 2


def grey_binary(win, shift=(1, 0)):
    a = binary(**BIN)
    return Case("binary_w%d" % win, [a], [scenes.shift_image(a, *shift)], win)


def grey_identical(win):
    a = binary(**BIN)
    return Case("identical_w%d" % win, [a], [a], win)


def grey_negative(win):
    """the complement of the binary image, shifted the other way: the derivatives and the mismatch change sign against grey_binary"""
    a = 255 - binary(**BIN)
    return Case("negative_w%d" % win, [a], [scenes.shift_image(a, -1, 0)], win)


def grey_stripes(win=STRIPE_WIN):
    a = stripes(H, W_IMG, STRIPE_SEED)
    return Case("stripes_w%d" % win, [a], [scenes.shift_image(a, 1, 0)], win)


def bgr_binary(win, shift=(1, 0)):
    pl = [binary(H, W_IMG, 2, s) for s in (5, 6, 7)]
    return Case("bgr_w%d" % win, pl, [scenes.shift_image(p, *shift) for p in pl], win)


def binarised(frame):
    """a frame at its median: 0 / 255"""
    return np.ascontiguousarray((frame > np.median(frame)).astype(np.uint8) * 255)
