"""The LK kernel's minimum-eigenvalue test at its decision boundary, bit for bit against the CPU oracle.

The kernel screens "minEig < threshold" with the hardware's approximate square root and only evaluates the exact IEEE expression when
the approximate numerator lies within a band of the cut-off (or the radicand is too small for the bare instruction).  Smooth scenes at
the default threshold never come near the cut-off, so nothing else in the suite runs the band's exact path or could tell a band that
is too narrow.  Here the threshold itself is moved onto the features: for a dozen points of each scene the oracle is bisected over the
doubles for the `optical_flow_min_eig_threshold` at which the point's status flips, and the kernel then runs at that double, at its
predecessor, and at the float32 neighbours up to three steps to either side — the chosen point sits inside the band (its exact
numerator equals the cut-off or misses it by a few ulp), the other points of the call take the screened decision.  Statuses and
points of all ~60 points must equal the oracle's at every threshold.

Scenes (112 x 96, so that w = 21 has three levels: 112 x 96, 56 x 48, 28 x 24):
    texture   band-limited noise, shifted by one pixel with +-2 grey levels of noise
    flat      a constant image with isolated single-pixel bumps.  A window centred on a bump has A11 == A22 and A12 == 0 by symmetry:
              radicand exactly 0 under a positive trace (asserted below from the oracle's derivative image); a window without a bump
              has A == 0.  Both take the small-radicand exit of the screen.
    ramp      one gradient: I = 2 x plus a faint row pattern, so A is rank one up to that pattern and the root equals the trace to within
              less than one per cent — the numerator is the difference of two nearly equal floats."""
import numpy as np
import pytest

import oracle_lib as orc
import scenes
from gpu_kit import api, f32_bits as bits  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

W_IMG, H_IMG, WIN = 112, 96, 21
N_POINTS, N_FLIPS = 60, 12
FIXED = [0.0, 1e-3, 1e-12, -1.0, 1e30]           # besides the flips: the default, "everything passes", "everything fails"


def bump_centres():
    return [(30 + 26 * i, 28 + 40 * j) for i in range(3) for j in range(2)]


def make_scene(name):
    """-> (a, b, points): the first N_FLIPS points are the candidates whose flips are looked for"""
    rng = np.random.default_rng(77)
    if name == "texture":
        a = scenes.random_texture(H_IMG, W_IMG, 31, smooth=2)
        b = np.clip(scenes.shift_image(a, 1, 0).astype(np.int32) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)
        first = np.stack([rng.uniform(8, W_IMG - 8, N_FLIPS), rng.uniform(8, H_IMG - 8, N_FLIPS)], 1)
    elif name == "flat":
        a = np.full((H_IMG, W_IMG), 100, np.uint8)
        for x, y in bump_centres():
            a[y, x] = 180
        b = a.copy()
        first = np.array(bump_centres() + [(31, 28), (56.5, 68.25), (80, 50), (4, 4), (82.5, 27.5), (57, 69)], np.float64)
    else:
        x = np.arange(W_IMG)[None, :]
        y = np.arange(H_IMG)[:, None]
        a = (2 * x + (y % 7 == 0) * ((x // 3) % 2)).astype(np.uint8)
        b = scenes.shift_image(a, 1, 0)
        first = np.stack([rng.uniform(12, W_IMG - 12, N_FLIPS), rng.uniform(12, H_IMG - 12, N_FLIPS)], 1)
    rest = np.stack([rng.uniform(-3, W_IMG + 3, N_POINTS - len(first)), rng.uniform(-3, H_IMG + 3, N_POINTS - len(first))], 1)
    rest[:6] = np.floor(rest[:6])
    return a, b, np.concatenate([first, rest]).astype(np.float32)


def f64_from_key(k):
    return float(np.array([k], np.uint64).view(np.float64)[0])


def flip_threshold(pa, pb, pt, lv):
    """Bisection over the non-negative doubles (their bit patterns are ordered as they are): -> (last threshold at which the point's
    status is 1, the next double, at which it is 0), or None if the status is the same at 0 and at 1e9."""
    def st(t):
        return int(orc.lk_track(pa, pb, pt[None], (WIN, WIN), lv, min_eig=t)[1][0])
    lo, hi = 0, int(np.array([1e9], np.float64).view(np.uint64)[0])
    if st(0.0) != 1 or st(1e9) != 0:
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if st(f64_from_key(mid)) == 1:
            lo = mid
        else:
            hi = mid
    return f64_from_key(lo), f64_from_key(hi)


def thresholds_around(lo, hi):
    out = [lo, hi]
    for start in (np.float32(hi), np.float32(lo)):
        up = down = start
        out.append(float(start))
        for _ in range(3):
            up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
            out += [float(up), float(down)]
    return sorted(set(out))


_CASES = {}


def case(name, lv):
    """(a, b, points, pyramids, thresholds, number of flips found) of a scene at a max_level, built once"""
    key = (name, lv)
    if key not in _CASES:
        a, b, pts = make_scene(name)
        pa, pb = orc.Pyramid(a, (WIN, WIN), lv), orc.Pyramid(b, (WIN, WIN), lv)
        assert pa.nlevels == lv + 1
        thr, flips = list(FIXED), 0
        for i in range(N_FLIPS):
            f = flip_threshold(pa, pb, pts[i], lv)
            if f is not None:
                flips += 1
                thr += thresholds_around(*f)
        _CASES[key] = (a, b, pts, pa, pb, sorted(set(thr)), flips)
    return _CASES[key]


MIN_FLIPS = {"texture": 10, "flat": 3, "ramp": 1}


@pytest.mark.parametrize("lv", [0, 2])
@pytest.mark.parametrize("name", ["texture", "flat", "ramp"])
def test_single_pass_stage_call(api, name, lv):
    a, b, pts, pa, pb, thr, flips = case(name, lv)
    print("%s max_level %d: %d flips, %d thresholds" % (name, lv, flips, len(thr)))
    assert flips >= MIN_FLIPS[name], flips
    took = np.zeros((2, N_FLIPS), bool)                         # [status][candidate]: the status was seen at some threshold
    for t in thr:
        got, gst = api.calcOpticalFlowPyrLK(a, b, pts, WIN, lv, min_eig_threshold=t)
        want, wst = orc.lk_track(pa, pb, pts, (WIN, WIN), lv, min_eig=t)
        assert np.array_equal(gst, wst), (t.hex(), np.flatnonzero(gst != wst))
        assert np.array_equal(bits(got), bits(want)), (t.hex(), np.flatnonzero((bits(got) != bits(want)).any(1)))
        took[0] |= wst[:N_FLIPS] == 0
        took[1] |= wst[:N_FLIPS] == 1
    assert (took[0] & took[1]).sum() >= flips, (took, flips)     # the thresholds really move every candidate that has a flip


@pytest.mark.parametrize("lv", [0, 2])
@pytest.mark.parametrize("name", ["texture", "flat", "ramp"])
def test_fused_circular_match(api, name, lv):
    """The same thresholds through k_lk_chain: pass L0 -> L1 is the pair the flips were found on"""
    a, b, pts, _, _, thr, _ = case(name, lv)
    c, d = scenes.shift_image(a, 0, 1), scenes.shift_image(b, 0, 1)
    P = [orc.Pyramid(i, (WIN, WIN), lv) for i in (a, c, b, d)]
    for t in thr:
        over = dict(win_w=WIN, win_h=WIN, max_level=lv, optical_flow_min_eig_threshold=t)
        res = api.circularMatching(api.default_config(**over), a, c, b, d, pts)
        ref = orc.circular_match(P[0], P[1], P[2], P[3], pts, orc.default_config(**over))
        assert np.array_equal(res[4], ref[4]), (t.hex(), np.flatnonzero(res[4] != ref[4]))
        for k, (g, o) in enumerate(zip(res[:4], ref[:4])):
            assert np.array_equal(bits(g), bits(o)), (t.hex(), k, np.flatnonzero((bits(g) != bits(o)).any(1)))


def window_sums(p, x, y):
    """A11, A12, A22 (exact integers) of the window centred on the integer point (x, y) at level 0: its origin is an integer, so the
    bilinear weights are (1, 0, 0, 0) and the window's derivatives are the derivative image's"""
    h = (WIN - 1) // 2
    d = p.deriv(0).astype(np.int64)[y - h:y + h + 1, x - h:x + h + 1]
    return int((d[..., 0] ** 2).sum()), int((d[..., 0] * d[..., 1]).sum()), int((d[..., 1] ** 2).sum())


def test_scenes_are_what_they_claim():
    """No GPU needed for the claim, but the module is a GPU module: the symmetric bump has radicand 0 under a positive trace, an empty
    window has A == 0, and the ramp's A is rank one up to its faint row pattern"""
    a, _, _ = make_scene("flat")
    p = orc.Pyramid(a, (WIN, WIN), 0)
    for x, y in bump_centres():
        a11, a12, a22 = window_sums(p, x, y)
        assert a11 == a22 > 0 and a12 == 0, (x, y, a11, a12, a22)
    assert window_sums(p, 56, 48) == (0, 0, 0)
    a, _, _ = make_scene("ramp")
    p = orc.Pyramid(a, (WIN, WIN), 0)
    a11, a12, a22 = window_sums(p, 56, 48)
    assert 0 < a22 < a11 / 100, (a11, a12, a22)
