"""The inputs of tests/test_gpu_lk_limits.py do what that file relies on, shown on the CPU oracle alone (tests/lk_limits_scenes.py has
the argument): every proof point's window totals 2^31 or more in sum Ix^2 or sum Iy^2, so no int32 reduction can have summed it; at
least half the points do the same in the first step's mismatch sums; and the oracle still tracks the case.  The per-case shares are
printed (pytest -s) and recorded as user properties.

Measured here on binary(120, 160, 2, seed 5), 150 points, max_level = 0, b = shift_image(a, 1, 0):
    w    PRE  wide in A  wide in b  tracked    worst error of a tracked point from the true shift
    21   3    100 %      100 %      150 / 150  1.2e-3 px
    31   2    100 %      100 %      150 / 150  6.4e-4 px
other shifts at w = 21: (1, 1) 27 % wide in b, (2, 1) 0 % — which is why the cases shift by (1, 0).
Stripes (seed 2), shift (1, 0):  w = 15 and w = 16 (PRE = 4): 100 % wide in A (smallest total 1.25 and 1.38 x 2^31), 100 % wide in b,
150 / 150 tracked within 4e-3 px.
BGR from three binary planes (seeds 5, 6, 7): w = 21 (PRE = 1) and w = 15 (PRE = 2): 100 % / 100 %.  BGR kernels exist up to w = 21 only
(a lane of a wider window would hold three planes of eleven or more pixels), so there is no BGR case at w = 31.
"""
import numpy as np
import pytest

import oracle_lib as orc
import lk_limits_scenes as lim

F32 = np.float32

# name -> (case, PRE the kernel compiles for it, true shift, whether at least half the points must be provably wide in b)
CASES = {
    "binary_w21": (lambda: lim.grey_binary(21), 3, (1, 0), True),
    "binary_w31": (lambda: lim.grey_binary(31), 2, (1, 0), True),
    "negative_w21": (lambda: lim.grey_negative(21), 3, (-1, 0), True),
    "negative_w31": (lambda: lim.grey_negative(31), 2, (-1, 0), True),
    "stripes_w15": (lambda: lim.grey_stripes(15), 4, (1, 0), False),
    "stripes_w16": (lambda: lim.grey_stripes(16), 4, (1, 0), False),
    "bgr_w21": (lambda: lim.bgr_binary(21), 1, (1, 0), True),
    "bgr_w15": (lambda: lim.bgr_binary(15), 2, (1, 0), True),
}


def oracle_track_cn(case, max_level=0, max_count=30):
    """orc.lk_track for grey; for BGR the oracle's multi-plane entry through the same binding"""
    import ctypes as C
    win = case.win
    pa = [orc.Pyramid(p, (win, win), max_level) for p in case.planes_a]
    pb = [orc.Pyramid(p, (win, win), max_level) for p in case.planes_b]
    if case.cn == 1:
        return orc.lk_track(pa[0], pb[0], case.pts, (win, win), max_level, max_count=max_count)
    n = len(case.pts)
    out = np.zeros((n, 2), np.float32); st = np.zeros(n, np.uint8)
    A = (C.c_void_p * case.cn)(*[C.addressof(p.p) for p in pa]); B = (C.c_void_p * case.cn)(*[C.addressof(p.p) for p in pb])
    cfg = orc.default_config()
    orc.lib().orc_lk_track_cn(case.cn, A, B, n, orc._p(case.pts), orc._p(out), orc._p(st), win, win, max_level, max_count,
                              C.c_double(cfg.lk_epsilon), C.c_double(cfg.optical_flow_min_eig_threshold))
    return out, st


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_provably_wide_and_tracked(name, record_property):
    make, pre, shift, need_b = CASES[name]
    case = make()
    assert (case.h, case.w, len(case.pts)) == (lim.H, lim.W_IMG, lim.N_POINTS)
    assert lim.presplit_steps(case.win, case.cn) == pre
    s = lim.first_step_sums(case)
    wa, wb = lim.provably_wide_A(case), lim.provably_wide_b(case)
    nxt, st = oracle_track_cn(case)
    err = np.abs(nxt - case.pts - np.array(shift, np.float32)).max(1)
    worst = float(err[st > 0].max())
    small = float(np.maximum(s["A11"], s["A22"]).min()) / lim.TWO31
    print("%-13s PRE %d  wide in A %5.1f %%  wide in b %5.1f %%  tracked %d / %d  worst error %.1e px  smallest max(A11, A22) %.3f x 2^31"
          % (name, pre, 100 * wa.mean(), 100 * wb.mean(), int(st.sum()), len(st), worst, small))
    record_property("wide_A_share", float(wa.mean())); record_property("wide_b_share", float(wb.mean())); record_property("tracked", int(st.sum()))
    assert wa.all(), "a proof point's A sums fit an int32 reduction"
    if need_b:
        assert wb.mean() >= 0.5
    assert st.sum() >= 140
    assert worst < 0.01                                     # the oracle finds the true shift: the case is a track, not noise


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_sums_are_the_oracles(name):
    """The int64 sums the proof is made of are the ones the oracle accumulates: its result after ONE Newton step, rebuilt from them
    in f32 by the formulas of lk_level (oracle/orc_lk.c), must be the oracle's bits for every point."""
    case = CASES[name][0]()
    s = lim.first_step_sums(case)
    nxt, st = oracle_track_cn(case, max_count=1)
    assert st.all()
    sc = F32(1.0) / F32(1 << 20)
    f = {k: v.astype(np.float64).astype(np.float32) * sc for k, v in s.items()}
    D = f["A11"] * f["A22"] - f["A12"] * f["A12"]
    D = F32(1.0) / D
    dx = (f["A12"] * f["b2"] - f["A22"] * f["b1"]) * D
    dy = (f["A12"] * f["b1"] - f["A11"] * f["b2"]) * D
    half = F32((case.win - 1) * 0.5)
    org = case.origins().astype(np.float32)
    want = np.stack([(org[:, 0] + dx) + half, (org[:, 1] + dy) + half], 1).astype(np.float32)
    assert np.array_equal(want.view(np.uint32), nxt.view(np.uint32))


def test_identical_images_have_zero_mismatch():
    for win in (21, 31):
        case = lim.grey_identical(win)
        s = lim.first_step_sums(case)
        assert lim.provably_wide_A(case).all() and not s["b1"].any() and not s["b2"].any()
        nxt, st = lim.oracle_track(case)
        assert st.all() and np.array_equal(nxt.view(np.uint32), case.pts.view(np.uint32))


def test_signs_of_the_extremes():
    """binary + shift (1, 0) drives b1 to -2^31 and below, the complement shifted the other way to +2^31 and above; A12 has both signs"""
    for win in (21, 31):
        neg, pos = lim.first_step_sums(lim.grey_binary(win)), lim.first_step_sums(lim.grey_negative(win))
        assert (neg["b1"] <= -lim.TWO31).all() and (pos["b1"] >= lim.TWO31).all()
        assert (neg["A12"] < 0).any() and (neg["A12"] > 0).any()


def test_windows_that_cannot_reach_the_bound():
    """w <= 10: at most two pixels per lane, 2 * 4080^2 < 2^25 — no wide form to test; w = 11: the total stays below 2^31, nothing
    can be proven; w = 12 .. 16 are PRE = 4 and need stripes: random 2 x 2 blocks stay below 2^31 there"""
    assert all(lim.lk_layout(win)[0] * 4080 * 4080 < (1 << 25) for win in range(5, 11))
    assert 11 * 11 * 4080 * 4080 < lim.TWO31 <= 12 * 12 * 4080 * 4080
    assert [lim.presplit_steps(w, 1) for w in (12, 15, 16, 21, 31)] == [4, 4, 4, 3, 2]
    assert [lim.presplit_steps(w, 3) for w in (15, 21)] == [2, 1]
    c = lim.Case("blocks_w15", [lim.binary(**lim.BIN)], [lim.binary(**lim.BIN)], 15)
    assert not lim.provably_wide_A(c).any()


def test_pipeline_frames_carry_large_coarse_derivatives():
    """The binarised synthetic stream of the frame-pipeline tests: level 1 of a fed frame holds a Scharr value of 3500 or more (the
    derivative planes store four times that), and the oracle tracks more than 20 features into LK."""
    import lk_limits_child as lch
    fr = lch.frames()
    d1 = max(int(np.abs(orc.Pyramid(L, (21, 21), 3).deriv(1)).max()) for s in fr for L, _ in s)
    assert d1 >= 3500, d1
    assert all(set(np.unique(L)) == {0, 255} for s in fr for L, _ in s)
    want = lch.oracle_frames()
    into = [int(r["stats"][lch.STAT_NAMES.index("n_into_lk")]) for s in want for r in s]
    after = [int(r["stats"][lch.STAT_NAMES.index("n_after_circular")]) for s in want for r in s]
    print("level-1 |Scharr| max %d, n_into_lk %s, n_after_circular %s" % (d1, into, after))
    assert max(into) > 20 and max(after) > 10
