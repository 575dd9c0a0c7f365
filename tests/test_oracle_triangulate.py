"""The oracle's triangulation (orc_triangulate: DLT, orc_svd on the 4 x 4, f32 dehomogenisation) against an independent f64
reference (tests/triangulate_ref.py: numpy's LAPACK SVD) on the inputs circular matching really delivers: disparities of a few
thousandths of a pixel, zero and negative, with and without vertical mismatch, at and beyond the image corners and at the
principal point, next to ordinary points — about 900 track pairs per calibration.  The GPU suite holds the kernels to the oracle
bit for bit (test_gpu_triangulate_edges.py), so a mistake the two share — which singular vector, which dehomogenisation rule —
would pass there; here the oracle answers to something that shares nothing with it.

No tolerance here is tuned.  A correct SVD returns a unit vector v with ||A v|| = sigma_4; storing it in f32 moves each
component by at most 2^-24 relative, hence the residual by at most 2^-24 sigma_1, doubled for the renormalisation: the bound is
sigma_4 + 2^-23 sigma_1.  The vector of the NEXT singular value has residual sigma_3, orders of magnitude above that for most
of the fixture (asserted, so the test cannot go vacuous).

Regimes of the fixture (share of its 908 points; measured with the oracle, printed by test_regimes_of_the_fixture):
                     sigma_3 > 100 bound    not separated    |Wh| < 1e-6    Wh == 0
    kitti                  96.4 %               3.6 %           6.9 %          4
    run1                   88.2 %              11.8 %           2.4 %          4
    general                91.5 %               8.5 %           1.7 %          1
"Not separated" is no tie: sigma_3 / sigma_4 stays above 74 (kitti), 16 (run1), 34 (general) — with a baseline, a vertical
mismatch lifts sigma_4 but never to sigma_3.  Exact ties (sigma_3 = sigma_4 = 0) exist only without a baseline: 7 pairs of the
fourth calibration, which the GPU suite compares with the oracle bit for bit.
The Wh == 0 points are honest fixture points: left = right = the principal point (any dy for the rectified pairs).  The third
column of the DLT matrix is then zero (with a mismatch: orthogonal to columns 0 and 3), Jacobi never rotates it against the
fourth, and the null vector (0, 0, 1, 0) — (0, y, z, 0) with a mismatch — keeps an exact zero: the `else` branch of the
dehomogenisation rule needs no hand-made input.
"""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import triangulate_ref as ref

CALS = list(ref.WITH_BASELINE)


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything the tests of one calibration share, computed once and never written to."""
    Pl, Pr, f = ref.fixture(name)
    xyz, homog = orc.triangulate(Pl, Pr, f["pl"], f["pr"])
    A = ref.dlt_matrix(Pl, Pr, f["pl"], f["pr"])
    sv = ref.singular_values(A)
    out = dict(Pl=Pl, Pr=Pr, f=f, xyz=xyz, homog=homog, A=A, sv=sv, bound=ref.residual_bound(sv))
    for v in list(out.values()) + list(f.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_fixture_is_deterministic_and_exact():
    """Same bytes on every call; the disparities the construction names are the disparities of the f32 points, 2^-12 included."""
    for name in ref.calibrations():
        Pl, Pr, f = ref.fixture(name)
        _, _, g = ref.fixture(name)
        assert all(np.array_equal(f[k], g[k], equal_nan=True) for k in f)
        n = len(f["pl"])
        assert n == len(ref.DISPARITIES) * len(ref.MISMATCHES) * 7 + ref.N_RANDOM == 908
        grid = f["pos"] >= 0
        d32 = f["pl"][grid, 0].astype(np.float64) - f["pr"][grid, 0].astype(np.float64)
        assert np.array_equal(d32, f["d"][grid])
        assert set(np.abs(d32)) == {abs(d) for d in ref.DISPARITIES}
        pp = f["pos"] == 2
        assert np.array_equal(f["pl"][pp], np.tile(Pl.reshape(3, 4)[:2, 2], (pp.sum(), 1)))     # the principal point itself


def test_reference_dehomogenise_rule():
    h = np.array([[2, 4, 6, 2], [1, 2, 3, 0], [1, -2, 0, np.float32(1e-45)], [0, 1, 2, -0.0], [3, 0, 0, np.inf]], np.float32)
    got = ref.dehomogenise_f32(h)
    assert np.array_equal(got[0], [1, 2, 3]) and np.array_equal(got[1], [1, 2, 3]) and np.array_equal(got[3], [0, 1, 2])
    assert got[2, 0] == np.inf and got[2, 1] == -np.inf and np.isnan(got[2, 2])               # 1 / denormal overflows: inf * 0
    assert np.array_equal(got[4], [0, 0, 0])
    assert got.dtype == np.float32


@pytest.mark.parametrize("name", CALS)
def test_null_vector_is_the_right_one(name):
    c = case(name)
    r = ref.residual(c["A"], c["homog"])
    sv, bound = c["sv"], c["bound"]
    separated = sv[:, 2] > 100 * bound
    print("%s: residual / bound max %.6f; worst (residual - bound) / sigma_1 = %.3e; sigma_3 > 100 bound for %.1f %%"
          % (name, (r / bound).max(), ((r - bound) / sv[:, 0]).max(), 100 * separated.mean()))
    bad = np.flatnonzero(~(r <= bound))
    assert len(bad) == 0, [(int(i), c["f"]["d"][i], c["f"]["dy"][i], int(c["f"]["pos"][i]), sv[i].tolist(), r[i]) for i in bad[:5]]
    assert separated.mean() >= 0.60


@pytest.mark.parametrize("name", CALS)
def test_the_residual_bound_bites(name):
    """The check of the check: the right singular vector of sigma_3 — what reading row 2 of Vt instead of row 3 returns — taken
    from the reference's own SVD and rounded to f32 misses the bound on every well-separated point."""
    c = case(name)
    wrong = np.linalg.svd(c["A"])[2][:, 2, :].astype(np.float32)
    separated = c["sv"][:, 2] > 100 * c["bound"]
    assert (ref.residual(c["A"], wrong) > c["bound"])[separated].all()


@pytest.mark.parametrize("name", CALS)
def test_unit_norm(name):
    h = case(name)["homog"].astype(np.float64)
    assert np.abs(np.linalg.norm(h, axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("name", CALS)
def test_dehomogenisation_bit_for_bit(name):
    c = case(name)
    want = ref.dehomogenise_f32(c["homog"])
    assert np.array_equal(want.view(np.uint32), c["xyz"].view(np.uint32))


@pytest.mark.parametrize("name", CALS)
def test_zero_homogeneous_coordinate_is_reached(name):
    """Both branches of the rule run on fixture points (see the module docstring for why Wh is exactly zero there), and an
    unconditional 1 / Wh would give other bits on them."""
    c = case(name)
    wh = c["homog"][:, 3]
    zero = np.flatnonzero(wh == 0)
    tiny = np.flatnonzero(np.abs(wh) < 1e-6)
    print("%s: Wh == 0 at %s; |Wh| < 1e-6 at %d points (%.1f %%)" % (name, zero.tolist(), len(tiny), 100 * len(tiny) / len(wh)))
    assert len(zero) >= 1 and len(tiny) > len(zero)
    assert np.array_equal(c["xyz"][zero], c["homog"][zero, :3])                                  # scale 1
    with np.errstate(all="ignore"):
        unconditional = c["homog"][zero, :3] * (np.float32(1) / wh[zero])[:, None]
    assert not np.array_equal(unconditional.view(np.uint32), c["xyz"][zero].view(np.uint32))
    assert (wh != 0).sum() > 800


@pytest.mark.parametrize("name", ref.RECTIFIED)
def test_depth_follows_the_disparity_sign_included(name):
    c = case(name)
    sel, d, tol = ref.depth_check(c["Pr"], c["f"])
    assert len(sel) == 5 * 7 and (d < 0).sum() == 2 * 7
    z = c["xyz"][sel, 2].astype(np.float64)
    err = np.abs(z * d / -float(c["Pr"].reshape(3, 4)[0, 3]) - 1)
    print("%s: depth error / allowed, max %.3f" % (name, (err / tol).max()))
    assert (err <= tol).all(), (err / tol).max()
    assert np.array_equal(np.sign(z), np.sign(d))


def test_regimes_of_the_fixture():
    """Prints the table of the module docstring (run with -s) and holds its qualitative content: every regime is populated."""
    for name in CALS:
        c = case(name)
        separated = c["sv"][:, 2] > 100 * c["bound"]
        tiny = np.abs(c["homog"][:, 3]) < 1e-6
        with np.errstate(divide="ignore"):
            ratio = (c["sv"][:, 2] / c["sv"][:, 3]).min()
        print("%-8s sigma_3 > 100 bound %.1f %%, not separated %.1f %%, |Wh| < 1e-6 %.1f %%, Wh == 0: %d, min sigma_3 / sigma_4 %.3g"
              % (name, 100 * separated.mean(), 100 * (~separated).mean(), 100 * tiny.mean(), (c["homog"][:, 3] == 0).sum(), ratio))
        assert 0.6 <= separated.mean() < 1 and tiny.any()
