"""tests/guide_ref.py on its own, no GPU: the rules of include/svo.h ("Guided search") on hand-made cases and exact rational arithmetic,
and the repeated-structure scene of tests/guide_cases.py — 160 landmarks, each stored twice 4 m apart with the same descriptor.

Measured on the CPU with np.random.default_rng(2501) and the draw order of guide_cases.repeated_scene: the unguided rules
(reloc_ref) give 0 candidates; the same rules over the rows the prior projects within 24 px give 160, every one the first copy; the
oracle's PnP on them (threshold 2.0 px, the prior as its guess) succeeds with 160 inliers, |R - R_true| <= 1.1e-4 and
|t - t_true| <= 1.2e-3.  The condition asserted: unguided 0, guided at least 150 of 160, a successful PnP at 2.0 px."""
from fractions import Fraction

import numpy as np

import desc_match_ref as mref
import guide_cases as cases
import guide_ref as gref
import oracle_lib as orc
import reloc_ref as rref


def test_the_repeated_structure_scene():
    s = cases.repeated_scene()
    arrays = (s["desc"], s["ids"], s["xyz"], s["tags"])
    plain = mref.match(s["query"], s["desc"], s["ids"])
    assert (plain["dist"] == 12).all() and (plain["dist2"] == 12).all()           # the copy looks exactly like the landmark
    assert (plain["row"] == np.arange(160)).all() and (plain["row2"] == np.arange(160) + 160).all()
    assert len(rref.select_index(s["query"], s["xy"], *arrays)["query"]) == 0
    got = gref.select_index(s["K"], s["R0"], s["t0"], s["radius"], s["query"], s["xy"], *arrays)
    print("guided candidates:", len(got["query"]))
    assert len(got["query"]) >= 150 and (got["row"] == got["query"]).all()         # the first copy, never the second
    assert len(got["query"]) == 160
    ok, R, t, inl, _ = orc.camera_to_world(s["K"], got["xy"], got["xyz"], s["R0"], s["t0"], 100, 2.0, 0.98)
    print("PnP:", ok, len(inl), np.abs(R - s["R"]).max(), np.abs(t - s["t"]).max())
    assert ok and len(inl) >= 150
    assert np.abs(R - s["R"]).max() < 1e-3 and np.abs(t - s["t"]).max() < 1e-2
    # the prior really is off: by about 0.01 rad and 0.1 m, some pixels by more than 10 px, all inside the radius
    off = np.abs(gref.project(s["K"], s["R0"], s["t0"], s["xyz"][:160], s["tags"][:160]) - s["xy"]).max(1)
    assert 10 < off.max() < s["radius"]
    assert 0.005 < np.linalg.norm(s["R0"] - s["R"]) < 0.02 and 0.09 < np.linalg.norm(s["t0"] - s["t"]) < 0.11


def test_projection_is_the_rounded_chain():
    rng = np.random.default_rng(3)
    for scale in (1.0, 1e3):
        R, t = rng.normal(size=(3, 3)), rng.normal(size=3) * scale
        K = np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32)
        p = (rng.normal(size=(60, 3)) * scale).astype(np.float32)
        uv = gref.project(K, R, t, p, np.zeros(60, np.int32))
        seen = 0
        for i in range(60):
            c = []
            for r in range(3):                                                      # each step rounded to f64, left to right
                v = float(Fraction(R[r, 0]) * Fraction(float(p[i, 0])))
                v = float(Fraction(v) + Fraction(float(Fraction(R[r, 1]) * Fraction(float(p[i, 1])))))
                v = float(Fraction(v) + Fraction(float(Fraction(R[r, 2]) * Fraction(float(p[i, 2])))))
                c.append(float(Fraction(v) + Fraction(t[r])))
            if not c[2] > 0:
                assert np.isposinf(uv[i]).all()
                continue
            seen += 1
            u = float(Fraction(float(Fraction(float(K[0, 0])) * Fraction(float(Fraction(c[0]) / Fraction(c[2]))))) + Fraction(float(K[0, 2])))
            v = float(Fraction(float(Fraction(float(K[1, 1])) * Fraction(float(Fraction(c[1]) / Fraction(c[2]))))) + Fraction(float(K[1, 2])))
            assert uv[i, 0] == np.float32(u) and uv[i, 1] == np.float32(v), i
        assert 10 < seen < 50                                                       # rows in front and behind


def test_rule_1_every_clause():
    xyz, tags = cases.clause_rows()
    for (K, R, t), want in zip(cases.CLAUSE_GUIDES, cases.CLAUSE_VISIBLE):
        uv = gref.project(K, R, t, xyz, tags)
        assert np.isfinite(uv).all(1).tolist() == want
        assert np.isposinf(uv[~np.isfinite(uv).all(1)]).all()                      # (+inf, +inf), never NaN or a half
    uv = gref.project(*cases.CLAUSE_GUIDES[0], xyz, tags)
    assert uv[0].tolist() == [400.0, 200.0] and uv[6].tolist() == [400.0, 200.0] and uv[7, 0] > 3e38
    assert np.float64(400) * (np.float64(1) / np.float64(np.float32(1e-37))) < 1e300   # row 3: finite in f64, beyond f32


def test_rule_2_every_clause():
    for radius in (24.0, 0.0, 0.25):
        xy, want = cases.clause_pixels(400, 200, radius)
        got = gref.admissible(np.array([[400, 200]], np.float32), xy, radius)[:, 0]
        assert got.tolist() == want.tolist(), radius
    xy, _ = cases.clause_pixels(400, 200, 24.0)                                     # radius 3e38: every finite pixel of an image is inside
    assert gref.admissible(np.array([[400, 200]], np.float32), xy, 3e38)[:, 0].tolist() == np.isfinite(xy).all(1).tolist()
    inv = np.array([[np.inf, np.inf]], np.float32)                                  # an invisible row is admissible for nobody
    xy, _ = cases.clause_pixels(400, 200, 24.0)
    assert not gref.admissible(inv, xy, 3e38).any()


def test_rule_3_is_the_search_over_the_admissible_rows():
    rng = np.random.default_rng(5)
    desc = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    ids = np.array([1, 1, 2, 3, 1, 2], np.uint64)
    uv = np.array([[10, 10], [12, 10], [np.inf, np.inf], [10, 14], [100, 100], [11, 11]], np.float32)
    query = desc[[2, 0, 4]].copy()
    xy = np.array([[10, 10], [10, 10], [50, 50]], np.float32)
    m = gref.match(query, xy, desc, ids, uv, 4.0)
    # query 0 is row 2's descriptor, but row 2 is invisible: the best of rows {0, 1, 3, 5}
    D = [[bin(int.from_bytes(bytes(a ^ b), "little")).count("1") for b in desc] for a in query]
    adm = [0, 1, 3, 5]
    best = min(adm, key=lambda r: (D[0][r], r))
    assert m["row"][0] == best and m["dist"][0] == D[0][best]
    second = min((r for r in adm if ids[r] != ids[best]), key=lambda r: (D[0][r], r))
    assert m["row2"][0] == second and m["id2"][0] == ids[second]
    assert m["row"][1] == 0 and m["dist"][1] == 0 and m["row2"][1] == min((3, 5), key=lambda r: (D[1][r], r))
    assert m["row"][2] == mref.NONE and m["dist"][2] == mref.NO_DIST and m["row2"][2] == mref.NONE   # admits nothing: an empty range's row
    # radius 3e38 and every row visible: the unguided search
    uv2 = np.where(np.isfinite(uv), uv, 0).astype(np.float32)
    assert gref.match(query, xy, desc, ids, uv2, 3e38).tobytes() == mref.match(query, desc, ids).tobytes()
    assert gref.match(query, xy, desc, ids, uv2, 3e38, 1, 4).tobytes() == mref.match(query, desc, ids, 1, 4).tobytes()
