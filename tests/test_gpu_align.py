"""The descriptor index's map alignment (include/svo.h, "Map alignment": svo_desc_index_match_rows, svo_desc_index_pair_rows,
svo_desc_index_align) on a real GPU against the numpy reference (tests/align_ref.py) on the synthetic rows of tests/align_cases.py.

Tolerances.  Rules 1 - 5 are integers: equality.  Rules 6 - 10 are f64 on both sides, with eigenvectors and sums taken differently,
so the models agree to rounding and not in every bit; each test first asserts on the CPU that no residual of the reference's final
model lies within 10 % of inlier_dist of the threshold, and then holds the sets to equality, t to 1e-6 m and the angle of
R_gpu R_ref^T to 1e-6 rad — the pose tolerance the project holds its HIP path to against the oracle.  best_hypothesis and best_count
are asserted where the reference's margin over ALL hypotheses is above 1e-6 (the noise-free scenes are), and printed elsewhere."""
import numpy as np
import pytest

import align_cases as ac
import align_ref as aref
from gpu_kit import projections, streams
from stereo_visual_odometry_amd import _lib, api

pytestmark = pytest.mark.gpu

T_TOL, R_TOL = 1e-6, 1e-6


# ---- 1. match_rows equals match, bit for bit
@pytest.fixture(scope="module")
def big_rows():
    """4096 + 300 + 4096 rows: a span of 4096 on either side of a middle one; descriptors from a pool of 512 so that distances tie"""
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 256, (512, 32), dtype=np.uint8)
    m = 4096 + 300 + 4096
    lm = rng.integers(0, 512, m)
    desc = ac.flip_bits(rng, pool[lm], rng.integers(0, 3, m))
    return desc, (lm % 200).astype(np.uint64)


@pytest.mark.parametrize("chunk", (1, 64, 0))
def test_match_rows_equals_match(big_rows, chunk):
    desc, ids = big_rows
    m = len(desc)
    index = api.DescriptorIndex(m)                     # rule 1 needs no points
    index.add(desc, ids)
    index.chunk_rows = chunk
    # (src, dst): source spans of 0, 1, 63, 64, 65 and 4096 rows, in front of and behind the destination; destinations that start
    # and end inside a chunk of 64 and of 1024 rows; spans that touch; an empty destination
    spans = [((4500, 4500), (0, 4396)), ((4396, 4397), (100, 4301)), ((4396, 4459), (37, 1500)), ((4396, 4460), (1025, 3000)),
             ((0, 65), (65, 300)), ((4396, m), (3, 4393)), ((0, 4096), (4100, m - 5)), ((0, 4096), (4096, 4396)), ((10, 20), (30, 30))]
    if chunk == 1:                                     # a chunk per row: keep the pieces few
        spans = [(s, (d[0], min(d[1], d[0] + 150))) for s, d in spans]
    for src, dst in spans:
        got = index.match_rows(src, dst)
        want = index.match(desc[src[0]:src[1]], dst[0], dst[1])
        assert len(got) == src[1] - src[0] and got.tobytes() == want.tobytes(), (src, dst)
    assert index.match_rows((m - 10, -1), (0, 100)).tobytes() == index.match(desc[m - 10:], 0, 100).tobytes()   # row_hi = -1


def test_match_rows_above_the_scratch_budget():
    """n x pieces above 1 << 22 partial states: the search goes in launches of fewer queries, by the existing plan"""
    rng = np.random.default_rng(11)
    desc = rng.integers(0, 256, (4096 + 1100, 32), dtype=np.uint8)
    ids = np.arange(len(desc)).astype(np.uint64)
    index = api.DescriptorIndex(len(desc))
    index.add(desc, ids)
    index.chunk_rows = 1                               # 1100 pieces x 4096 queries = 4.5 M states
    got = index.match_rows((1100, 1100 + 4096), (0, 1100))
    index.chunk_rows = 0
    assert got.tobytes() == index.match(desc[1100:], 0, 1100).tobytes()


# ---- 2. pair_rows equals the reference
@pytest.mark.parametrize("name", ac.PAIR_SCENES)
def test_pair_rows_equals_the_reference(name):
    case = ac.pair_scene(name)
    index = ac.build_index(api, case)
    ps, pd = index.pair_rows(case["src"], case["dst"])
    want_s, want_d = aref.pairs(case["desc"], case["ids"], case["tags"], case["src"], case["dst"])
    assert np.array_equal(ps, want_s) and np.array_equal(pd, want_d)
    res, pairs = index.align(case["src"], case["dst"], 0.05)                        # the same lists from the whole call
    assert np.array_equal(pairs["src"], want_s) and np.array_equal(pairs["dst"], want_d) and res.n_pairs == len(want_s)
    tight = dict(max_dist=3, ratio_num=1, ratio_den=2)                              # another rule 2
    ps, pd = index.pair_rows(case["src"], case["dst"], **tight)
    want_s, want_d = aref.pairs(case["desc"], case["ids"], case["tags"], case["src"], case["dst"], 3, 1, 2)
    assert np.array_equal(ps, want_s) and np.array_equal(pd, want_d)


def test_pair_rows_of_4096_rows_that_all_collapse():
    """4096 accepted source rows of ONE landmark against 3 destination landmarks: both walks at their full length"""
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    lm = rng.integers(0, 3, 4096)
    desc = np.concatenate([base, ac.flip_bits(rng, base[lm], rng.integers(0, 4, 4096))])
    ids = np.concatenate([[10, 11, 12], 100 + (np.arange(4096) % 2)]).astype(np.uint64)    # two source landmarks, seen 2048 times each
    xyz = rng.uniform(-5, 5, (4099, 3)).astype(np.float32)
    case = dict(desc=desc, ids=ids, xyz=xyz, tags=np.zeros(4099, np.int32), src=(3, 4099), dst=(0, 3))
    index = ac.build_index(api, case)
    ps, pd = index.pair_rows(case["src"], case["dst"])
    want_s, want_d = aref.pairs(desc, ids, case["tags"], case["src"], case["dst"])
    assert np.array_equal(ps, want_s) and np.array_equal(pd, want_d) and 1 <= len(ps) <= 2


# ---- 3. align against the reference
def check_against_reference(res, pairs, want, assert_best):
    assert res.n_pairs == want["n_pairs"] and np.array_equal(pairs["src"], want["pair_src"]) and np.array_equal(pairs["dst"], want["pair_dst"])
    assert np.array_equal(pairs["inlier"], want["inlier"]) and res.n_inliers == want["n_inliers"] and res.success == want["success"]
    dt, dr = np.abs(res.t - want["t"]).max(), aref.rotation_angle(res.R, want["R"])
    print("t %.3g m, R %.3g rad, rms %.6g / %.6g, best %d (%d) / %d (%d), rounds %d / %d, margin %.3g" % (
        dt, dr, res.rms, want["rms"], res.best_hypothesis, res.best_count, want["best_hypothesis"], want["best_count"],
        res.refit_rounds_run, want["refit_rounds_run"], want["margin"]))
    assert dt <= T_TOL and dr <= R_TOL
    assert np.array_equal(res.T[:3, :3], res.R) and np.array_equal(res.T[:3, 3], res.t) and np.array_equal(res.T[3], [0, 0, 0, 1])
    assert abs(res.rms - want["rms"]) <= 1e-6
    if assert_best:
        assert (res.best_hypothesis, res.best_count, res.refit_rounds_run) == (want["best_hypothesis"], want["best_count"], want["refit_rounds_run"])


@pytest.mark.parametrize("n, share, H, sigma", ac.MOTION_CASES)
def test_align_against_the_reference(n, share, H, sigma):
    case, want = ac.motion_scene(n, share, sigma), ac.motion_reference(n, share, H, sigma)
    assert want["success"] and want["n_pairs"] == n and want["margin_final"] > 0.1          # the scene's condition, on the CPU
    index = ac.build_index(api, case)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H)
    check_against_reference(res, pairs, want, assert_best=want["margin"] > 1e-6)
    assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"])                    # exactly the true inliers


# ---- 4. gates
def test_too_few_pairs():
    case = ac.motion_scene(4, 0.0, 0.0)
    index = ac.build_index(api, case)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=5)
    assert not res.success and res.n_pairs == 4 and len(pairs["src"]) == 4 and not pairs["inlier"].any()
    assert (res.n_inliers, res.best_hypothesis, res.best_count, res.refit_rounds_run, res.rms) == (0, -1, 0, 0, 0.0)
    assert not res.T.any() and not res.R.any() and not res.t.any()
    res, _ = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=4)
    assert res.success and res.n_inliers == 4


def test_all_outliers():
    case = ac.motion_scene(64, 1.0, 0.0)
    index = ac.build_index(api, case)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, hypotheses=64)
    print(res.n_pairs, res.n_inliers, res.best_count)
    assert not res.success and res.n_pairs == 64 and res.n_inliers < 6 and not res.T.any() and res.rms == 0.0


def test_without_refit_the_result_is_the_best_hypothesis():
    n, share, H, sigma = 64, 0.5, 128, 0.0
    case = ac.motion_scene(n, share, sigma)
    want = ac.motion_reference(n, share, H, sigma, refit_rounds=0)
    assert want["margin"] > 1e-6 and want["refit_rounds_run"] == 0
    index = ac.build_index(api, case)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H, refit_rounds=0)
    check_against_reference(res, pairs, want, assert_best=True)
    P, Q = case["xyz"][want["pair_src"]], case["xyz"][want["pair_dst"]]
    pick = aref.sample(res.best_hypothesis, n)
    R, t = aref.horn(P[pick].astype(np.float64), Q[pick].astype(np.float64))               # the model of that hypothesis' three pairs
    assert np.abs(res.t - t).max() <= T_TOL and aref.rotation_angle(res.R, R) <= R_TOL and res.n_inliers == res.best_count


# ---- 5. independence
def result_bytes(res, pairs):
    return b"".join([np.array(res[:6], np.int64).tobytes(), res.R.tobytes(), res.t.tobytes(), res.T.tobytes(), np.float64(res.rms).tobytes(),
                     pairs["src"].tobytes(), pairs["dst"].tobytes(), pairs["inlier"].tobytes()])


def test_same_bits_twice_and_at_any_chunk():
    n, share, H, sigma = 1025, 0.6, 512, 0.0
    case = ac.motion_scene(n, share, sigma)
    index = ac.build_index(api, case)
    args = (case["src"], case["dst"], ac.INLIER_DIST)
    first = result_bytes(*index.align(*args, hypotheses=H))
    assert result_bytes(*index.align(*args, hypotheses=H)) == first
    index.pair_rows(case["dst"], case["src"])                                       # another call in between leaves nothing behind
    index.chunk_rows = 1
    assert result_bytes(*index.align(*args, hypotheses=H)) == first
    other = ac.build_index(api, case, extra=10)
    assert result_bytes(*other.align(*args, hypotheses=H)) == first


def test_beside_frames_in_flight():
    """align on the index's own stream while a context has frames in flight: the same bits, and the frames' results unchanged"""
    import torch
    W, Hh, n_seq, n_frames = 320, 160, 2, 6
    seqs = streams(n_seq, n_frames, 900, W, Hh)
    dev = [[(torch.from_numpy(L[k]).cuda(), torch.from_numpy(R[k]).cuda()) for L, R in seqs] for k in range(n_frames)]
    torch.cuda.synchronize()

    def run(between):
        """six frames of two sequences as device frames, three in flight -> per frame (ok, poses, features) as bytes"""
        vo = api.BatchVisualOdometry(W, Hh, n_seq, api.default_config(max_translation_norm=2.0, ransac_reprojection_error=0.25))
        vo.initalize_projection_matricies(*projections(W, Hh))
        out = []
        try:
            for k0 in range(0, n_frames, 3):
                for k in range(k0, k0 + 3):
                    vo.submit_device([a.data_ptr() for a, _ in dev[k]], [b.data_ptr() for _, b in dev[k]], W)
                    between()
                for k in range(k0, k0 + 3):
                    ok, T = vo.collect()
                    out.append((ok.tobytes(), T.tobytes(), b"".join(vo.features(i)[0].tobytes() for i in range(n_seq))))
        finally:
            vo.close()
        return out

    n, share, H, sigma = 65, 0.5, 128, 0.005
    case = ac.motion_scene(n, share, sigma)
    index = ac.build_index(api, case)
    alone = result_bytes(*index.align(case["src"], case["dst"], ac.INLIER_DIST, hypotheses=H))
    beside = []
    quiet = run(lambda: None)
    busy = run(lambda: beside.append(result_bytes(*index.align(case["src"], case["dst"], ac.INLIER_DIST, hypotheses=H))))
    assert busy == quiet and len(beside) == n_frames and all(b == alone for b in beside)
    assert np.frombuffer(quiet[-1][0], np.uint8).any()                              # the frames did produce poses


# ---- 6. the round trip
@pytest.mark.parametrize("n, share, H, sigma", ((1024, 0.6, 512, 0.005), (4096, 0.0, 8, 0.0)))
def test_round_trip_through_transform_points(n, share, H, sigma):
    """align, move the source span by T, align again: the identity, with the same inliers.  The moved points are rounded to f32 at up
    to 80 m (half an ulp: 4e-6 m a coordinate); the least-squares fit of hundreds of inliers averages that to well below 1e-6."""
    case = ac.motion_scene(n, share, sigma)
    index = ac.build_index(api, case)
    args = (case["src"], case["dst"], ac.INLIER_DIST)
    res, pairs = index.align(*args, min_pairs=3, hypotheses=H)
    assert res.success
    assert index.transform_points(res.T, rows=case["src"]) == (n, 0)
    again, pairs2 = index.align(*args, min_pairs=3, hypotheses=H)
    print("t %.3g m, R %.3g rad" % (np.abs(again.t).max(), aref.rotation_angle(again.R, np.eye(3))))
    assert again.success and again.n_inliers == res.n_inliers and np.array_equal(pairs2["inlier"], pairs["inlier"])
    assert np.abs(again.t).max() <= T_TOL and aref.rotation_angle(again.R, np.eye(3)) <= R_TOL


# ---- 7. refusals
def test_refusals_leave_the_outputs_untouched():
    case = ac.motion_scene(64, 0.5, 0.0)
    index = ac.build_index(api, case)
    size = index.size
    ok = dict(src_lo=64, src_hi=128, dst_lo=0, dst_hi=64)
    bad = [dict(src_lo=-1), dict(src_hi=size + 1), dict(src_lo=100, src_hi=99), dict(dst_lo=-1), dict(dst_hi=size + 1), dict(dst_lo=60, dst_hi=59),
           dict(dst_hi=65), dict(dst_hi=-1), dict(src_lo=63), dict(src_lo=0, src_hi=-1),
           dict(max_dist=-1), dict(max_dist=257), dict(ratio_num=0), dict(ratio_den=0), dict(ratio_num=(1 << 20) + 1), dict(ratio_den=(1 << 20) + 1),
           dict(min_pairs=2), dict(min_pairs=4097), dict(hypotheses=0), dict(hypotheses=1025), dict(refit_rounds=-1), dict(refit_rounds=9),
           dict(inlier_dist=0.0), dict(inlier_dist=-0.05), dict(inlier_dist=float("inf")), dict(inlier_dist=float("nan"))]
    import ctypes as C
    for over in bad:
        p = api.DescriptorIndex.align_params((ok["src_lo"], ok["src_hi"]), (ok["dst_lo"], ok["dst_hi"]), 0.05)
        for k, v in over.items():
            setattr(p, k, v)
        r = _lib.SvoAlignResult()
        C.memset(C.byref(r), 0x5A, C.sizeof(r))
        before = bytes(r)
        ps, pd, pi = np.full(200, 77, np.int32), np.full(200, 77, np.int32), np.full(200, 77, np.uint8)
        k = C.c_int(-7)
        assert _lib.lib.svo_desc_index_align(index._h, C.byref(p), C.byref(r), _lib.ptr(ps), _lib.ptr(pd), _lib.ptr(pi)) == _lib.SVO_ERR_ARG, over
        assert _lib.lib.svo_desc_index_pair_rows(index._h, C.byref(p), C.byref(k), _lib.ptr(ps), _lib.ptr(pd)) == _lib.SVO_ERR_ARG, over
        assert bytes(r) == before and (ps == 77).all() and (pd == 77).all() and (pi == 77).all() and k.value == -7, over
    rows = np.zeros(10, _lib.DESC_MATCH_DTYPE); rows["row"] = 99
    for src, dst in (((-1, 5), (10, 20)), ((0, size + 1), (0, 0)), ((5, 4), (10, 20)), ((0, 5), (-1, 20)), ((0, 5), (10, size + 1)), ((0, 5), (4, 20)), ((0, 10), (0, -1))):
        assert _lib.lib.svo_desc_index_match_rows(index._h, src[0], src[1], dst[0], dst[1], _lib.ptr(rows)) == _lib.SVO_ERR_ARG, (src, dst)
        assert (rows["row"] == 99).all()
    assert _lib.lib.svo_desc_index_match_rows(index._h, 0, 5, 10, 20, None) == _lib.SVO_ERR_ARG
    # spans that touch are legal, and so is an empty source span inside the destination
    res, _ = index.align((64, 128), (0, 64), 0.05)
    assert res.success
    res, pairs = index.align((10, 10), (0, 64), 0.05)
    assert not res.success and res.n_pairs == 0 and len(pairs["src"]) == 0
    # more than 4096 source rows
    big = api.DescriptorIndex(4200, points=True)
    big.add_points(np.zeros((4200, 32), np.uint8), np.arange(4200), np.zeros((4200, 3), np.float32))
    with pytest.raises(_lib.SvoError, match="4096 source rows"):
        big.align((0, 4097), (4097, 4200), 0.05)
    with pytest.raises(_lib.SvoError, match="4096 source rows"):
        big.match_rows((0, 4097), (4097, 4200))
    assert len(big.match_rows((0, 4096), (4096, 4200))) == 4096
    # an index without points
    plain = api.DescriptorIndex(16)
    plain.add(np.zeros((8, 32), np.uint8), np.arange(8))
    r = _lib.SvoAlignResult()
    p = api.DescriptorIndex.align_params((0, 4), (4, 8), 0.05)
    assert _lib.lib.svo_desc_index_align(plain._h, C.byref(p), C.byref(r), None, None, None) == _lib.SVO_ERR_STATE
    assert _lib.lib.svo_desc_index_pair_rows(plain._h, C.byref(p), None, None, None) == _lib.SVO_ERR_STATE
    assert len(plain.match_rows((0, 4), (4, 8))) == 4                               # rule 1 needs no points
    assert _lib.lib.svo_desc_index_align(index._h, None, C.byref(r), None, None, None) == _lib.SVO_ERR_ARG
    assert _lib.lib.svo_desc_index_align(index._h, C.byref(p), None, None, None, None) == _lib.SVO_ERR_ARG


def test_null_lists_and_timing():
    import ctypes as C
    case = ac.motion_scene(64, 0.5, 0.0)
    index = ac.build_index(api, case)
    p = api.DescriptorIndex.align_params(case["src"], case["dst"], 0.05)
    r = _lib.SvoAlignResult()
    assert _lib.lib.svo_desc_index_align(index._h, C.byref(p), C.byref(r), None, None, None) == 0 and r.success == 1 and r.n_inliers == 32
    assert index.stats()["last_kernels_ms"] == 0.0
    index.set_timing(True)
    index.align(case["src"], case["dst"], 0.05)
    assert 0.0 < index.stats()["last_kernels_ms"] < 1000.0
