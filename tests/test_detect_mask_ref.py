"""The detection-mask reference (tests/detect_mask_ref.py) on the CPU: the composition of stereo_callback from the oracle's stage
functions is pinned to orc_vo_stereo_callback before anything on the GPU is compared with it, and the filter rule is checked at
its rounding edges."""
import numpy as np

import detect_mask_ref as ref
import oracle_lib as orc
from gpu_kit import f32_bits as bits

W, H = 323, 163
OVER = dict(max_translation_norm=2.0)


def test_all_255_mask_reproduces_the_oracle_bit_for_bit():
    """A stream with a blank frame: a failing frame (the blank one), then one that takes the second pass, finds nothing and keeps
    the stale pyramids, then recovery.  Poses, feature sets, tracks and inlier masks equal orc_vo_stereo_callback's, with an
    all-255 mask and with none."""
    (L, R), (Pl, Pr) = ref.stream(7, 41, W, H, blank=(3,))
    full = np.full((H, W), 255, np.uint8)
    o = orc.VisualOdometry(orc.default_config(**OVER)); o.initalize_projection_matricies(Pl, Pr)
    ms = [ref.MaskedOracleVO(orc.default_config(**OVER)) for _ in range(2)]
    for m in ms:
        m.initalize_projection_matricies(Pl, Pr)
    fails, seconds, oks = [], [], []
    for k in range(len(L)):
        ok_o, T_o = o.stereo_callback(L[k], R[k])
        fo, to = o.features(), o.last_tracks()
        for m, mask in zip(ms, (full, None)):
            ok_m, T_m = m.stereo_callback(L[k], R[k], mask)
            assert ok_m == ok_o and np.array_equal(T_m.view(np.uint64), T_o.view(np.uint64)), k
            assert m.fail_reason == o.stats.fail_reason and int(m.second_pass) == o.stats.second_pass or k == 0, k
            fm = m.features()
            assert np.array_equal(bits(fm[0]), bits(fo[0])) and np.array_equal(fm[1], fo[1]) and np.array_equal(fm[2], fo[2]), k
            if k > 0:
                tm = m.last_tracks()
                for key in ("pl0", "pr0", "pl1", "pr1", "world"):
                    assert np.array_equal(bits(tm[key]), bits(to[key])), (k, key)
                assert np.array_equal(tm["inlier"], to["inlier"]), k
        fails.append(o.stats.fail_reason); seconds.append(o.stats.second_pass); oks.append(ok_o)
    print(fails, seconds, oks)
    assert 2 in fails and 1 in seconds and oks[1] and oks[-1], (fails, seconds, oks)
    assert o.stats.n_into_lk > 0 and 0 in [s for s in fails[1:]]


def test_mask_filter_rounding_edges():
    """(int)(v + 0.5f) in f32: k + 0.49999997 is 0.49999997 only at k = 0, where the f32 sum 0.99999997 rounds to 1.0 (ties to even),
    so the entry reads pixel 1, not 0 — OpenCV's behaviour, kept; at k >= 1 the coordinate itself rounds to k + 0.5.  v = size - 0.5
    rounds to `size` and is clamped to size - 1."""
    w, h = 9, 7
    for axis in (0, 1):
        n = (w, h)[axis]
        cases = [(np.float32(0.49999997), 1), (np.float32(0.5), 1), (np.float32(0.49), 0), (np.float32(3 + 0.49999997), 4), (np.float32(3.5), 4),
                 (np.float32(3.4999), 3), (np.float32(n - 0.5), n - 1), (np.float32(n - 1), n - 1), (np.float32(0), 0)]
        for v, pix in cases:
            for other in (0, 2):
                mask = np.zeros((h, w), np.uint8)
                xy = np.zeros((1, 2), np.float32); xy[0, axis] = v; xy[0, 1 - axis] = other
                idx = [0, 0]; idx[axis] = pix; idx[1 - axis] = other
                mask[idx[1], idx[0]] = 7
                assert ref.mask_filter(xy, mask)[0], (axis, v, pix)
                assert not ref.mask_filter(xy, np.where(mask != 0, 0, 255).astype(np.uint8))[0], (axis, v, pix)   # every other pixel allowed


def test_masked_append_keeps_ranks_and_drops_tracks():
    """A filtered entry makes no offer: a masked-out old track leaves its bucket to the FAST hit behind it; an all-zero mask
    empties the set; an all-255 one changes nothing."""
    (L, _), _ = ref.stream(2, 41, W, H)
    cfg = orc.default_config()
    none = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    base = ref.masked_append(L[0], none, None, cfg)
    assert len(base[1]) > 100
    same = ref.masked_append(L[0], none, np.full((H, W), 1, np.uint8), cfg)
    assert all(np.array_equal(a, b) for a, b in zip(base, same))
    assert len(ref.masked_append(L[0], base, np.zeros((H, W), np.uint8), cfg)[1]) == 0
    aged = (base[0], base[1] + 5, base[2])                            # old tracks win their buckets by age
    m = ref.band_mask(W, H, 100, 200)
    out = ref.masked_append(L[0], aged, m, cfg)
    assert ref.mask_filter(out[0], m).all() and 0 < len(out[1]) < len(ref.masked_append(L[0], aged, None, cfg)[1])
