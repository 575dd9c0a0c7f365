"""The reference for track ids (tests/track_ids_ref.py) on the CPU: with the ids ignored IdOracleVO is MaskedOracleVO without a
mask, bit for bit; and on every frame the identity rule's invariants hold — ids unique within a feature set, a row whose id was in
the previous feature set starts (l0) at that feature's position with its age + 1, every other row's id is at least the next_id the
frame's detection started from.  The same asserts keep the streams from being vacuous: from the third frame on every frame must
have continuing and fresh ids, ages must grow, and the stream with independently moving blobs must have non-inlier rows (the plain
stream is all-inlier and alone could not catch a wrong inlier move).  323 x 163, seed 900, max_translation_norm = 2.0."""
import numpy as np
import pytest

import detect_mask_ref as mref
import oracle_lib as orc
import track_ids_ref as ref

W, H, SEED = 323, 163, 900
OVER = dict(max_translation_norm=2.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def runs():
    """{stream name: per-frame records of one IdOracleVO run}, computed once"""
    out = {}
    for name, n, movers in (("plain", 6, 0.0), ("movers", 5, 0.3)):
        (L, R), P = ref.stream(n, SEED, W, H, movers=movers)
        o = ref.IdOracleVO(orc.default_config(**OVER)); o.initalize_projection_matricies(*P)
        m = mref.MaskedOracleVO(orc.default_config(**OVER)); m.initalize_projection_matricies(*P)
        recs = []
        for k in range(n):
            prev = (o.features()[0].copy(), o.features()[1].copy(), o.feature_ids().copy())
            ok, T = o.stereo_callback(L[k], R[k])
            ok_m, T_m = m.stereo_callback(L[k], R[k])
            recs.append(dict(ok=ok, T=T, ok_m=ok_m, T_m=T_m, prev=prev, next_before=o.next_id_before_detect, next_after=o.next_id,
                             feats=tuple(a.copy() for a in o.features()), ids=o.feature_ids().copy(), obs=o.obs(), fail=o.fail_reason,
                             m_feats=tuple(a.copy() for a in m.features()), m_tracks=m.last_tracks(), tracks=o.last_tracks(), m_fail=m.fail_reason))
        out[name] = recs
    return out


@pytest.mark.parametrize("name", ["plain", "movers"])
def test_ids_ignored_it_is_the_masked_oracle_without_a_mask(runs, name):
    for k, r in enumerate(runs[name]):
        assert r["ok"] == r["ok_m"] and r["fail"] == r["m_fail"], k
        assert np.array_equal(r["T"], r["T_m"]), k
        assert np.array_equal(bits(r["feats"][0]), bits(r["m_feats"][0])) and np.array_equal(r["feats"][1], r["m_feats"][1]) and \
            np.array_equal(r["feats"][2], r["m_feats"][2]), k
        if r["m_tracks"] is None:
            continue
        for key in ("pl0", "pr0", "pl1", "pr1", "world"):
            assert np.array_equal(bits(r["tracks"][key]), bits(r["m_tracks"][key])), (k, key)
        assert np.array_equal(r["tracks"]["inlier"], r["m_tracks"]["inlier"]), k


@pytest.mark.parametrize("name", ["plain", "movers"])
def test_identity_invariants_on_every_frame(runs, name):
    max_age, non_inlier_frames = 0, 0
    for k, r in enumerate(runs[name]):
        ids, obs = r["ids"], r["obs"]
        assert len(ids) == len(r["feats"][1]) and len(np.unique(ids)) == len(ids), "frame %d: feature ids not unique" % k
        assert len(np.unique(obs["id"])) == len(obs), "frame %d: row ids not unique" % k
        assert r["next_after"] >= r["next_before"] and (len(ids) == 0 or ids.max() < r["next_after"]), k
        pxy, page, pid = r["prev"]
        where = {int(i): j for j, i in enumerate(pid)}
        cont = np.array([int(i) in where for i in obs["id"]], bool)
        for row in obs[cont]:
            j = where[int(row["id"])]
            assert np.array_equal(bits(row["l0"]), bits(pxy[j])), "frame %d id %d: l0 is not the previous feature's position" % (k, row["id"])
            assert row["age"] == page[j] + 1, "frame %d id %d: age" % (k, row["id"])
        assert (obs["id"][~cont] >= r["next_before"]).all(), "frame %d: a fresh row's id is below the detection's next_id" % k
        assert (obs["age"][~cont] == 1).all(), k
        print("%s frame %d: %d rows, %d continue, %d fresh, %d inliers, max age %d, fail %d" %
              (name, k, len(obs), cont.sum(), (~cont).sum(), (obs["flags"] & ref.OBS_INLIER).astype(bool).sum(), obs["age"].max() if len(obs) else 0, r["fail"]))
        if k >= 3:
            assert cont.sum() >= 1 and (~cont).sum() >= 1, "frame %d: the stream is vacuous (continuing %d, fresh %d)" % (k, cont.sum(), (~cont).sum())
        if len(obs):
            max_age = max(max_age, int(obs["age"].max()))
            if r["fail"] in (0, 4):
                non_inlier_frames += int(((obs["flags"] & ref.OBS_INLIER) == 0).any())
                # rule 3: the feature set after the frame is the inlier rows, in order
                inl = (obs["flags"] & ref.OBS_INLIER).astype(bool)
                assert np.array_equal(ids, obs["id"][inl]) and np.array_equal(bits(r["feats"][0]), bits(obs["l1"][inl])), k
    if name == "plain":
        assert max_age >= 5, max_age
        assert len(runs[name][1]["obs"]) == 445 and len(runs[name][2]["obs"]) == 623, "the stream is not the one the counts were measured on"
    else:
        assert non_inlier_frames >= 2, non_inlier_frames
