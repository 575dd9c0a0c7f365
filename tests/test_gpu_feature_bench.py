"""tools/feature_bench.py on a real GPU, once per feature, in a fresh process at the smallest shape its harness runs: two contexts
of two sequences, three measured steps, one round.  Checked: one JSON line with every leg of the feature, work done in every leg
(frame pairs, inliers), ratio lists of the right length, and the feature's own evidence that a leg took its path.  No rate is
checked: two sequences per context are the lone-stream path, whose rates say nothing about the bench shape."""
import json
import os

import pytest

from gpu_kit import run_child

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "feature_bench.py")
# the legs as the recorded profiles name them, the baseline first
LEGS = dict(rectify=["a", "b", "c"], input_format=["mono8", "bgr8", "bgra8", "yuv422"], pose_cov=["off", "residual"],
            detect_mask=["off", "shared", "per_seq"], clahe=["off", "on", "on_bgr8"])
BPP = dict(mono8=1, bgr8=3, bgra8=4, yuv422=2)
REPEAT = 1
SMALL = ["--seqs", "4", "--contexts", "2", "--pool", "2", "--frames", "3", "--steps", "3", "--warmup", "1", "--depth", "2", "--repeat", str(REPEAT)]
W, H = 1241, 376                          # the tool's fixed image size


@pytest.mark.parametrize("feature", list(LEGS))
def test_feature_bench_runs_every_leg(feature):
    r = run_child(TOOL, feature, *SMALL, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    print(out)
    names = LEGS[feature]
    base = names[0]
    assert out["feature"] == feature and list(out["legs"]) == names
    for name, leg in out["legs"].items():
        assert all(len(v) == REPEAT for v in leg.values()), (name, leg)
        assert all(x > 0 for x in leg["frame_pairs_per_s"]) and all(x > 0 for x in leg["inliers"]), (name, leg)
        assert len([k for k in leg if k.endswith("_ms")]) == 1, (name, leg)
    for key in ("ratio_to_%s_per_round" % base, "ratio_to_%s" % base):
        assert sorted(out[key]) == sorted(names[1:]), out[key]
    assert all(len(v) == REPEAT for v in out["ratio_to_%s_per_round" % base].values())
    assert out["%s_round_to_round_spread" % base] >= 0
    legs = out["legs"]
    if feature == "detect_mask":
        assert legs["off"]["masked_frames"] == [0] * REPEAT
        assert all(x > 0 for x in legs["shared"]["masked_frames"] + legs["per_seq"]["masked_frames"]), legs
    elif feature == "pose_cov":
        assert all(x > 0 for x in legs["residual"]["valid_covariances"]), legs
    elif feature == "input_format":
        for name, leg in legs.items():
            assert leg["source_bytes_per_pair"] == [2 * W * H * BPP[name]] * REPEAT, (name, leg)
