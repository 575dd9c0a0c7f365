"""tools/feature_bench.py descriptors on a real GPU, in a fresh process at the smallest shape its harness runs (as
tests/test_gpu_feature_bench.py): two contexts of two sequences, three measured steps, one round.  Checked: one JSON line with the
three legs off / tracks / descriptors, work done in every leg, and the feature's evidence — only the descriptors leg reads
descriptor rows.  No rate is checked."""
import json
import os

import pytest

from gpu_kit import run_child

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "feature_bench.py")
SMALL = ["--seqs", "4", "--contexts", "2", "--pool", "2", "--frames", "3", "--steps", "3", "--warmup", "1", "--depth", "2", "--repeat", "1"]


def test_feature_bench_descriptors_runs_every_leg():
    r = run_child(TOOL, "descriptors", *SMALL, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    print(out)
    assert out["feature"] == "descriptors" and list(out["legs"]) == ["off", "tracks", "descriptors"]
    for name, leg in out["legs"].items():
        assert all(x > 0 for x in leg["frame_pairs_per_s"]) and all(x > 0 for x in leg["inliers"]), (name, leg)
    assert sorted(out["ratio_to_off"]) == ["descriptors", "tracks"]
    legs = out["legs"]
    assert legs["off"]["descriptor_rows_of_sequence_0"] == [0] and legs["tracks"]["descriptor_rows_of_sequence_0"] == [0]
    assert legs["descriptors"]["descriptor_rows_of_sequence_0"][0] > 0, legs
    assert legs["descriptors"]["inliers"] == legs["tracks"]["inliers"] == legs["off"]["inliers"], "the outputs changed the frames"
