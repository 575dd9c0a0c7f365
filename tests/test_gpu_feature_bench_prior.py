"""tools/feature_bench.py prior on a real GPU, in a fresh process at the smallest shape its harness runs (the pattern of
tests/test_gpu_feature_bench.py): two contexts of two sequences, three measured steps, one round, a turning scene (--yaw-amp 8: up to
3 degrees per frame).  Checked: one JSON line with the legs off, identity and rotation; work done in every leg; the path bit as evidence
that the prior legs launched the prior kernel and the off leg never did; the identity leg does the off leg's work (same tracks, same
Newton steps: an identity prior changes no bit); the rotation leg needs fewer Newton steps than the off leg on the same frames.  No
rate is checked."""
import json
import os

import pytest

from gpu_kit import run_child

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "feature_bench.py")
REPEAT = 1
SMALL = ["--seqs", "4", "--contexts", "2", "--pool", "2", "--frames", "3", "--steps", "3", "--warmup", "1", "--depth", "2", "--repeat", str(REPEAT),
         "--yaw-amp", "8"]


def test_feature_bench_prior_runs_every_leg():
    r = run_child(TOOL, "prior", *SMALL, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    print(out)
    legs = out["legs"]
    assert out["feature"] == "prior" and list(legs) == ["off", "identity", "rotation"]
    for name, leg in legs.items():
        assert all(len(v) == REPEAT for v in leg.values()), (name, leg)
        assert all(x > 0 for x in leg["frame_pairs_per_s"]) and all(x > 0 for x in leg["lk_newton_steps"]) and "lk_ms" in leg, (name, leg)
    assert sorted(out["ratio_to_off"]) == ["identity", "rotation"] and out["off_round_to_round_spread"] >= 0
    assert legs["off"]["prior_frames"] == [0] * REPEAT
    assert all(x > 0 for x in legs["identity"]["prior_frames"] + legs["rotation"]["prior_frames"]), legs
    for field in ("n_after_circular", "lk_newton_steps", "inliers", "ok_frames"):
        assert legs["identity"][field] == legs["off"][field], (field, legs)
    assert legs["rotation"]["lk_newton_steps"][0] < legs["off"]["lk_newton_steps"][0], legs
    assert legs["rotation"]["n_after_circular"][0] >= legs["off"]["n_after_circular"][0], legs
