"""The register-walking pyrDown (k_pyr_walk: ingest + level 1, then every further level) and the row-wise border kernel
(k_pad_pyramid) of the plain many-sequence contexts, at the sizes of tests/pyr_walk_cases.py (tests/test_pyr_walk_cases.py guards
the matrix and runs the walk on the host).

Every case is a plain grey context of 9 .. 12 sequences in the exact-sums mode; every frame must report SVO_PATH_INGEST_AHEAD.  For
the three frames after which no frame is in flight, every sequence and both cameras:
- every byte of every level of the T1 pyramids and of lastLeftPyramid's pair, border included, equals tests/pyramid_ref.py;
- the derivative planes built on them, border included, equal tests/deriv_ref.py sample for sample;
- the flags, every statistics field, the feature sets and the poses — bit for bit: everything downstream reads the same bytes —
  equal those of the same frames run in a child process with SVO_PYR_WALK=0, which keeps the LDS-tiled pyramid kernels.
The SVO_INGEST_AHEAD=0 route runs in a child of its own (both switches are read once per process)."""
import json
import os

import numpy as np
import pytest

import pyr_walk_cases as pw
import pyr_walk_child as child
from gpu_kit import api, run_child  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent_reports(tmp_path_factory):
    """What every frame of every case reports with the parent's pyramid kernels: one child process for the whole matrix."""
    path = str(tmp_path_factory.mktemp("pyr_walk") / "parent.npz")
    r = run_child("pyr_walk_child.py", json.dumps(pw.CASES), path, env=dict(os.environ, SVO_PYR_WALK="0"), timeout=600)
    assert "pyr walk child ok: %d cases" % len(pw.CASES) in r.stdout
    return np.load(path)


@pytest.mark.parametrize("case", pw.CASES, ids=pw.case_id)
def test_levels_planes_and_frame_results(api, parent_reports, case):
    assert "SVO_PYR_WALK" not in os.environ, "the suite runs the walking kernels: unset SVO_PYR_WALK"
    got = child.run(api, case, check=True)
    what = pw.case_id(case)
    assert len(got) == 2 + case[6].get("depth", 1)
    assert any(fr["ok"].any() for fr in got) and any(fr["n_feat"].sum() > 0 for fr in got), (what, "no frame gave a pose or features")
    for k, fr in enumerate(got):
        for name, a in fr.items():
            want = parent_reports["%s/%d/%s" % (what, k, name)]
            assert a.shape == want.shape and np.array_equal(a, want), (what, "frame", k, name, "differs from the run with SVO_PYR_WALK=0")


def test_many_sequences_without_build_ahead():
    """The same kernels on the frame's own stream (SVO_INGEST_AHEAD=0): pyramids byte for byte, through test_gpu_pyramids.run_case."""
    env = dict(os.environ, SVO_INGEST_AHEAD="0")
    env.pop("SVO_PYR_WALK", None)
    r = run_child("pyramid_child.py", json.dumps(pw.MANY_CASES), env=env, timeout=600)
    assert "pyramid child ok: %d cases" % len(pw.MANY_CASES) in r.stdout
