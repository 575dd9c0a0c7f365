"""The C++ facade's predicted prior (include/svo/visual_odometry.hpp) on a GPU: tests/cpp/auto_prior_test.cpp runs the three frames of
the turning scene through a VisualOdometry in SVO_PRIOR_LAST_ROTATION and through a C-ABI context that is handed the host
restatement of the rule, and compares them byte for byte."""
import subprocess

import numpy as np
import pytest

import lk_prior_cases as pc
from test_auto_prior_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_agrees_with_the_host_restatement(tmp_path):
    w, h = 320, 240
    sc = pc.scene(w, h)
    Pl, Pr = pc.projections(w, h)
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([3, h, w], np.int32).tobytes())
        f.write(Pl.tobytes()); f.write(Pr.tobytes()); f.write(np.ascontiguousarray(pc.rotation(w, h, 1), np.float64).tobytes())
        for k in range(3):
            f.write(sc.left[k].tobytes()); f.write(sc.right[k].tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "AUTO PRIOR FACADE OK" in out.stdout, out.stdout + out.stderr
