"""The C++ facade's guided search (include/svo/visual_odometry.hpp: DescriptorIndex::project, match_guided, select_guided,
localize_guided) on a real GPU: tests/cpp/guide_facade_test.cpp, compiled with g++ -Wall -Werror, on the repeated-structure scene of
tests/guide_cases.py — each of the facade's four calls returns its C entry's bytes, its candidates are the reference's (written
into the program's input), and its pose is svo_camera_to_world's on the candidate arrays."""
import subprocess

import numpy as np
import pytest

import guide_cases as cases
import guide_ref as gref
from test_guide_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    s = cases.repeated_scene()
    want = gref.select_index(s["K"], s["R0"], s["t0"], s["radius"], s["query"], s["xy"], s["desc"], s["ids"], s["xyz"], s["tags"])
    n, m, k = len(s["query"]), len(s["desc"]), len(want["query"])
    assert k == 160
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([n, m, k], np.int32).tobytes()); f.write(s["K"].astype(np.float32).tobytes())
        f.write(s["R0"].astype(np.float64).tobytes()); f.write(s["t0"].astype(np.float64).tobytes()); f.write(np.float32(s["radius"]).tobytes())
        f.write(s["query"].tobytes()); f.write(s["xy"].tobytes()); f.write(s["desc"].tobytes()); f.write(s["ids"].astype("<u8").tobytes())
        f.write(s["xyz"].tobytes()); f.write(s["tags"].tobytes()); f.write(want["query"].tobytes()); f.write(want["row"].tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GUIDE FACADE OK" in out.stdout, out.stdout + out.stderr
