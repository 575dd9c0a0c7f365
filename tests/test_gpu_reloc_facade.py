"""The C++ facade's relocaliser (include/svo/visual_odometry.hpp: DescriptorIndex::enable_points, add_points, select, localize) on a
real GPU: tests/cpp/reloc_facade_test.cpp, compiled with g++ -Wall -Werror, on a 70-landmark scene of tests/reloc_cases.py with ten
pixels moved and some queries sharing a landmark — the facade's candidates are the reference's (written into the program's input),
and its pose, inlier flags and iteration count are svo_camera_to_world's on the candidate arrays byte for byte."""
import subprocess

import numpy as np
import pytest

import reloc_cases as cases
import reloc_ref as rref
from test_reloc_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    s = cases.scene(70, 9, outliers=10)
    ids = s["ids"].copy()
    ids[60:] = ids[50:60]                               # ten landmarks seen twice in the index: rule 2 has work
    want = rref.select_index(s["query"], s["xy"], s["desc"], ids, s["xyz"], s["tags"])
    n, m, k = len(s["query"]), len(s["desc"]), len(want["query"])
    assert k == 60
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([n, m, k], np.int32).tobytes()); f.write(s["K"].astype(np.float32).tobytes())
        f.write(s["query"].tobytes()); f.write(s["xy"].tobytes()); f.write(s["desc"].tobytes()); f.write(ids.astype("<u8").tobytes())
        f.write(s["xyz"].tobytes()); f.write(s["tags"].tobytes()); f.write(want["query"].tobytes()); f.write(want["row"].tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RELOC FACADE OK" in out.stdout, out.stdout + out.stderr
