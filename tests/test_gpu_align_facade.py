"""The C++ facade's map alignment (include/svo/visual_odometry.hpp: DescriptorIndex::match_rows, pair_rows, align, align_params) on a
real GPU: tests/cpp/align_facade_test.cpp, compiled with g++ -Wall -Werror, on the 1024-pair scene of tests/align_cases.py with 60 %
outliers — match_rows against match byte for byte, the pairs, the inliers and the transform against the numpy reference (written
into the program's input), the round trip through transform_points, and a refusal."""
import subprocess

import numpy as np
import pytest

import align_cases as ac
from test_align_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    n, share, H, sigma = 1024, 0.6, 512, 0.005
    case, want = ac.motion_scene(n, share, sigma), ac.motion_reference(n, share, H, sigma)
    assert want["success"] and want["n_pairs"] == n and want["margin_final"] > 0.1
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([2 * n, *case["src"], *case["dst"], n, H, 3], np.int32).tobytes())
        f.write(np.float32(ac.INLIER_DIST).tobytes())
        f.write(case["desc"].tobytes()); f.write(case["ids"].astype("<u8").tobytes()); f.write(case["xyz"].tobytes()); f.write(case["tags"].tobytes())
        f.write(want["pair_src"].astype(np.int32).tobytes()); f.write(want["pair_dst"].astype(np.int32).tobytes()); f.write(want["inlier"].tobytes())
        f.write(want["R"].astype(np.float64).tobytes()); f.write(want["t"].astype(np.float64).tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "ALIGN FACADE OK" in out.stdout, out.stdout + out.stderr
