"""The C++ facade's index maintenance (include/svo/visual_odometry.hpp: DescriptorIndex::retire, transform_points) on a real GPU:
tests/cpp/desc_retire_test.cpp, compiled with g++ -Wall -Werror, on a 60-row case of tests/desc_retire_ref.py's generator — the
facade, the C entry and the reference's kept_before and counts (written into the program's input) agree."""
import subprocess

import numpy as np
import pytest

import desc_retire_ref as ref
from test_desc_retire_host import build_facade_test
from test_desc_retire_ref import some_ids

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    m, window = 60, (1, 6)
    case = ref.index_case(m, seed=60, points=False)                       # every row has a point: the facade's add_points takes tags >= 0
    drop = some_ids(case)
    keep, kept_before = ref.retire(case["ids"], case["tags"], (2, m - 3), tag_window=window, drop_ids=drop, latest_per_id=True)
    T = np.array([[0, -1, 0, 2.5], [1, 0, 0, -1], [0, 0, 1.5, 0.25], [0, 0, 0, 1]], np.float64)
    _, moved, skipped = ref.transform(case["xyz"][keep], case["tags"][keep], T, tag_window=window)
    assert 4 <= keep.sum() < m and moved >= 1
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([m, len(drop), window[0], window[1]], np.int32).tobytes())
        f.write(case["desc"].tobytes()); f.write(case["ids"].astype("<u8").tobytes()); f.write(case["xyz"].astype("<f4").tobytes())
        f.write(case["tags"].astype("<i4").tobytes()); f.write(drop.astype("<u8").tobytes()); f.write(kept_before.astype("<i4").tobytes())
        f.write(T.tobytes()); f.write(np.array([moved, skipped], np.int32).tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DESC RETIRE OK" in out.stdout, out.stdout + out.stderr
