"""The C++ facade's batched insertion (include/svo/visual_odometry.hpp: DescriptorIndex::add_obs, add_frames, insert_stats) on a
real GPU: tests/cpp/insert_facade_test.cpp, compiled with g++ -Wall -Werror, on nine entries of 0 to 513 rows with transforms, tags
and id offsets onto an index that holds three rows — the rows read back, first_row and n_added against the numpy reference (written
into the program's input), the statistics, the plain call on an index with points, and five refusals."""
import subprocess

import numpy as np
import pytest

import insert_ref as ir
from test_insert_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    sizes = [40, 0, 513, 1, 64, 257, 0, 65, 300]
    entries = [ir.make_entry(r, ir.flag_pattern("random", r, 60 + b), 9 * b + 2, id0=500 * b) for b, r in enumerate(sizes)]
    n = len(entries)
    base = np.arange(n, dtype=np.uint64) << np.uint64(48)
    T = [ir.pose(20 + b) for b in range(n)]
    tags = list(range(3, 3 + n))
    want = ir.insert(entries, ir.OBS_INLIER, base, True, T, tags, size=3)
    assert 300 < len(want["ids"]) < sum(sizes)
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([n, ir.OBS_INLIER, sum(sizes), len(want["ids"])], np.int32).tobytes()); f.write(begin.tobytes())
        f.write(np.concatenate([o for o, _ in entries]).tobytes()); f.write(np.concatenate([d for _, d in entries]).tobytes())
        f.write(base.astype("<u8").tobytes()); f.write(np.array(tags, np.int32).tobytes()); f.write(np.array(T, np.float64).tobytes())
        f.write(want["desc"].tobytes()); f.write(want["ids"].astype("<u8").tobytes()); f.write(want["xyz"].tobytes()); f.write(want["tags"].tobytes())
        f.write(want["first_row"].tobytes()); f.write(want["n_added"].tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "INSERT FACADE OK" in out.stdout, out.stdout + out.stderr
