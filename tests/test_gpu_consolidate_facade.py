"""The C++ facade's landmark consolidation (include/svo/visual_odometry.hpp: DescriptorIndex::consolidate_params, consolidate,
read_rows) on a real GPU: tests/cpp/consolidate_facade_test.cpp, compiled with g++ -Wall -Werror, on 900 rows of about 6 views a
landmark with a partial scope and a tag window — read_rows after add_points, the record, kept_before and the rows afterwards
against the numpy reference (written into the program's input), a second call, and five refusals."""
import subprocess

import numpy as np
import pytest

import consolidate_ref as cr
from test_consolidate_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    c = cr.index_case(900, views=6, seed=21, none_every=0)
    rows, window, radius = (50, 850), (1, 6), 0.25
    want = cr.consolidate(c["desc"], c["ids"], c["xyz"], c["tags"], radius, rows, window)
    assert want["result"].n_dropped > 300 and want["result"].n_far_views > 20
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([900, *rows, *window, len(want["ids"]), *want["result"]], np.int32).tobytes()); f.write(np.float32(radius).tobytes())
        f.write(c["desc"].tobytes()); f.write(c["ids"].astype("<u8").tobytes()); f.write(c["xyz"].tobytes()); f.write(c["tags"].tobytes())
        f.write(want["kept_before"].tobytes())
        f.write(want["desc"].tobytes()); f.write(want["ids"].astype("<u8").tobytes()); f.write(want["xyz"].tobytes()); f.write(want["tags"].tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "CONSOLIDATE FACADE OK" in out.stdout, out.stdout + out.stderr
