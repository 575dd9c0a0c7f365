"""The C++ facade's landmark fusion (include/svo/visual_odometry.hpp: DescriptorIndex::fuse_params, match_near, pair_near, relabel,
fuse) on a real GPU: tests/cpp/fuse_facade_test.cpp, compiled with g++ -Wall -Werror, on the 1500-on-3000-row merge scene of
tests/fuse_cases.py — match_near's rows, the dry run's pairs, fuse's four counts, its pairs and the ids afterwards against the numpy
reference (written into the program's input), a second call that finds everything fused, a relabel, and a refusal."""
import subprocess

import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref as fr
from test_fuse_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    c = fc.merge_scene(1500, 3000)
    tags = np.where(c["tags"] < 0, 0, c["tags"]).astype(np.int32)       # the facade's add_points gives every row a point
    rows = fr.match_near(c["desc"], c["ids"], c["xyz"], tags, c["src"], c["dst"], c["radius"])
    want = fr.fuse(c["desc"], c["ids"], c["xyz"], tags, c["src"], c["dst"], c["radius"])
    assert want["n_fused"] > 0 and want["n_same"] > 0
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(c["desc"]), *c["src"], *c["dst"], want["n_pairs"], want["n_same"], want["n_fused"], want["n_rows_relabelled"]], np.int32).tobytes())
        f.write(np.float32(c["radius"]).tobytes())
        f.write(c["desc"].tobytes()); f.write(c["ids"].astype("<u8").tobytes()); f.write(c["xyz"].tobytes()); f.write(tags.tobytes())
        f.write(rows.tobytes())
        f.write(want["pair_src"].astype(np.int32).tobytes()); f.write(want["pair_dst"].astype(np.int32).tobytes())
        f.write(want["ids"].astype("<u8").tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "FUSE FACADE OK" in out.stdout, out.stdout + out.stderr
