"""The C++ facade's descriptor index (include/svo/visual_odometry.hpp: DescriptorIndex) on a real GPU: tests/cpp/desc_index_test.cpp,
compiled with g++ -Wall -Werror, on the 65 x 27 slice of tests/test_desc_match_ref.py's tie set — the facade, the C entry and the
reference's rows (written into the program's input) agree byte for byte."""
import subprocess

import numpy as np
import pytest

import desc_match_ref as mref
from test_desc_match_host import build_facade_test
from test_desc_match_ref import shared_case

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    q, d, ids = shared_case()
    q = q[:65]
    want = mref.match(q, d, ids)
    assert want.dtype.itemsize == 32 and len(d) == 27
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(q), len(d)], np.int32).tobytes())
        f.write(q.tobytes()); f.write(d.tobytes()); f.write(ids.astype("<u8").tobytes()); f.write(want.tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DESC INDEX OK" in out.stdout, out.stdout + out.stderr
