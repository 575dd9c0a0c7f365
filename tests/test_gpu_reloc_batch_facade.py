"""The C++ facade's batched relocalisation (include/svo/visual_odometry.hpp: DescriptorIndex::localize_batch, batch_order) on a real
GPU: tests/cpp/reloc_batch_facade_test.cpp, compiled with g++ -Wall -Werror, on nine cameras of tests/reloc_batch_cases.py — per
camera the facade's single call's record byte for byte and its candidate lists, guided and unguided; the first camera's candidates
are the numpy reference's (written into the program's input)."""
import subprocess

import numpy as np
import pytest

import reloc_batch_cases as bc
import reloc_batch_ref as bref
from test_reloc_batch_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    rows = dict(bc.index_rows())
    rows["tags"] = np.maximum(rows["tags"], 0).astype(np.int32)           # the program adds every row with its point (the origin where the case has none)
    names, K, guides, queries, xys = bc.small(9)
    want = bref.select_batch(rows, [bc.cameras()[names[0]]], True)[0]
    assert names[0] == "repeated" and len(want["query"]) == 160
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(names), len(rows["desc"]), len(want["query"])], np.int32).tobytes())
        f.write(rows["desc"].tobytes()); f.write(rows["ids"].astype("<u8").tobytes()); f.write(rows["xyz"].tobytes())
        f.write(rows["tags"].tobytes())
        for b in range(len(names)):
            f.write(np.int32(len(queries[b])).tobytes()); f.write(K[b].astype(np.float32).tobytes())
            f.write(guides[b][0].astype(np.float64).tobytes()); f.write(guides[b][1].astype(np.float64).tobytes()); f.write(np.float32(guides[b][2]).tobytes())
            f.write(queries[b].tobytes()); f.write(xys[b].tobytes())
        f.write(want["query"].astype(np.int32).tobytes()); f.write(want["row"].astype(np.int32).tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RELOC BATCH FACADE OK" in out.stdout, out.stdout + out.stderr
