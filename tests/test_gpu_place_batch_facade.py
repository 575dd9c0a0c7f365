"""The C++ facade's batched place candidates (include/svo/visual_odometry.hpp: DescriptorIndex::places_batch,
places_from_ids_batch, tag_votes_batch) on a real GPU: tests/cpp/place_batch_facade_test.cpp, compiled with g++ -Wall -Werror, on
the planted scene of 12 keyframes of tests/place_cases.py with five cameras — the whole query set, two halves of it, no query at all
and random descriptors — every camera against the numpy reference (written into the program's input) and against the facade's
single calls, a second call, and six refusals."""
import subprocess

import numpy as np
import pytest

import place_batch_ref as pbr
import place_cases as pc
from test_place_batch_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_batch_facade_round_trip_from_gxx(tmp_path):
    c = pc.planted_scene()
    q = c["query"]
    rows, span, min_votes, separation, max_places = (40, 1200), (2, 10), 2, 1, 4
    queries = [q, q[:20], q[20:], q[:0], np.random.default_rng(5).integers(0, 256, (7, 32), dtype=np.uint8)]
    want = pbr.places_batch(queries, c["desc"], c["ids"], c["tags"], rows=rows, tag_span=span, min_votes=min_votes, separation=separation,
                            max_places=max_places)
    assert want[0]["places"]["tag"].tolist() == [5, 7] and [w["n_landmarks"] for w in want] == [40, 20, 20, 0, 0]
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(c["desc"]), len(queries), *rows, *span, min_votes, separation, max_places], np.int32).tobytes())
        f.write(c["desc"].tobytes()); f.write(c["ids"].astype("<u8").tobytes()); f.write(c["xyz"].tobytes()); f.write(c["tags"].tobytes())
        for qb, w in zip(queries, want):
            f.write(np.array([len(qb), w["n_landmarks"], w["n_tags_voted"], w["n_places"]], np.int32).tobytes())
            f.write(np.ascontiguousarray(qb).tobytes()); f.write(w["places"].tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "PLACE BATCH FACADE OK" in out.stdout, out.stdout + out.stderr
