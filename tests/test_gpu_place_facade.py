"""The C++ facade's place candidates (include/svo/visual_odometry.hpp: DescriptorIndex::place_params, places, places_from_ids,
tag_votes) on a real GPU: tests/cpp/place_facade_test.cpp, compiled with g++ -Wall -Werror, on the planted scene of 12 keyframes
of tests/place_cases.py — the counts, the places and the recognised landmarks against the numpy reference (written into the
program's input), tag_votes' four arrays, places_from_ids with the same landmarks, a second call, and five refusals."""
import subprocess

import numpy as np
import pytest

import place_cases as pc
import place_ref as pr
from test_place_host import build_facade_test

pytestmark = pytest.mark.gpu


def test_facade_round_trip_from_gxx(tmp_path):
    c = pc.planted_scene()
    rows, span, min_votes, separation, max_places = (40, 1200), (2, 10), 2, 1, 4
    want = pr.places(c["query"], c["desc"], c["ids"], c["tags"], rows=rows, tag_span=span, min_votes=min_votes, separation=separation, max_places=max_places)
    votes = pr.tag_votes(c["ids"], c["tags"], c["ids"][want["cand_row"]], rows, span)
    assert want["places"]["tag"].tolist() == [5, 7] and want["n_landmarks"] == 40
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(c["desc"]), len(c["query"]), *rows, *span, min_votes, separation, max_places, want["n_landmarks"], want["n_tags_voted"],
                          want["n_places"]], np.int32).tobytes())
        f.write(c["desc"].tobytes()); f.write(c["ids"].astype("<u8").tobytes()); f.write(c["xyz"].tobytes()); f.write(c["tags"].tobytes())
        f.write(c["query"].tobytes()); f.write(want["places"].tobytes())
        f.write(want["cand_query"].astype(np.int32).tobytes()); f.write(want["cand_row"].astype(np.int32).tobytes())
        for a in votes:
            f.write(a.astype(np.int32).tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "PLACE FACADE OK" in out.stdout, out.stdout + out.stderr
