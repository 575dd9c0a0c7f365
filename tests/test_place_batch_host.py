"""tests/cpp/place_batch_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_place_batch.hpp, the rules of the
batched place candidates compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as
tests/test_place_host.py does for the single calls': every refusal, the layouts' sizes at the limits (2^24 bins accepted, 2^24 + 1
refused), and against the numpy reference's vectors (written into the program's input) the table of (id, camera) pairs — the lists
of tests/place_batch_cases.py inserted in three orders with a sequential stand-in for the compare-and-swap, colliding ids among
them — with the one sweep over 20 011 rows behind it, and rule 3 over a row of votes against the reference and the single pick.
And the facade round trip (tests/cpp/place_batch_facade_test.cpp) compiles and links with g++; tests/test_gpu_place_batch_facade.py
runs it."""
import os
import subprocess

import numpy as np

import place_batch_cases as pbc
import place_batch_ref as pbr
import place_cases as pc
import place_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
KIND = "interleaved"


def write_vectors(path):
    c = pc.vote_scene(KIND)
    rows, span = (101, 19_990), (3, 45)
    cases = [pbc.mixed_lists(KIND), pbc.shared_lists(KIND), pbc.colliding_lists(KIND), pbc.small_lists(KIND, 9), (np.zeros(0, np.uint64),) * 3]
    with open(path, "wb") as f:
        f.write(np.array([len(c["ids"]), *rows, *span, len(cases), len(pc.PICK_CASES)], np.int32).tobytes())
        f.write(c["ids"].astype("<u8").tobytes()); f.write(c["tags"].astype("<i4").tobytes())
        shared = pr.tag_votes(c["ids"], c["tags"], [], rows, span)[1:]
        assert shared[0].sum() > 0
        for a in shared:
            f.write(a.astype("<i4").tobytes())
        for lists in cases:
            want = pbr.tag_votes_batch(c["ids"], c["tags"], lists, rows, span)
            assert all(np.array_equal(a, b) for a, b in zip(want[1:], shared))
            begin = pbc.offsets(lists)
            f.write(np.array([len(lists), begin[-1]], np.int32).tobytes()); f.write(begin.astype("<i4").tobytes())
            f.write(np.concatenate(lists).astype("<u8").tobytes())
            f.write(np.array([len(np.unique(m)) for m in lists], np.int32).tobytes())
            f.write(want[0].astype("<i4").tobytes())
        for _, votes, tag_lo, min_votes, separation, max_places, _ in pc.PICK_CASES:
            v = np.array(votes, np.int32)
            n_rows, first = v + 2, np.arange(len(v), dtype=np.int32) * 100
            end = first + 50
            _, pl = pr.pick(v, n_rows, first, end, tag_lo, min_votes, separation, max_places)
            f.write(np.array([len(v), tag_lo, min_votes, separation, max_places, len(pl)], np.int32).tobytes())
            for a in (v, n_rows, first, end):
                f.write(a.astype("<i4").tobytes())
            f.write(pl.tobytes())


def test_place_batch_rules_under_sanitizers(tmp_path):
    exe, vec = str(tmp_path / "place_batch_host"), str(tmp_path / "vectors.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "place_batch_host.cpp"), "-o", exe])
    write_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "PLACE BATCH HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "place_batch_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "place_batch_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
