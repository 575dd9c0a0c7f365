"""tests/cpp/place_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_place.hpp, the rules of the place
candidates compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as
tests/test_fuse_host.py does for the fusion's: every refusal of a call, the scratch's and the LDS's sizes, and against the numpy
reference's vectors (written into the program's input) the hash on 2 000 ids, the set on the planted 4096-entry list (ids 0 and
2^64 - 1, a repeated id, colliding ids, ids absent from the rows) inserted in three orders with rule 2's sweep over 70 000 rows
behind it, and rule 3 on the hand-made histograms with the key list in both orders.  And the facade round trip
(tests/cpp/place_facade_test.cpp) compiles and links with g++; tests/test_gpu_place_facade.py runs it."""
import os
import subprocess

import numpy as np

import align_ref as aref
import place_cases as pc
import place_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def write_vectors(path):
    c = pc.vote_scene("runs")
    lst = pc.id_list("runs", 4096)
    slots = pc.table_slots(len(lst))
    rows, span = (1_001, 69_000), (3, 400)
    want = pr.tag_votes(c["ids"], c["tags"], lst, rows, span)
    assert want[0].sum() > 0 and (want[1] == 0).any() and (c["tags"][rows[0]:rows[1]] > span[1]).any()
    u = c["universe"][:2000]
    slot = np.array([aref.mix64(int(v)) & (slots - 1) for v in u], np.uint32)
    with open(path, "wb") as f:
        f.write(np.array([len(lst), len(c["ids"]), *rows, *span, slots, len(np.unique(lst)), len(u), len(pc.PICK_CASES)], np.int32).tobytes())
        f.write(lst.astype("<u8").tobytes()); f.write(c["ids"].astype("<u8").tobytes()); f.write(c["tags"].astype("<i4").tobytes())
        for a in want:
            f.write(a.astype("<i4").tobytes())
        f.write(u.astype("<u8").tobytes()); f.write(slot.tobytes())
        for _, votes, tag_lo, min_votes, separation, max_places, _ in pc.PICK_CASES:
            v = np.array(votes, np.int32)
            n_rows, first = v + 2, np.arange(len(v), dtype=np.int32) * 100
            end = first + 50
            _, pl = pr.pick(v, n_rows, first, end, tag_lo, min_votes, separation, max_places)
            f.write(np.array([len(v), tag_lo, min_votes, separation, max_places, len(pl)], np.int32).tobytes())
            for a in (v, n_rows, first, end):
                f.write(a.astype("<i4").tobytes())
            f.write(pl.tobytes())


def test_place_rules_under_sanitizers(tmp_path):
    exe, vec = str(tmp_path / "place_host"), str(tmp_path / "vectors.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "place_host.cpp"), "-o", exe])
    write_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "PLACE HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "place_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "place_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
