"""tests/cpp/fuse_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_fuse.hpp, the rules of the landmark fusion
compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as tests/test_align_host.py
does for the alignment's: every refusal of a call, the scratch's sizes, and against the numpy reference's vectors (written into the
program's input) the gate on 12 000 point pairs at three radii, the hash on 2 000 ids, and the table and the sweep on the planted
4096-entry list (a chain, a repeated `from`, from == to, colliding `from` values) over 50 000 ids, inserted in three orders.  And the
facade round trip (tests/cpp/fuse_facade_test.cpp) compiles and links with g++; tests/test_gpu_fuse_facade.py runs it."""
import os
import subprocess

import numpy as np

import align_ref as aref
import fuse_cases as fc
import fuse_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def write_vectors(path):
    c = fc.near_scene(65, 1000)
    (s0, _), (d0, _) = c["src"], c["dst"]
    src, dst = np.arange(s0, s0 + 20), np.arange(d0, d0 + 200)
    gate = []
    for radius in fc.RADII:
        adm = fr.gate(c["xyz"], c["tags"], src, dst, radius)
        for i, s in enumerate(src):
            for j, r in enumerate(dst):
                gate.append(np.concatenate([c["xyz"][r], c["xyz"][s], [np.float32(radius)]]).astype(np.float32).tobytes() +
                            np.array([c["tags"][r], c["tags"][s], int(adm[i, j])], np.int32).tobytes())
    assert any(g[-4:] == b"\x01\x00\x00\x00" for g in gate) and any(g[-4:] == b"\x00\x00\x00\x00" for g in gate)
    frm, to = fc.relabel_lists(4096)
    slots = fc.table_slots(len(frm))
    u = fc.relabel_index()["universe"][:2000]
    slot = np.array([aref.mix64(int(v)) & (slots - 1) for v in u], np.uint32)
    ids = fc.relabel_index()["ids"][:50_000]
    lo, hi = 1000, 45_000
    want, changed = fr.relabel(ids, frm, to, (lo, hi))
    assert 0 < changed < hi - lo
    with open(path, "wb") as f:
        f.write(np.array([len(gate), len(u), len(frm), len(ids), lo, hi, changed, slots], np.int32).tobytes())
        f.write(b"".join(gate))
        f.write(u.astype("<u8").tobytes()); f.write(slot.tobytes())
        f.write(frm.astype("<u8").tobytes()); f.write(to.astype("<u8").tobytes())
        f.write(ids.astype("<u8").tobytes()); f.write(want.astype("<u8").tobytes())


def test_fuse_rules_under_sanitizers(tmp_path):
    exe, vec = str(tmp_path / "fuse_host"), str(tmp_path / "vectors.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "fuse_host.cpp"), "-o", exe])
    write_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "FUSE HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "fuse_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "fuse_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
