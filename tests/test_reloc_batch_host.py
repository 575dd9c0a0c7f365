"""tests/cpp/reloc_batch_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_reloc_batch.hpp, the arithmetic of
the batched relocalisation compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as
tests/test_desc_retire_host.py does for the maintenance calls' rules: every refusal of a call's offsets, and at the maximal shape
(1024 cameras of 1024 queries, 1 << 24 rows, chunk rows 1 .. 1 << 24) and at small ones that every planned launch stays within 65 535
blocks along y and z, that its partial states fit the budget and that the launches cover every (query, row) exactly once.  And the
facade round trip (tests/cpp/reloc_batch_facade_test.cpp) compiles and links with g++; tests/test_gpu_reloc_batch_facade.py runs it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_batch_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "reloc_batch_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "reloc_batch_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "RELOC BATCH HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "reloc_batch_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "reloc_batch_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
