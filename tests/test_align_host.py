"""tests/cpp/align_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_align.hpp, the rules of the map alignment
compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as
tests/test_reloc_batch_host.py does for the batch's arithmetic: every refusal of a call, the spans' overlap where they touch and
where they share one row, the sampler for every n_pairs 3 .. 4096 at a spread of h (three distinct numbers below n_pairs; the
64-draw fallback forced at n_pairs = 3), Horn's closed form and the residual, and the staging's sizes at n = 4096, H = 1024.  And the
facade round trip (tests/cpp/align_facade_test.cpp) compiles and links with g++; tests/test_gpu_align_facade.py runs it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_align_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "align_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "align_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALIGN HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "align_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "align_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
