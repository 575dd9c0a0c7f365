"""tests/cpp/desc_match_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_match.hpp, the integer rules of the
descriptor index's search compiled for the host from the text the kernels run, and the capacity rule of the index's growable buffers
(match_grow_capacity: the sequence from empty, the clamp at the budget, a need above it, no growth for a smaller need, and
need <= cap < max(2 * need, first + 1)) — built with AddressSanitizer and UBSan and run, as tests/test_descriptor_host.py does for
the descriptor rules.  And the facade round trip (tests/cpp/desc_index_test.cpp) compiles and
links with g++; tests/test_gpu_desc_index_facade.py runs it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_match_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "desc_match_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "desc_match_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "DESC MATCH HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "desc_index_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "desc_index_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
