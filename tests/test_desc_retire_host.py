"""tests/cpp/desc_retire_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_retire.hpp, the rules of the
descriptor index's maintenance calls compiled for the host from the text the kernels run — built with AddressSanitizer and UBSan and
run, as tests/test_desc_match_host.py does for the search's rules (-ffp-contract=off as the library's Makefile has it: the transform
rounds every operation on its own).  And the facade round trip (tests/cpp/desc_retire_test.cpp) compiles and links with g++;
tests/test_gpu_desc_retire_facade.py runs it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_retire_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "desc_retire_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "desc_retire_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "DESC RETIRE HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "desc_retire_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "desc_retire_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
