"""No-GPU checks of the ragged / continuous batching entry points (svo_process_batch_masked, svo_submit_batch_masked,
svo_reset_sequence): declared in include/svo.h, exported by libsvo_hip.so, bound in _lib.EXPORTS, and a NULL context is an
argument error rather than a crash."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svo_process_batch_masked", "svo_submit_batch_masked", "svo_reset_sequence")


def test_declared_exported_and_bound():
    from stereo_visual_odometry_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "svo.h does not declare %s" % s
        assert hasattr(_lib.lib, s), "libsvo_hip.so does not export %s" % s
        assert s in _lib.EXPORTS


def test_idle_reason_documented():
    txt = open(os.path.join(ROOT, "include", "svo.h")).read()
    assert re.search(r"5 idle", txt)


def test_null_context_is_an_argument_error():
    from stereo_visual_odometry_amd import _lib
    lib = _lib.lib
    P = (C.c_float * 12)()
    assert lib.svo_reset_sequence(None, -1, None, None) == _lib.SVO_ERR_ARG
    assert lib.svo_reset_sequence(None, 0, P, P) == _lib.SVO_ERR_ARG
    act = (C.c_uint8 * 4)(1, 0, 1, 0)
    ptrs = (C.c_void_p * 4)()
    assert lib.svo_submit_batch_masked(None, ptrs, ptrs, 1241, act) == _lib.SVO_ERR_ARG
    assert lib.svo_submit_batch_masked(None, None, None, 1241, None) == _lib.SVO_ERR_ARG
    assert lib.svo_process_batch_masked(None, ptrs, ptrs, 1241, 1, act, None, None, None) == _lib.SVO_ERR_ARG
    assert lib.svo_process_batch_masked(None, None, None, 1241, 0, None, None, None, None) == _lib.SVO_ERR_ARG
