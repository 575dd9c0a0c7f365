"""Run in a fresh process with SVO_LK_DERIV=0 or SVO_INGEST_AHEAD=0 (test_gpu_deriv_planes.py::test_switched_off_in_the_environment):
either switch is read once per process, and under either a many-sequence grey context keeps no derivative planes and says so."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from stereo_visual_odometry_amd import _lib, api  # noqa: E402
from gpu_kit import projections  # noqa: E402
from test_gpu_pyramids import make_stream  # noqa: E402


def main():
    var = sys.argv[1]
    assert os.environ.get(var) == "0", "run with %s=0" % var
    w, h, B = 134, 70, 9
    vo = api.BatchVisualOdometry(w, h, B, api.default_config(win_w=5, win_h=5, max_level=3, max_translation_norm=2.0))
    vo.initalize_projection_matricies(*projections(w, h))
    L, R = make_stream(w, h, 2, 5)
    buf = np.zeros(1 << 16, np.int16)
    for k in range(2):
        assert not vo.has_derivatives()
        for a in (None, _lib.ptr(buf)):
            assert _lib.lib.svo_get_derivatives(vo._h, 0, 0, 0, 1, a, a, buf.size, None, None, None, None) == _lib.SVO_ERR_STATE
            assert "no planes" in _lib.lib.svo_last_error().decode()
        vo.stereo_callback_batch([L[k]] * B, [R[k]] * B)
        ahead = bool(vo.last_frame_path() & _lib.PATH_INGEST_AHEAD)
        assert ahead == (var != "SVO_INGEST_AHEAD"), (var, vo.last_frame_path())
    assert vo.pyramid(0, "t1", 0, 1)[0].any()                          # the pyramids are there; only the planes are not
    vo.close()
    print("deriv planes child ok: no planes under %s=0" % var)


if __name__ == "__main__":
    main()
