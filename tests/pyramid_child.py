"""Run in a fresh process with SVO_INGEST_AHEAD=0 (test_gpu_pyramids.py::test_many_sequences_without_build_ahead): the
many-sequence cases given as JSON on the command line, through test_gpu_pyramids.run_case — the switch is read once per process."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from stereo_visual_odometry_amd import api  # noqa: E402
import test_gpu_pyramids as t  # noqa: E402


def main():
    assert os.environ.get("SVO_INGEST_AHEAD") == "0", "run with SVO_INGEST_AHEAD=0"
    cases = [(c[0], tuple(c[1]), c[2], c[3], c[4], c[5], c[6]) for c in json.loads(sys.argv[1])]
    for c in cases:
        t.run_case(api, c)
        print("ok", t.case_id(c), flush=True)
    print("pyramid child ok: %d cases" % len(cases))


if __name__ == "__main__":
    main()
