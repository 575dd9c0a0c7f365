"""The timing contract of the descriptor index on a real GPU (include/svo.h, "Descriptor index", diagnostics): with timing on,
stats()["last_kernels_ms"] is the device time of the span the last call times — the search kernels after match, the selection kernel
after select and localize, the projection and the guided search after a guided call, the projection after project — and 0 when that
call launched nothing or timing is off.  An index of 300 rows with points, 65 queries (two waves) that are rows of the index seen at
their own projections, so that every search finds candidates."""
import numpy as np
import pytest

from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

N_ROWS, N_QUERIES, RADIUS = 300, 65, 8.0
K = np.array([[400.0, 0, 320], [0, 400, 240], [0, 0, 1]], np.float32)
R, T = np.eye(3), np.zeros(3)


@pytest.fixture(scope="module")
def scene(api):
    rng = np.random.default_rng(26)
    desc = rng.integers(0, 256, (N_ROWS, 32), dtype=np.uint8)
    xyz = np.column_stack([rng.uniform(-3, 3, N_ROWS), rng.uniform(-2, 2, N_ROWS), rng.uniform(4, 10, N_ROWS)]).astype(np.float32)
    ix = api.DescriptorIndex(N_ROWS, points=True)
    ix.add_points(desc, np.arange(N_ROWS, dtype=np.uint64), xyz)
    xy = (xyz[:N_QUERIES, :2] / xyz[:N_QUERIES, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)
    yield dict(ix=ix, query=desc[:N_QUERIES].copy(), xy=xy)
    ix.close()


def calls(s):
    """every timed call of the index, by name"""
    ix, q, xy = s["ix"], s["query"], s["xy"]
    return dict(match=lambda: ix.match(q), select=lambda: ix.select(q, xy), localize=lambda: ix.localize(K, q, xy),
                project=lambda: ix.project(K, R, T), match_guided=lambda: ix.match_guided(K, R, T, RADIUS, q, xy),
                select_guided=lambda: ix.select_guided(K, R, T, RADIUS, q, xy), localize_guided=lambda: ix.localize_guided(K, R, T, RADIUS, q, xy))


def test_every_call_times_its_span_and_nothing_launched_is_zero(scene):
    ix = scene["ix"]
    ix.set_timing(True)
    try:
        for name, call in calls(scene).items():
            call()
            ms = ix.stats()["last_kernels_ms"]
            print(name, ms)
            assert ms > 0, name
        assert len(ix.match(np.zeros((0, 32), np.uint8))) == 0                 # behind a timed call: the figure is reset, not left over
        assert ix.stats()["last_kernels_ms"] == 0
        ix.match(scene["query"])
        assert ix.stats()["last_kernels_ms"] > 0
        assert ix.project(K, R, T, 7, 7).shape == (0, 2)
        assert ix.stats()["last_kernels_ms"] == 0
    finally:
        ix.set_timing(False)


def test_timing_off_is_zero_after_every_call(scene):
    ix = scene["ix"]
    ix.set_timing(True)
    ix.match(scene["query"])
    ix.set_timing(False)
    for name, call in calls(scene).items():
        call()
        assert ix.stats()["last_kernels_ms"] == 0, name
