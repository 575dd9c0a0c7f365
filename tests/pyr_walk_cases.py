"""The case matrix of tests/test_gpu_pyr_walk.py: the register-walking pyrDown (k_pyr_walk) and the row-wise border kernel
(k_pad_pyramid; svo_kernels_img.hip, svo_pyr_walk.hpp) at the sizes their work plan makes special.  tests/test_pyr_walk_cases.py
guards the matrix on the CPU and runs the walk itself, compiled for the host, against tests/pyramid_ref.py.

The plan's constants, restated:
- WALK_V: consecutive outputs of a destination row a thread owns (one 8-byte store); its vectors start at x = WALK_V k - (pad & 7).
- WALK_ROWS: destination rows a thread walks down (the walk length) at the levels >= 2; WALK_ROWS_INGEST: at level 1, built from the
  caller's image.
- WALK_SPAN: source bytes of a row a thread needs (five dwords from column 2 x - 2); WALK_LOAD: what a fast vector loads, the six
  aligned dwords around them (up to three bytes before the span).  A vector whose loads could leave the row at either end takes the
  edge form: dwords from inside the row, folded into place.

A case has the shape of tests/test_gpu_pyramids.py's: (route, (w, h), win, max_level, n_seq, input, extra) — plain grey contexts of
9 .. 12 sequences in the exact-sums mode, the smallest that take the many-sequence path; input = host | pinned | dev+K (device frames
whose rows are K bytes wider than the image); extra["depth"] = frames kept in flight (three frames are checked after the first
`depth` are in flight).  CASES run the build-ahead route, MANY_CASES the SVO_INGEST_AHEAD=0 route in a child process."""
import pyramid_ref

WALK_V, WALK_ROWS, WALK_ROWS_INGEST, WALK_SPAN, WALK_LOAD = 8, 8, 16, 20, 24


def lk_pad_for(win):
    """The border the library stores around every level (svo_kernels_lk.hip lk_pad_for)."""
    ppl = next(p for p in range(1, win + 1) if win * -(-win // p) <= 64)
    return (-(-win // ppl) * ppl + 5 + 3) & ~3


CASES = [
    ("ahead", (1241, 376), 21, 3, 9, "dev+0", {"depth": 1}),   # the bench image: levels 621x188 311x94 156x47, pad 28
    ("ahead", (129, 97), 5, 5, 12, "host", {}),                # 65x49 33x25 17x13 9x7: k V + 1 twice, rows k R + 1 of both walks, a level narrower than the pad (12)
    ("ahead", (142, 78), 5, 4, 10, "dev+1", {"depth": 2}),     # 71x39 36x20 18x10 (9x5 stops the chain): k V - 1, rows k R - 1
    ("ahead", (100, 207), 5, 5, 9, "dev+3", {"depth": 3}),     # 50x104 25x52 13x26 7x13: rows k R, a level narrower than one vector
    ("ahead", (384, 160), 21, 2, 10, "host", {}),              # 192x80 96x40: k V at both levels, pad 28 (vectors start at x = -4)
    ("ahead", (383, 159), 15, 3, 9, "dev+64", {"depth": 2}),   # k V - 1, an odd height; 192x80 96x40 48x20, pad 24 (vectors start at 0)
    ("ahead", (385, 189), 10, 3, 9, "pinned", {}),             # k V + 1 at both levels, level 1 rows k R - 1 of the ingest walk; 193x95 97x48 49x24, pad 16
    ("ahead", (90, 46), 5, 3, 11, "dev+0", {"depth": 3}),      # 45x23 23x12 12x6: a level no taller than (pad + 1) / 2: the border folds twice
]
MANY_CASES = [
    ("many", (142, 78), 5, 4, 10, "dev+1", {"depth": 2}),
    ("many", (385, 161), 10, 3, 9, "host", {}),
    ("many", (129, 97), 5, 5, 12, "dev+64", {}),
]
# Sizes only the host build of the walk can be given (a level of the library is larger than its window, so it has at least six rows
# and columns): at most two rows, where the five taps fold twice; one pixel; spans that just fit and just do not fit a row.
HOST_ONLY_SIZES = [(9, 2), (37, 2), (5, 1), (1, 1), (2, 2), (3, 5), (19, 9), (20, 9), (21, 9), (22, 3), (29, 9), (30, 9), (35, 17), (36, 16)]
ROW_EXTRA = (0, 1, 3, 64)


def case_id(c):
    route, (w, h), win, ml, B, inp, ex = c
    return "%s-%dx%d-w%d-l%d-B%d-%s%s" % (route, w, h, win, ml, B, inp, "".join("-%s%s" % kv for kv in sorted(ex.items())))


def levels_of(case):
    route, (w, h), win, ml, B, inp, ex = case
    return pyramid_ref.level_sizes(w, h, win, ml)


def vectors(w1, pad):
    """Vectors of a destination row of w1 pixels."""
    return (w1 + (pad & 7) + WALK_V - 1) // WALK_V


def fast_vectors(w, pad):
    """The vectors of a level built from a source row of w bytes whose span lies inside that row."""
    c = pad & 7
    return [v for v in range(vectors((w + 1) // 2, pad)) if 2 * (WALK_V * v - c) - 2 >= 3 and 2 * (WALK_V * v - c) - 2 + WALK_LOAD <= w]
