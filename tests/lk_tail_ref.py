"""An instrumented copy of the oracle's LK level loop (oracle/orc_lk.c, lk_level) in numpy, for the tests of the kernel's scalar tail
(tests/test_gpu_lk_mineig_band.py, tests/test_gpu_lk_epoch_reach.py).  The oracle reports points, statuses and two totals; these tests
also need what it does not report: per feature the level visits and Newton steps, per visit the rule that ended it, and every integer
search-window origin a track went through.  The copy is only trusted as far as it is checked: `track` is compared by its callers with
the oracle's points bit for bit, with its statuses, and with the oracle's own visit and step totals (orc_lk_counters) on the same input.

Arithmetic follows the C source operation for operation: float32 scalars (numpy rounds every float32 operation once, as the C
compiler does without contraction), exact integers for the window sums, one rounding from the exact sum to float32."""
import numpy as np

import oracle_lib as orc

W_BITS = 14
F = np.float32
FLT_SCALE = F(1.0) / F(1 << 20)
FLT_EPSILON = F(1.1920928955078125e-07)
END_CONVERGED, END_OSCILLATION, END_LIMIT, END_REACH = 0, 1, 2, 3           # how a level visit's Newton loop ended


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    one, sc = F(1.0), F(1 << W_BITS)
    iw00 = int(np.rint((one - a) * (one - b) * sc))
    iw01 = int(np.rint(a * (one - b) * sc))
    iw10 = int(np.rint((one - a) * b * sc))
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _f32_of_int(v):
    return F(float(int(v)))                          # |v| < 2^53: exact as a double, rounded once to float32


class Levels:
    """The levels of an oracle pyramid with the borders the loop reads: REFLECT_101 around the image, constant zero around the
    derivatives (buildOpticalFlowPyramid), each wide enough for any origin in reach."""

    def __init__(self, img, win, max_level):
        p = orc.Pyramid(img, (win, win), max_level)
        self.pyr, self.win, self.pad = p, win, win + 2
        self.n = p.nlevels
        self.size = [(p.p.w[l], p.p.h[l]) for l in range(self.n)]
        self.img = [np.pad(p.level(l).astype(np.int64), self.pad, mode="reflect") for l in range(self.n)]
        self.der = [np.pad(p.deriv(l).astype(np.int64), ((self.pad, self.pad), (self.pad, self.pad), (0, 0))) for l in range(self.n)]

    def box(self, arr, ox, oy, n):
        return arr[oy + self.pad:oy + self.pad + n, ox + self.pad:ox + self.pad + n]


def _bilinear(lv, arr, ox, oy, w, wts, shift):
    b = lv.box(arr, ox, oy, w + 1)
    return _descale(b[:-1, :-1] * wts[0] + b[:-1, 1:] * wts[1] + b[1:, :-1] * wts[2] + b[1:, 1:] * wts[3], shift)


def track(A, B, pts, max_level, max_count=30, epsilon=1e-4, min_eig=1e-3):
    """cv::calcOpticalFlowPyrLK of the points from Levels A to Levels B -> dict: next (n, 2) float32, status (n,) uint8,
    visits / steps (n,) per feature, ends = [(feature, level, END_*)] per level visit that reached the Newton loop,
    origins = [(feature, level, inx, iny)] per epoch test (the out-of-reach ones included)."""
    w = A.win
    half = F(w - 1) * F(0.5)
    top = min(max_level, A.n - 1, B.n - 1)
    max_count = min(max(max_count, 0), 100)
    eps2 = min(max(epsilon, 0.0), 10.0) ** 2
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    nxt = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    visits, steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
    ends, origins = [], []
    den = F(2 * w * w)
    for level in range(top, -1, -1):
        scale = F(1.0 / (1 << level))
        cols, rows = A.size[level]
        for i in range(n):
            ppx, ppy = pts[i, 0] * scale, pts[i, 1] * scale
            if level == top:
                npx, npy = ppx, ppy
            else:
                npx, npy = nxt[i, 0] * F(2.0), nxt[i, 1] * F(2.0)
            nxt[i] = (npx, npy)
            ppx, ppy = ppx - half, ppy - half
            ipx, ipy = int(np.floor(ppx)), int(np.floor(ppy))
            if ipx < -w or ipx >= cols or ipy < -w or ipy >= rows:
                if level == 0:
                    status[i] = 0
                continue
            wts = _weights(ppx - F(ipx), ppy - F(ipy))
            I = _bilinear(A, A.img[level], ipx, ipy, w, wts, W_BITS - 5)
            d = A.der[level]
            Ix = _bilinear(A, d[:, :, 0], ipx, ipy, w, wts, W_BITS)
            Iy = _bilinear(A, d[:, :, 1], ipx, ipy, w, wts, W_BITS)
            A11 = _f32_of_int((Ix * Ix).sum()) * FLT_SCALE
            A12 = _f32_of_int((Ix * Iy).sum()) * FLT_SCALE
            A22 = _f32_of_int((Iy * Iy).sum()) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            min_e = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4.0) * A12 * A12)) / den
            if float(min_e) < min_eig or D < FLT_EPSILON:
                if level == 0:
                    status[i] = 0
                continue
            D = F(1.0) / D
            visits[i] += 1
            npx, npy = npx - half, npy - half
            pdx = pdy = F(0.0)
            end = END_LIMIT
            for j in range(max_count):
                inx, iny = int(np.floor(npx)), int(np.floor(npy))
                origins.append((i, level, inx, iny))
                if inx < -w or inx >= cols or iny < -w or iny >= rows:
                    if level == 0:
                        status[i] = 0
                    end = END_REACH
                    break
                steps[i] += 1
                wj = _weights(npx - F(inx), npy - F(iny))
                diff = _bilinear(B, B.img[level], inx, iny, w, wj, W_BITS - 5) - I
                b1 = _f32_of_int((diff * Ix).sum()) * FLT_SCALE
                b2 = _f32_of_int((diff * Iy).sum()) * FLT_SCALE
                dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                npx, npy = npx + dx, npy + dy
                nxt[i] = (npx + half, npy + half)
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                    end = END_CONVERGED
                    break
                if j > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                    nxt[i] = (nxt[i, 0] - dx * F(0.5), nxt[i, 1] - dy * F(0.5))
                    end = END_OSCILLATION
                    break
                pdx, pdy = dx, dy
            ends.append((i, level, end))
            if status[i] and level == 0:
                ix, iy = int(np.floor(nxt[i, 0] - half)), int(np.floor(nxt[i, 1] - half))
                if ix < -w or ix >= cols or iy < -w or iy >= rows:
                    status[i] = 0
    return dict(next=nxt, status=status, visits=visits, steps=steps, ends=ends, origins=origins)


def oracle_track_counted(A, B, pts, max_level, **kw):
    """the oracle itself on the same input -> (next, status, level visits that reached the loop, Newton steps)"""
    c = (orc.C.c_longlong * 4).in_dll(orc.lib(), "orc_lk_counters")
    before = list(c)
    out, st = orc.lk_track(A.pyr, B.pyr, pts, (A.win, A.win), max_level, **kw)
    return out, st, c[0] - before[0], c[1] - before[1]


def same_as_oracle(A, B, pts, max_level, **kw):
    """track() on the input, checked against the oracle as far as the oracle reports; returns track()'s dict"""
    r = track(A, B, pts, max_level, **kw)
    ok = dict(max_count=kw.get("max_count", 30), epsilon=kw.get("epsilon", 1e-4), min_eig=kw.get("min_eig", 1e-3))
    out, st, nv, ns = oracle_track_counted(A, B, pts, max_level, **ok)
    assert np.array_equal(st, r["status"]), np.flatnonzero(st != r["status"])
    assert np.array_equal(out.view(np.uint32), r["next"].view(np.uint32)), np.flatnonzero((out.view(np.uint32) != r["next"].view(np.uint32)).any(1))
    assert (nv, ns) == (int(r["visits"].sum()), int(r["steps"].sum())), (nv, ns, int(r["visits"].sum()), int(r["steps"].sum()))
    return r
