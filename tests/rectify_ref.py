"""numpy restatement of the rectification arithmetic of include/svo.h, written independently of the HIP code:
the map generator (cv::initUndistortRectifyMap's scalar loop, CV_16SC2 output) and the bilinear fixed-point remap
(cv::remap, INTER_LINEAR, BORDER_CONSTANT 0).  Every f64 operation is element-wise and in the loop's own order — the
incremental column walk is a column-by-column row-vector addition, nothing is reduced — so it must equal the library bit
for bit."""
import numpy as np


def inv3(A):
    """Matx's fast 3x3 inverse: adjugate / determinant, OpenCV's operand order."""
    a = lambda r, c: A[r, c]
    d = (a(0, 0) * (a(1, 1) * a(2, 2) - a(2, 1) * a(1, 2)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(2, 0) * a(1, 2))
         + a(0, 2) * (a(1, 0) * a(2, 1) - a(2, 0) * a(1, 1)))
    d = 1.0 / d
    return np.array([
        (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) * d, (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) * d, (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) * d,
        (a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)) * d, (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) * d, (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) * d,
        (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)) * d, (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) * d, (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) * d])


def matmul3(A, B):
    """Matx product: ((a0 b0 + a1 b1) + a2 b2) per element."""
    C = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            C[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j]
    return C


def cv_round(v):
    """cvRound on an array: round half to even; outside int32 (or NaN): INT_MIN."""
    r = np.rint(v)
    ok = (r >= -2147483648.0) & (r <= 2147483647.0)
    return np.where(ok, np.nan_to_num(r), -2147483648.0).astype(np.int64)


def init_rectify_map(K, D, R, P, w, h):
    K = np.asarray(K, np.float64).reshape(3, 3)
    k = np.zeros(8)
    D = np.asarray(D if D is not None else [], np.float64).reshape(-1)
    k[:len(D)] = D
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    P33 = K if P is None else np.asarray(P, np.float64).reshape(3, 4)[:, :3]
    ir = inv3(matmul3(P33, R))
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    i = np.arange(h, dtype=np.float64)
    _x = i * ir[1] + ir[2]
    _y = i * ir[4] + ir[5]
    _w = i * ir[7] + ir[8]
    iu = np.zeros((h, w), np.int64); iv = np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        for j in range(w):                               # the column walk: one row-vector add per column
            ww = 1.0 / _w
            x = _x * ww; y = _y * ww
            x2 = x * x; y2 = y * y
            r2 = x2 + y2; _2xy = 2 * x * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
            yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
            u = fx * xd + u0; v = fy * yd + v0
            iu[:, j] = cv_round(u * 32); iv[:, j] = cv_round(v * 32)
            _x = _x + ir[0]; _y = _y + ir[3]; _w = _w + ir[6]
    map1 = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], -1)
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def remap(raw, map1, map2):
    """cv::remap(raw, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) in 5-bit fixed point -> the map's size, raw's channels."""
    raw = np.asarray(raw, np.uint8)
    img = raw if raw.ndim == 3 else raw[:, :, None]
    rh, rw, cn = img.shape
    x0 = map1[..., 0].astype(np.int64); y0 = map1[..., 1].astype(np.int64)
    f = map2.astype(np.int64) & 1023
    fx = f & 31; fy = f >> 5
    w = [(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy]
    acc = np.zeros(map2.shape + (cn,), np.int64)
    for (dx, dy), wt in zip(((0, 0), (1, 0), (0, 1), (1, 1)), w):
        xs, ys = x0 + dx, y0 + dy
        inside = (xs >= 0) & (xs < rw) & (ys >= 0) & (ys < rh)
        p = img[np.clip(ys, 0, rh - 1), np.clip(xs, 0, rw - 1)].astype(np.int64) * inside[..., None]
        acc += wt[..., None] * p
    out = ((acc + 512) >> 10).astype(np.uint8)
    return out if raw.ndim == 3 else out[..., 0]


# calibrations written out as numbers (ROS camera_info form): the KITTI-00 rectified pair and a ZED-sized raw pair whose P
# carries the ZED numbers of synthetic.py (fx 684.37, cx 689.89, cy 406.87, bf -82.124) with plumb_bob / rational_polynomial
# distortion and small rectifying rotations
KITTI00_LEFT = dict(width=1241, height=376,
                    K=[[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]],
                    D=[0.0, 0.0, 0.0, 0.0, 0.0],
                    R=np.eye(3).tolist(),
                    P=[[718.856, 0.0, 607.1928, 0.0], [0.0, 718.856, 185.2157, 0.0], [0.0, 0.0, 1.0, 0.0]])
KITTI00_RIGHT = dict(KITTI00_LEFT, P=[[718.856, 0.0, 607.1928, -386.1448], [0.0, 718.856, 185.2157, 0.0], [0.0, 0.0, 1.0, 0.0]])
ZED_LEFT = dict(width=1920, height=1080,
                K=[[699.5, 0.0, 652.7], [0.0, 699.1, 402.3], [0.0, 0.0, 1.0]],
                D=[-0.1711, 0.0257, 0.00031, -0.00042, 0.0],
                R=[[0.99998, 0.00211, -0.00562], [-0.00213, 0.99999, -0.00302], [0.00561, 0.00303, 0.99998]],
                P=[[684.37, 0.0, 689.89, 0.0], [0.0, 684.37, 406.87, 0.0], [0.0, 0.0, 1.0, 0.0]])
ZED_RIGHT = dict(width=1920, height=1080,
                 K=[[701.2, 0.0, 648.1], [0.0, 700.9, 409.8], [0.0, 0.0, 1.0]],
                 D=[0.41, -0.12, 0.0004, -0.0003, 0.02, 0.75, -0.05, 0.08],
                 R=[[0.99995, -0.00442, 0.00893], [0.00440, 0.99999, 0.00221], [-0.00894, -0.00217, 0.99996]],
                 P=[[684.37, 0.0, 689.89, -82.124], [0.0, 684.37, 406.87, 0.0], [0.0, 0.0, 1.0, 0.0]])
