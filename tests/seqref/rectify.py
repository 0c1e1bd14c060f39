"""Sequential restatement of the stereo rectification of Examples/Stereo/stereo_euroc.cc:63-98, 136-137:
cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F, M1, M2) and cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) on 8-bit
grey images, written from the published OpenCV 2.4 - 3.3 algorithms.  Pure Python / numpy; imports neither the package
under test nor the oracle.

Python floats and numpy float64 are IEEE doubles with one rounding per operation and no fused multiply-add, so the
operation ORDER below is the whole specification.  Along a row the homogeneous coordinates are advanced by repeated
addition; np.add.accumulate performs exactly that recurrence (each element = previous + step, in order), and everything
after it is elementwise, so a row is evaluated as a vector with the same result as a per-pixel loop
(init_undistort_rectify_map_scalar is that loop, kept for the cross-check in tests/test_rectify_cpu.py).

Stated choices (unpinned like the other OpenCV restatements):
  * A = P[0:3,0:3] * R, each element summed left to right over k = 0, 1, 2;
  * iR = adj(A) * (1 / det A), det expanded along the first row (OpenCV uses an LU decomposition);
  * the bilinear table row for fx = fy = 0 is (32768, 0, 0, 0).
"""
import numpy as np

INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS            # 32
INTER_REMAP_COEF_BITS = 15
INTER_REMAP_COEF_SCALE = 1 << INTER_REMAP_COEF_BITS
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def _inverse_of_product(P, R):
    P = [[float(P[i][j]) for j in range(3)] for i in range(3)]
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)] if R is not None else [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    A = [[P[i][0] * R[0][j] + P[i][1] * R[1][j] + P[i][2] * R[2][j] for j in range(3)] for i in range(3)]
    (a, b, c), (d, e, f), (g, h, k) = A
    c00, c01, c02 = e * k - f * h, d * k - f * g, d * h - e * g
    det = a * c00 - b * c01 + c * c02
    i = 1.0 / det
    return [c00 * i, (c * h - b * k) * i, (b * f - c * e) * i,
            (f * g - d * k) * i, (a * k - c * g) * i, (c * d - a * f) * i,
            c02 * i, (b * g - a * h) * i, (a * e - b * d) * i]


def _coefficients(D):
    D = [float(v) for v in np.asarray(D, np.float64).reshape(-1)]
    assert len(D) in (4, 5, 8)
    D = D + [0.0] * (8 - len(D)) if len(D) != 5 else D + [0.0, 0.0, 0.0]
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    return k1, k2, p1, p2, k3, k4, k5, k6


def init_undistort_rectify_map(K, D, R, P, size):
    """K 3x3, D 4 / 5 / 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]), R 3x3 or None, P 3x3 or 3x4, size = (cols, rows).
    Returns (map1, map2) float32 [rows, cols]."""
    cols, rows = int(size[0]), int(size[1])
    K = np.asarray(K, np.float64).reshape(3, 3)
    ir = _inverse_of_product(np.asarray(P, np.float64)[:3, :3], None if R is None else np.asarray(R, np.float64).reshape(3, 3))
    fx, fy, u0, v0 = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    k1, k2, p1, p2, k3, k4, k5, k6 = _coefficients(D)
    map1 = np.zeros((rows, cols), np.float32)
    map2 = np.zeros((rows, cols), np.float32)
    step = np.empty(cols, np.float64)
    for i in range(rows):
        acc = []
        for first, inc in ((i * ir[1] + ir[2], ir[0]), (i * ir[4] + ir[5], ir[3]), (i * ir[7] + ir[8], ir[6])):
            step[:] = inc
            step[0] = first
            acc.append(np.add.accumulate(step))          # [first, first + inc, (first + inc) + inc, ...]
        _x, _y, _w = acc
        w = 1.0 / _w
        x = _x * w
        y = _y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
        v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
        map1[i] = u.astype(np.float32)
        map2[i] = v.astype(np.float32)
    return map1, map2


def init_undistort_rectify_map_scalar(K, D, R, P, size):
    """The same, pixel by pixel with Python floats: the loop the vector form above stands for."""
    cols, rows = int(size[0]), int(size[1])
    K = np.asarray(K, np.float64).reshape(3, 3)
    ir = _inverse_of_product(np.asarray(P, np.float64)[:3, :3], None if R is None else np.asarray(R, np.float64).reshape(3, 3))
    fx, fy, u0, v0 = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    k1, k2, p1, p2, k3, k4, k5, k6 = _coefficients(D)
    map1 = np.zeros((rows, cols), np.float32)
    map2 = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        _x, _y, _w = i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8]
        for j in range(cols):
            w = 1.0 / _w
            x, y = _x * w, _y * w
            x2, y2 = x * x, y * y
            r2, _2xy = x2 + y2, 2 * x * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            map1[i, j] = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
            map2[i, j] = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
            _x += ir[0]
            _y += ir[3]
            _w += ir[6]
    return map1, map2


def bilinear_table():
    """The fixed-point INTER_LINEAR table of initInterTab2D: row (fy * 32 + fx) = weights of the taps (x, y), (x+1, y),
    (x, y+1), (x+1, y+1); (1 - fx/32 | fx/32) * (1 - fy/32 | fy/32) * 32768, which is an integer for every entry."""
    tab = np.zeros((INTER_TAB_SIZE * INTER_TAB_SIZE, 4), np.int64)
    for fy in range(INTER_TAB_SIZE):
        for fx in range(INTER_TAB_SIZE):
            wx = (INTER_TAB_SIZE - fx, fx)
            wy = (INTER_TAB_SIZE - fy, fy)
            row = [wy[a] * wx[b] * (INTER_REMAP_COEF_SCALE // (INTER_TAB_SIZE * INTER_TAB_SIZE)) for a in (0, 1) for b in (0, 1)]
            assert sum(row) == INTER_REMAP_COEF_SCALE
            tab[fy * INTER_TAB_SIZE + fx] = row
    return tab


def cv_round_fixed(m):
    """cvRound(m * 32) per map entry: round half to even, saturated to int; returns (int64 values, NaN mask)."""
    m = np.asarray(m, np.float32)
    nan = np.isnan(m)
    v = np.rint(np.where(nan, np.float32(0), m).astype(np.float64) * float(INTER_TAB_SIZE))
    v = np.clip(v, float(INT_MIN), float(INT_MAX))
    return v.astype(np.int64), nan


def tap_classes(map1, map2, src_shape):
    """Per destination pixel, the number of its four taps that lie inside the source (0..4)."""
    srows, scols = src_shape
    sx, nx = cv_round_fixed(map1)
    sy, ny = cv_round_fixed(map2)
    x0, y0 = sx >> INTER_BITS, sy >> INTER_BITS
    cnt = np.zeros(x0.shape, np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            cnt += ((x0 + dx >= 0) & (x0 + dx < scols) & (y0 + dy >= 0) & (y0 + dy < srows)).astype(np.int64)
    cnt[nx | ny] = 0
    return cnt


def remap_linear(img, map1, map2, table=None):
    """cv::remap(img, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) for a uint8 grey image and CV_32F maps:
        sx = cvRound(map1 * 32), sy = cvRound(map2 * 32); taps at (sx >> 5, sy >> 5) + {0, 1}^2, 0 outside the source;
        dst = min(255, (sum taps * table[(sy & 31) * 32 + (sx & 31)] + (1 << 14)) >> 15).
    Integer arithmetic throughout, so evaluating the destination pixels as arrays equals the per-pixel loop."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    tab = bilinear_table() if table is None else np.asarray(table, np.int64).reshape(INTER_TAB_SIZE * INTER_TAB_SIZE, 4)
    srows, scols = img.shape
    sx, nx = cv_round_fixed(map1)
    sy, ny = cv_round_fixed(map2)
    x0, y0 = sx >> INTER_BITS, sy >> INTER_BITS
    w = tab[(sy & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (sx & (INTER_TAB_SIZE - 1))]      # [rows, cols, 4]
    acc = np.full(x0.shape, 1 << (INTER_REMAP_COEF_BITS - 1), np.int64)
    wide = img.astype(np.int64)
    k = 0
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            inside = (x >= 0) & (x < scols) & (y >= 0) & (y < srows) & ~nx & ~ny
            tap = np.where(inside, wide[np.clip(y, 0, srows - 1), np.clip(x, 0, scols - 1)], 0)
            acc += tap * w[..., k]
            k += 1
    return np.minimum(acc >> INTER_REMAP_COEF_BITS, 255).astype(np.uint8)


def remap_linear_scalar(img, map1, map2, table=None):
    """The per-pixel loop remap_linear stands for (used on small images by the CPU tests)."""
    img = np.asarray(img)
    tab = (bilinear_table() if table is None else np.asarray(table, np.int64).reshape(-1, 4)).tolist()
    srows, scols = img.shape
    px = img.tolist()
    rows, cols = np.asarray(map1).shape
    sxs, nx = cv_round_fixed(map1)
    sys_, ny = cv_round_fixed(map2)
    out = np.zeros((rows, cols), np.uint8)
    for i in range(rows):
        for j in range(cols):
            if nx[i, j] or ny[i, j]:
                continue
            sx, sy = int(sxs[i, j]), int(sys_[i, j])
            x0, y0 = sx >> 5, sy >> 5
            w = tab[(sy & 31) * 32 + (sx & 31)]
            acc = 1 << 14
            for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                x, y = x0 + dx, y0 + dy
                if 0 <= x < scols and 0 <= y < srows:
                    acc += px[y][x] * w[k]
            out[i, j] = min(255, acc >> 15)
    return out
