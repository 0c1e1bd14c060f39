"""Sequential reference of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452) up to `new MapPoint`.

Plain loops over np.float32 / np.float64 scalars, written from src/LocalMapping.cc and src/ORBmatcher.cc and the
arithmetic conventions of DESIGN.md section 3: float products and sums one rounding at a time, double where the
reference's C++ promotes (1.0/z, the chi-square comparisons, cv::norm, Mat::dot), and the two stated choices
(cos(2 atan2(h, d)) = (d^2 - h^2) / (d^2 + h^2) in double; one-sided Jacobi SVD of the 4x4 system in fp32).
The descriptor search itself is not restated here: `create_new_map_points` takes it as a function.
"""
import numpy as np

f32, f64 = np.float32, np.float64

CREATED, NO_MATCH, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(10)
JACOBI_SWEEPS = 8
JACOBI_EPS = f32(2.0) * np.finfo(np.float32).eps


def _dot3(a0, a1, a2, b0, b1, b2):
    return f32(f32(f32(a0 * b0) + f32(a1 * b1)) + f32(a2 * b2))


def _mul3(A, B):
    C = np.zeros((3, 3), f32)
    for r in range(3):
        for c in range(3):
            C[r, c] = _dot3(A[r, 0], A[r, 1], A[r, 2], B[0, c], B[1, c], B[2, c])
    return C


def inv3(M):
    """cv::invert of a 3x3 CV_32F matrix: cofactors and determinant in double, elements rounded to float."""
    m = [[f64(M[r][c]) for c in range(3)] for r in range(3)]
    d = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
         + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    out = np.zeros((3, 3), f32)
    if d == 0.0:
        return out
    d = f64(1.0) / d
    out[0, 0] = f32((m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d)
    out[0, 1] = f32((m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d)
    out[0, 2] = f32((m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d)
    out[1, 0] = f32((m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d)
    out[1, 1] = f32((m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d)
    out[1, 2] = f32((m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d)
    out[2, 0] = f32((m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d)
    out[2, 1] = f32((m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d)
    out[2, 2] = f32((m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d)
    return out


def _pose(T):
    T = np.asarray(T, f32).reshape(3, 4)
    return T[:, :3], T[:, 3]


def camera_centre(T):
    """Ow = -Rcw^T * tcw."""
    R, t = _pose(T)
    return np.array([-_dot3(R[0, c], R[1, c], R[2, c], t[0], t[1], t[2]) for c in range(3)], f32)


def _norm3(x, y, z):
    return np.sqrt((f64(x) * f64(x) + f64(y) * f64(y)) + f64(z) * f64(z))


def baseline_gate(T1, T2, mb=None, median_depth=None):
    """:244-261.  Stereo (median_depth None): baseline < mb.  Monocular: (float)(baseline / median) < 0.01."""
    O1, O2 = camera_centre(T1), camera_centre(T2)
    baseline = f32(_norm3(f32(O2[0] - O1[0]), f32(O2[1] - O1[1]), f32(O2[2] - O1[2])))
    if median_depth is None:
        return bool(baseline < f32(mb))
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(f64(f32(baseline / f32(median_depth))) < 0.01)


def compute_f12(T1, T2, fx, fy, cx, cy):
    """LocalMapping::ComputeF12 (:536-553) with one camera for both key frames."""
    R1, t1 = _pose(T1)
    R2, t2 = _pose(T2)
    R12 = _mul3(R1, R2.T)
    t12 = np.zeros(3, f32)
    for r in range(3):
        t12[r] = f32(_dot3(-R12[r, 0], -R12[r, 1], -R12[r, 2], t2[0], t2[1], t2[2]) + t1[r])
    z = f32(0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], f32)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    return _mul3(_mul3(_mul3(inv3(K.T), tx), R12), inv3(K))


def epipole(T1, T2, fx, fy, cx, cy):
    """Epipole of camera 1 in image 2, src/ORBmatcher.cc:664-670."""
    Cw = camera_centre(T1)
    R2, t2 = _pose(T2)
    C2 = [f32(_dot3(R2[r, 0], R2[r, 1], R2[r, 2], Cw[0], Cw[1], Cw[2]) + t2[r]) for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = f32(f32(1.0) / C2[2])
        ex = f32(f32(f32(f32(fx) * C2[0]) * invz) + f32(cx))
        ey = f32(f32(f32(f32(fy) * C2[1]) * invz) + f32(cy))
    return ex, ey


def _dot4(a, b):
    return f32(f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2])) + f32(a[3] * b[3]))


def jacobi_null4(A, max_sweeps=None):
    """Right singular vector of the smallest singular value of the 4x4 float matrix A: one-sided (Hestenes) Jacobi on
    the columns, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a pair is rotated unless |a_p.a_q| <= 2 eps sqrt(|a_p|^2
    |a_q|^2); stops after a sweep without a rotation or after JACOBI_SWEEPS (max_sweeps, where given: the tests use it to
    show that the cap does not change x3D).  Returns (x[4], sweeps)."""
    a = [[f32(A[r][c]) for r in range(4)] for c in range(4)]   # a[c] = column c
    v = [[f32(1.0 if r == c else 0.0) for r in range(4)] for c in range(4)]
    two, half = f32(2.0), f32(0.5)
    sweeps = 0
    for sweep in range(JACOBI_SWEEPS if max_sweeps is None else max_sweeps):
        sweeps = sweep + 1
        changed = False
        for p in range(3):
            for q in range(p + 1, 4):
                alpha, beta, gamma = _dot4(a[p], a[p]), _dot4(a[q], a[q]), _dot4(a[p], a[q])
                if abs(gamma) <= f32(JACOBI_EPS * np.sqrt(f32(alpha * beta))):
                    continue
                changed = True
                p2, bt = f32(gamma * two), f32(alpha - beta)
                g = np.sqrt(f32(f32(p2 * p2) + f32(bt * bt)))
                if bt < 0:
                    delta = f32(f32(g - bt) * half)
                    sn = np.sqrt(f32(delta / g))
                    cs = f32(p2 / f32(f32(g * sn) * two))
                else:
                    cs = np.sqrt(f32(f32(g + bt) / f32(g * two)))
                    sn = f32(p2 / f32(f32(g * cs) * two))
                for r in range(4):
                    ap, aq, vp, vq = a[p][r], a[q][r], v[p][r], v[q][r]
                    a[p][r] = f32(f32(cs * ap) + f32(sn * aq))
                    a[q][r] = f32(f32(cs * aq) - f32(sn * ap))
                    v[p][r] = f32(f32(cs * vp) + f32(sn * vq))
                    v[q][r] = f32(f32(cs * vq) - f32(sn * vp))
        if not changed:
            break
    best, w = 0, _dot4(a[0], a[0])
    for c in range(1, 4):
        wc = _dot4(a[c], a[c])
        if wc < w:
            best, w = c, wc
    return np.array(v[best], f32), sweeps


def _row_dot(T, r, X):
    T = np.asarray(T, f32).reshape(3, 4)
    d = (f64(T[r, 0]) * f64(X[0]) + f64(T[r, 1]) * f64(X[1])) + f64(T[r, 2]) * f64(X[2])
    return f32(d + f64(T[r, 3]))


def _reproj_fails(cam, T, X, z, stereo, ku, kv, kur, sigma2):
    x, y = _row_dot(T, 0, X), _row_dot(T, 1, X)
    invz = f32(f64(1.0) / f64(z))
    u = f32(f32(f32(cam["fx"] * x) * invz) + cam["cx"])
    v = f32(f32(f32(cam["fy"] * y) * invz) + cam["cy"])
    ex, ey = f32(u - ku), f32(v - kv)
    e2 = f32(f32(ex * ex) + f32(ey * ey))
    if not stereo:
        return bool(f64(e2) > 5.991 * f64(sigma2))
    er = f32(f32(u - f32(cam["mbf"] * invz)) - kur)
    e2 = f32(e2 + f32(er * er))
    return bool(f64(e2) > 7.8 * f64(sigma2))


def cos_parallax_stereo(mb, depth):
    h, d = f64(f32(f32(mb) * f32(0.5))), f64(f32(depth))
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32((d * d - h * h) / (d * d + h * h))


def unproject_stereo(T, u, v, z, cam):
    """KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631) on the given keypoint coordinates."""
    R, _ = _pose(T)
    Ow = camera_centre(T)
    invfx, invfy = f32(f32(1.0) / cam["fx"]), f32(f32(1.0) / cam["fy"])
    x = f32(f32(f32(u - cam["cx"]) * z) * invfx)
    y = f32(f32(f32(v - cam["cy"]) * z) * invfy)
    return np.array([f32(f32(f32(f32(R[0, r] * x) + f32(R[1, r] * y)) + f32(R[2, r] * z)) + Ow[r]) for r in range(3)], f32)


def make_cam(fx, fy, cx, cy, mbf, mb):
    return {k: f32(v) for k, v in dict(fx=fx, fy=fy, cx=cx, cy=cy, mbf=mbf, mb=mb).items()}


def triangulation_matrix(T1, T2, kp1, kp2, cam):
    """The 4x4 A of :322-326 (float)."""
    T1, T2 = np.asarray(T1, f32).reshape(3, 4), np.asarray(T2, f32).reshape(3, 4)
    invfx, invfy = f32(f32(1.0) / cam["fx"]), f32(f32(1.0) / cam["fy"])
    xn1 = (f32(f32(f32(kp1[0]) - cam["cx"]) * invfx), f32(f32(f32(kp1[1]) - cam["cy"]) * invfy))
    xn2 = (f32(f32(f32(kp2[0]) - cam["cx"]) * invfx), f32(f32(f32(kp2[1]) - cam["cy"]) * invfy))
    A = np.zeros((4, 4), f32)
    for c in range(4):
        A[0, c] = f32(f32(xn1[0] * T1[2, c]) - T1[0, c])
        A[1, c] = f32(f32(xn1[1] * T1[2, c]) - T1[1, c])
        A[2, c] = f32(f32(xn2[0] * T2[2, c]) - T2[0, c])
        A[3, c] = f32(f32(xn2[1] * T2[2, c]) - T2[1, c])
    return A, xn1, xn2


def triangulate_pair(T1, T2, kp1, kp2, cam, level_sigma2, scale_factors, info=None):
    """Loop body :286-431 for one matched pair.  kp = (x, y, octave, u_right, depth) with u_right < 0 = monocular.
    Returns (status, x3D[3]); x3D is zero where no point was computed.  info (a dict) receives linear = the linear
    triangulation :322-337 was the branch taken."""
    T1, T2 = np.asarray(T1, f32).reshape(3, 4), np.asarray(T2, f32).reshape(3, 4)
    X0 = np.zeros(3, f32)
    x1, y1, o1, ur1, z1d = f32(kp1[0]), f32(kp1[1]), int(kp1[2]), f32(kp1[3]), f32(kp1[4])
    x2, y2, o2, ur2, z2d = f32(kp2[0]), f32(kp2[1]), int(kp2[2]), f32(kp2[3]), f32(kp2[4])
    s1, s2 = bool(ur1 >= 0), bool(ur2 >= 0)
    A, xn1, xn2 = triangulation_matrix(T1, T2, (x1, y1), (x2, y2), cam)
    one = f32(1.0)
    r1 = [_dot3(T1[0, r], T1[1, r], T1[2, r], xn1[0], xn1[1], one) for r in range(3)]
    r2 = [_dot3(T2[0, r], T2[1, r], T2[2, r], xn2[0], xn2[1], one) for r in range(3)]
    dd = (f64(r1[0]) * f64(r2[0]) + f64(r1[1]) * f64(r2[1])) + f64(r1[2]) * f64(r2[2])
    cos_rays = f32(dd / (_norm3(*r1) * _norm3(*r2)))
    cs1 = cs2 = f32(cos_rays + one)
    if s1:
        cs1 = cos_parallax_stereo(cam["mb"], z1d)
    elif s2:
        cs2 = cos_parallax_stereo(cam["mb"], z2d)
    cs = cs2 if cs2 < cs1 else cs1
    linear = bool(cos_rays < cs and cos_rays > 0 and (s1 or s2 or f64(cos_rays) < 0.9998))
    if info is not None:
        info["linear"] = linear
    if linear:
        x, _ = jacobi_null4(A)
        if x[3] == 0:
            return W_ZERO, X0
        X = np.array([f32(x[r] / x[3]) for r in range(3)], f32)
    elif s1 and cs1 < cs2:
        X = unproject_stereo(T1, x1, y1, z1d, cam)
    elif s2 and cs2 < cs1:
        X = unproject_stereo(T2, x2, y2, z2d, cam)
    else:
        return LOW_PARALLAX, X0
    z1, z2 = _row_dot(T1, 2, X), _row_dot(T2, 2, X)
    if z1 <= 0:
        return BEHIND_1, X
    if z2 <= 0:
        return BEHIND_2, X
    if _reproj_fails(cam, T1, X, z1, s1, x1, y1, ur1, f32(level_sigma2[o1])):
        return REPROJ_1, X
    if _reproj_fails(cam, T2, X, z2, s2, x2, y2, ur2, f32(level_sigma2[o2])):
        return REPROJ_2, X
    O1, O2 = camera_centre(T1), camera_centre(T2)
    d1 = f32(_norm3(f32(X[0] - O1[0]), f32(X[1] - O1[1]), f32(X[2] - O1[2])))
    d2 = f32(_norm3(f32(X[0] - O2[0]), f32(X[1] - O2[1]), f32(X[2] - O2[2])))
    if d1 == 0 or d2 == 0:
        return ZERO_DIST, X
    sf = np.asarray(scale_factors, f32)
    ratio_factor = f32(f32(1.5) * sf[1 if len(sf) > 1 else 0])
    ratio_dist, ratio_oct = f32(d2 / d1), f32(sf[o1] / sf[o2])
    if f32(ratio_dist * ratio_factor) < ratio_oct or ratio_dist > f32(ratio_oct * ratio_factor):
        return SCALE, X
    return CREATED, X


def create_new_map_points(frames, cur, kf_index, cam, level_sigma2, scale_factors, search, median_depth=None):
    """The per-row arrays of the batched call.  frames[r] = dict(keys (KP_DTYPE), n, u_right / depth (arrays or None),
    T [12]); search(k, f, F12, ex, ey) -> matches12[n_cur] of that pair (the caller's SearchForTriangulation).
    Returns dict of f12 [K,3,3], epipole [K,2], skipped [K], matches12 [K,n], nmatches [K], status [K,n], x3d [K,n,3]."""
    K, C = len(kf_index), frames[cur]
    n = C["n"]
    out = {"f12": np.zeros((K, 3, 3), f32), "epipole": np.zeros((K, 2), f32), "skipped": np.zeros(K, np.uint8),
           "matches12": np.full((K, n), -1, np.int32), "nmatches": np.zeros(K, np.int32),
           "status": np.full((K, n), NO_MATCH, np.uint8), "x3d": np.zeros((K, n, 3), f32)}
    mono = C["u_right"] is None
    for k, f in enumerate(kf_index):
        F = frames[f]
        if baseline_gate(C["T"], F["T"], cam["mb"], None if not mono else median_depth[k]):
            out["skipped"][k] = 1
            continue
        F12 = compute_f12(C["T"], F["T"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        ex, ey = epipole(C["T"], F["T"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        out["f12"][k], out["epipole"][k] = F12, (ex, ey)
        m12 = np.asarray(search(k, f, F12, ex, ey), np.int32)
        out["matches12"][k] = m12[:n]
        out["nmatches"][k] = int((m12[:n] >= 0).sum())
        for i in range(n):
            j = int(m12[i])
            if j < 0:
                continue
            k1, k2 = C["keys"][i], F["keys"][j]
            p1 = (k1["x"], k1["y"], k1["octave"], -1.0 if mono else C["u_right"][i], 0.0 if mono else C["depth"][i])
            p2 = (k2["x"], k2["y"], k2["octave"], -1.0 if mono else F["u_right"][j], 0.0 if mono else F["depth"][j])
            st, X = triangulate_pair(C["T"], F["T"], p1, p2, cam, level_sigma2, scale_factors)
            out["status"][k, i], out["x3d"][k, i] = st, X
    return out


def apply_rows(rows, has_point_cur, has_point_kf, kf_index):
    """The row-application rule of INTEGRATION.md section 3: walk the rows in neighbour order and keep a CREATED entry
    unless its current key point was given a point by an earlier row or (repeated targets) its neighbour slot was.  The
    marks of a row are set when the row is finished: within one row two current key points may match the same neighbour
    slot, and the reference, which never sets vbMatched2, creates both points (:434 onwards).
    Returns the kept (k, i, j) triples; has_point arrays are updated in place."""
    kept = []
    for k, f in enumerate(kf_index):
        row = []
        for i in range(rows["status"].shape[1]):
            j = int(rows["matches12"][k, i])
            if j < 0 or rows["status"][k, i] != CREATED or has_point_cur[i] or has_point_kf[f][j]:
                continue
            row.append((k, i, j))
        for _, i, j in row:
            has_point_cur[i] = 1
            has_point_kf[f][j] = 1
        kept += row
    return kept
