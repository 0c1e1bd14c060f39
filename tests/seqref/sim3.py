"""Sequential reference of Sim3Solver (src/Sim3Solver.cc) over the project's tables.

Plain loops over np.float32 / np.float64 scalars, written from the reference text and the conventions of DESIGN.md
section 3: a cv::Mat product (and a product with an added or subtracted matrix, which OpenCV folds into one gemm)
accumulates in fp64 and rounds once; Mat::dot is a double; sums of .at<float>() values are float sums even where the
result lands in a double variable (N11 .. N44, :251-260); everything else is float, one rounding per operation.  Stated
choices: the centroid divides by 3.0f; the eigenvector of the largest eigenvalue comes from a two-sided cyclic Jacobi
method in fp32 (jacobi_eig4); the rotation is built from the normalised quaternion without the angle-axis detour.

The rand() stream of the reference is not part of its defined behaviour: the draws are caller data, draws[it][k] in
[0, N-1-k], and sample() replays the list handling of :163-177 literally.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64

RETURNED, CONTINUE, NO_MORE, TOO_FEW = range(4)
MATCH_POINTS, MATCH_SLOTS = 0, 1
POINT_PRESENT = 1
# Jacobi: a pair is skipped when |a_pq| <= JACOBI_EPS * ||N||_F (the Frobenius norm of the matrix as it comes in, summed in
# float in row-major order); the method stops after a sweep without a rotation or after JACOBI_SWEEPS sweeps.
JACOBI_SWEEPS = 10
JACOBI_EPS = f32(2.0) * np.finfo(np.float32).eps


def iteration_limit(N, prob, min_inliers, max_its):
    """SetRansacParameters (:114-138).  0 where N < min_inliers: iterate never runs then (:146)."""
    if N < min_inliers:
        return 0
    if N == min_inliers:
        return 1
    epsilon = float(f32(f32(min_inliers) / f32(N)))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = f64(math.log(1.0 - prob)) / f64(math.log(1.0 - math.pow(epsilon, 3)))
    d = np.ceil(d)
    if not d >= 1:
        return 1
    return int(min(d, max_its))


def _row_dot(T, r, X):
    d = (f64(T[r][0]) * f64(X[0]) + f64(T[r][1]) * f64(X[1])) + f64(T[r][2]) * f64(X[2])
    return f32(d + f64(T[r][3]))


def _to_image(X, cam):
    """FromCameraToImage (:405-423) / the tail of Project (:397-401)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = f32(f32(1.0) / X[2])
        x, y = f32(X[0] * invz), f32(X[1] * invz)
        return f32(f32(cam["fx"] * x) + cam["cx"]), f32(f32(cam["fy"] * y) + cam["cy"])


def max_error(sigma2):
    """mvnMaxError* is a vector<size_t> (include/Sim3Solver.h:78-79): 9.210 * sigma2 in double, truncated."""
    return int(9.210 * float(f32(sigma2)))


def index_in_key_frame(T, p, row):
    """MapPoint::GetIndexInKeyFrame: the first entry of the point's list that names the row, or -1."""
    for o in range(int(T["obs_start"][p]), int(T["obs_start"][p + 1])):
        if int(T["obs_kf"][o]) == row:
            return int(T["obs_idx"][o])
    return -1


def make_cam(fx, fy, cx, cy):
    return {k: f32(v) for k, v in dict(fx=fx, fy=fy, cx=cx, cy=cy).items()}


def setup(T, cur, kf, matched12, match_form, cam, level_sigma2, prob=0.99, min_inliers=20, max_its=300):
    """The constructor (:37-112) and SetRansacParameters for the current row `cur` and the candidate row `kf`.
    T: slot_point [rows, cap], n [rows], obs_start / obs_kf / obs_idx, flags, world [pcap, 3], Tcw [rows, 12], kps [rows, cap]
    (KP_DTYPE).  matched12 [n[cur]]: point indices (MATCH_POINTS) or key-point slots of `kf` (MATCH_SLOTS).
    Returns the solver: x1, x2 [N, 3], p1, p2 [N, 2], max_err1, max_err2 [N], slot1 [N], n_corr, n1, limit, state [2]."""
    n1 = int(T["n"][cur])
    T1, T2 = np.asarray(T["Tcw"][cur], f32).reshape(3, 4), np.asarray(T["Tcw"][kf], f32).reshape(3, 4)
    S = {k: [] for k in ("x1", "x2", "p1", "p2", "max_err1", "max_err2", "slot1")}
    for i1 in range(n1):
        m = int(matched12[i1])
        if m < 0:
            continue
        p2 = int(T["slot_point"][kf][m]) if match_form == MATCH_SLOTS else m
        if p2 < 0:
            continue
        p1 = int(T["slot_point"][cur][i1])
        if p1 < 0:
            continue
        if not (T["flags"][p1] & POINT_PRESENT) or not (T["flags"][p2] & POINT_PRESENT):
            continue
        idx1, idx2 = index_in_key_frame(T, p1, cur), index_in_key_frame(T, p2, kf)
        if idx1 < 0 or idx2 < 0:
            continue
        S["max_err1"].append(max_error(level_sigma2[int(T["kps"][cur][idx1]["octave"])]))
        S["max_err2"].append(max_error(level_sigma2[int(T["kps"][kf][idx2]["octave"])]))
        S["slot1"].append(i1)
        X1 = [_row_dot(T1, r, T["world"][p1]) for r in range(3)]
        X2 = [_row_dot(T2, r, T["world"][p2]) for r in range(3)]
        S["x1"].append(X1)
        S["x2"].append(X2)
        S["p1"].append(_to_image(X1, cam))
        S["p2"].append(_to_image(X2, cam))
    N = len(S["slot1"])
    out = {"x1": np.array(S["x1"], f32).reshape(N, 3), "x2": np.array(S["x2"], f32).reshape(N, 3),
           "p1": np.array(S["p1"], f32).reshape(N, 2), "p2": np.array(S["p2"], f32).reshape(N, 2),
           "max_err1": np.array(S["max_err1"], np.uint32), "max_err2": np.array(S["max_err2"], np.uint32),
           "slot1": np.array(S["slot1"], np.int32), "n_corr": N, "n1": n1,
           "limit": iteration_limit(N, prob, min_inliers, max_its), "state": [0, 0]}
    return out


def sample(N, draw):
    """:163-177: three indices out of the list of all indices, each taken out by moving the last entry into its place."""
    avail = list(range(N))
    idx = []
    for k in range(3):
        randi = int(draw[k])
        idx.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return idx


def jacobi_eig4(A):
    """Eigenvector of the largest eigenvalue of the symmetric 4x4 float matrix A: two-sided cyclic Jacobi in fp32, pairs
    (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), the rotation formulas of jacobi_null4 (seqref/triangulate.py) on (a_pp, a_qq, a_pq).
    A rotation updates the two columns, then the two rows, then stores exact zeros at (p,q) and (q,p).  Returns (the column
    of V under the first maximum of the diagonal, sweeps run)."""
    a = [[f32(A[r][c]) for c in range(4)] for r in range(4)]
    v = [[f32(1.0 if r == c else 0.0) for c in range(4)] for r in range(4)]
    two, half = f32(2.0), f32(0.5)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        fro = f32(0.0)
        for r in range(4):
            for c in range(4):
                fro = f32(fro + f32(a[r][c] * a[r][c]))
        thresh = f32(JACOBI_EPS * np.sqrt(fro))
        sweeps = 0
        for sweep in range(JACOBI_SWEEPS):
            sweeps = sweep + 1
            changed = False
            for p in range(3):
                for q in range(p + 1, 4):
                    gamma = a[p][q]
                    if not abs(gamma) > thresh:
                        continue
                    changed = True
                    p2, bt = f32(gamma * two), f32(a[p][p] - a[q][q])
                    g = np.sqrt(f32(f32(p2 * p2) + f32(bt * bt)))
                    if bt < 0:
                        delta = f32(f32(g - bt) * half)
                        sn = np.sqrt(f32(delta / g))
                        cs = f32(p2 / f32(f32(g * sn) * two))
                    else:
                        cs = np.sqrt(f32(f32(g + bt) / f32(g * two)))
                        sn = f32(p2 / f32(f32(g * cs) * two))
                    for r in range(4):
                        ap, aq, vp, vq = a[r][p], a[r][q], v[r][p], v[r][q]
                        a[r][p] = f32(f32(cs * ap) + f32(sn * aq))
                        a[r][q] = f32(f32(cs * aq) - f32(sn * ap))
                        v[r][p] = f32(f32(cs * vp) + f32(sn * vq))
                        v[r][q] = f32(f32(cs * vq) - f32(sn * vp))
                    for c in range(4):
                        ap, aq = a[p][c], a[q][c]
                        a[p][c] = f32(f32(cs * ap) + f32(sn * aq))
                        a[q][c] = f32(f32(cs * aq) - f32(sn * ap))
                    a[p][q] = a[q][p] = f32(0.0)
            if not changed:
                break
    best = 0
    for c in range(1, 4):
        if a[c][c] > a[best][best]:
            best = c
    return [v[r][best] for r in range(4)], sweeps


def horn_n(P1, P2):
    """Steps 1-3 of ComputeSim3 (:231-265).  P[k] = point k (a column of the 3x3).  Returns O1, O2, Pr1, Pr2, N (4x4)."""
    three = f32(3.0)
    O1 = [f32(f32(f32(P1[0][r] + P1[1][r]) + P1[2][r]) / three) for r in range(3)]
    O2 = [f32(f32(f32(P2[0][r] + P2[1][r]) + P2[2][r]) / three) for r in range(3)]
    Pr1 = [[f32(P1[k][r] - O1[r]) for r in range(3)] for k in range(3)]
    Pr2 = [[f32(P2[k][r] - O2[r]) for r in range(3)] for k in range(3)]
    M = [[f32((f64(Pr2[0][r]) * f64(Pr1[0][c]) + f64(Pr2[1][r]) * f64(Pr1[1][c])) + f64(Pr2[2][r]) * f64(Pr1[2][c]))
          for c in range(3)] for r in range(3)]
    N11 = f32(f32(M[0][0] + M[1][1]) + M[2][2])
    N12 = f32(M[1][2] - M[2][1])
    N13 = f32(M[2][0] - M[0][2])
    N14 = f32(M[0][1] - M[1][0])
    N22 = f32(f32(M[0][0] - M[1][1]) - M[2][2])
    N23 = f32(M[0][1] + M[1][0])
    N24 = f32(M[2][0] + M[0][2])
    N33 = f32(f32(-M[0][0] + M[1][1]) - M[2][2])
    N34 = f32(M[1][2] + M[2][1])
    N44 = f32(f32(-M[0][0] - M[1][1]) + M[2][2])
    N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    return O1, O2, Pr1, Pr2, N


def rotation_of(q):
    """The rotation of the quaternion (w, x, y, z), normalised first; the same for q and -q."""
    w, x, y, z = q
    one, two = f32(1.0), f32(2.0)
    nrm = np.sqrt(f32(f32(f32(f32(w * w) + f32(x * x)) + f32(y * y)) + f32(z * z)))
    w, x, y, z = f32(w / nrm), f32(x / nrm), f32(y / nrm), f32(z / nrm)
    xx, yy, zz = f32(x * x), f32(y * y), f32(z * z)
    xy, xz, yz = f32(x * y), f32(x * z), f32(y * z)
    wx, wy, wz = f32(w * x), f32(w * y), f32(w * z)
    return [[f32(one - f32(two * f32(yy + zz))), f32(two * f32(xy - wz)), f32(two * f32(xz + wy))],
            [f32(two * f32(xy + wz)), f32(one - f32(two * f32(xx + zz))), f32(two * f32(yz - wx))],
            [f32(two * f32(xz - wy)), f32(two * f32(yz + wx)), f32(one - f32(two * f32(xx + yy)))]]


def _dot3d(a, b):
    return (f64(a[0]) * f64(b[0]) + f64(a[1]) * f64(b[1])) + f64(a[2]) * f64(b[2])


def finish_sim3(O1, O2, Pr1, Pr2, R, fix_scale):
    """Steps 5-8 (:286-336) from the rotation on.  Returns s, t12, T12 [3][4], T21 [3][4]."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        P3 = [[f32(_dot3d(R[r], Pr2[k])) for r in range(3)] for k in range(3)]
        if fix_scale:
            s = f32(1.0)
        else:
            nom, den = f64(0.0), f64(0.0)
            for r in range(3):
                for k in range(3):
                    nom = nom + f64(Pr1[k][r]) * f64(P3[k][r])
                    den = den + f64(f32(P3[k][r] * P3[k][r]))
            s = f32(nom / den)
        t = [f32(f64(O1[r]) - f64(s) * _dot3d(R[r], O2)) for r in range(3)]
        sR = [[f32(s * R[r][c]) for c in range(3)] for r in range(3)]
        inv = f64(1.0) / f64(s)
        sRinv = [[f32(inv * f64(R[c][r])) for c in range(3)] for r in range(3)]
        tinv = [f32(-_dot3d(sRinv[r], t)) for r in range(3)]
    T12 = [sR[r] + [t[r]] for r in range(3)]
    T21 = [sRinv[r] + [tinv[r]] for r in range(3)]
    return s, t, T12, T21


def compute_sim3(P1, P2, fix_scale, info=None):
    """ComputeSim3 (:226-337).  Returns dict(R [3][3], t [3], s, T12, T21)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        O1, O2, Pr1, Pr2, N = horn_n(P1, P2)
        q, sweeps = jacobi_eig4(N)
        R = rotation_of(q)
    if info is not None:
        info["sweeps"] = sweeps
    s, t, T12, T21 = finish_sim3(O1, O2, Pr1, Pr2, R, fix_scale)
    return {"R": R, "t": t, "s": s, "T12": T12, "T21": T21}


def check_inliers(S, H, cam, errs=None):
    """CheckInliers (:340-364): Project of set 2 into image 1 with T12 and of set 1 into image 2 with T21.  errs (a list)
    receives (err1, err2) per correspondence."""
    inl = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(S["n_corr"]):
            u1, v1 = _to_image([_row_dot(H["T12"], r, S["x2"][i]) for r in range(3)], cam)
            u2, v2 = _to_image([_row_dot(H["T21"], r, S["x1"][i]) for r in range(3)], cam)
            dx1, dy1 = f32(S["p1"][i][0] - u1), f32(S["p1"][i][1] - v1)
            dx2, dy2 = f32(u2 - S["p2"][i][0]), f32(v2 - S["p2"][i][1])
            err1 = f32(f64(dx1) * f64(dx1) + f64(dy1) * f64(dy1))
            err2 = f32(f64(dx2) * f64(dx2) + f64(dy2) * f64(dy2))
            if errs is not None:
                errs.append((err1, err2))
            inl.append(bool(err1 < f32(S["max_err1"][i]) and err2 < f32(S["max_err2"][i])))
    return inl


def iterate(S, draws, n_iterations, min_inliers, fix_scale, cam):
    """iterate (:140-207); draws[it] serves iteration number it.  S["state"] = [mnIterations, mnBestInliers] is advanced.
    Returns (report [8], sim3 [16] or None, inliers [n1] uint8): report = {status, N, limit, iterations after, best inliers
    after, returned iteration or -1, nInliers, 0}; sim3 = R12 (9), t12 (3), s12, 0, 0, 0."""
    N, limit = S["n_corr"], S["limit"]
    inliers = np.zeros(S["n1"], np.uint8)
    if N < min_inliers:
        return np.array([TOO_FEW, N, limit, S["state"][0], S["state"][1], -1, 0, 0], np.int32), None, inliers
    cur = 0
    while S["state"][0] < limit and cur < n_iterations:
        cur += 1
        it = S["state"][0]
        S["state"][0] += 1
        idx = sample(N, draws[it])
        H = compute_sim3([S["x1"][i] for i in idx], [S["x2"][i] for i in idx], fix_scale)
        inl = check_inliers(S, H, cam)
        n_inl = sum(inl)
        if n_inl >= S["state"][1]:
            S["state"][1] = n_inl
            if n_inl > min_inliers:
                for i in range(N):
                    if inl[i]:
                        inliers[S["slot1"][i]] = 1
                sim3 = np.zeros(16, f32)
                sim3[:9] = np.array(H["R"], f32).reshape(9)
                sim3[9:12] = H["t"]
                sim3[12] = H["s"]
                return np.array([RETURNED, N, limit, S["state"][0], n_inl, it, n_inl, 0], np.int32), sim3, inliers
    status = NO_MORE if S["state"][0] >= limit else CONTINUE
    return np.array([status, N, limit, S["state"][0], S["state"][1], -1, 0, 0], np.int32), None, inliers
