"""Sequential reference of PnPsolver (src/PnPsolver.cc): the RANSAC state machine and EPnP, written from the reference text.

Plain loops over np.float64 / np.float32 scalars, one rounding per operation, no contraction.  The solver keeps doubles
wherever the reference does (pws, us, alphas, cws, ccs, mRi, mti, fu, fv, uc, vc); CheckInliers mixes float and double as
:308-339 declares its variables.  OpenCV is absent, so three of its routines have stand-ins, stated here and in DESIGN.md
section 3:

  cvSVD of a symmetric matrix (PW0tPW0 3x3, MtM 12x12)   jacobi_eig: two-sided cyclic Jacobi, pairs (p, q) in row-major
      order p < q, at most EIG_SWEEPS sweeps, a pair is skipped unless |a_pq| > EIG_EPS * ||A||_F (norm of the matrix as
      it comes in, summed row-major); a sweep without a rotation ends the method.  Eigenvalues = the diagonal, sorted in
      descending order, equal values keep their index order (the lower index first).  The principal axes of PW0tPW0 get
      a sign (pca_sign): the pose depends on the control points at the noise level, so the choice must be a stated one.
  cvSVD of ABt, cvInvert(CC, CV_SVD), cvSolve(CV_SVD)    svd_cols: one-sided (Hestenes) Jacobi on the columns, pairs in
      row-major order, at most SVD_SWEEPS sweeps, a pair is skipped unless |<p, q>| > SVD_EPS * sqrt(<p, p> <q, q>).
      R = U V^T does not depend on the order or sign of the singular triplets, so none is imposed.  The pseudo-inverse and
      the least-squares solutions drop the columns whose singular value is <= SVD_CUT * the largest one.

Every sum over correspondences (centroids, PW0tPW0, MtM, pc0 / pw0, ABt, the reprojection error) is taken left to right
in the order of the correspondences: the draw order for a four-point sample, the index order for Refine().  MtM adds, per
correspondence, the product of row 2i and then of row 2i + 1 of M, structural zeros included.

The rand() stream is not part of the reference's defined behaviour: draws[it][k] in [0, N-1-k] is caller data.
qr_solve reads an uninitialised X when it meets a zero pivot column (:887-890 return before X is written); here X is
what the previous Gauss-Newton step of the same gauss_newton call left, zeros on the first step.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64

REFINED, BEST, NO_MORE, TOO_FEW = range(4)
MATCH_POINTS, MATCH_SLOTS = 0, 1
POINT_PRESENT = 1
EIG_SWEEPS, EIG_EPS = 15, f64(2.0 ** -53)
SVD_SWEEPS, SVD_EPS, SVD_CUT = 30, f64(2.0 ** -52), f64(6 * 2.0 ** -52)
Z = f64(0.0)


# ---------------------------------------------------------------------------------------------------------------------
# SetRansacParameters (:121-157)
def ransac_parameters(N, prob=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991):
    """(adjusted mRansacMinInliers, adjusted mRansacMaxIts) for N correspondences.  The limit is 0 where N is below the
    adjusted minimum: iterate never runs then (:173)."""
    eps = f32(epsilon)
    n_min = int(f32(f32(N) * eps))                                              # :134, a float product, truncated
    if n_min < min_inliers:
        n_min = min_inliers
    if n_min < min_set:
        n_min = min_set
    if N < n_min:
        return n_min, 0
    q = f32(f32(n_min) / f32(N))
    if eps < q:
        eps = q
    if n_min == N:
        return n_min, 1
    with np.errstate(all="ignore"):
        d = f64(math.log(1.0 - prob)) / f64(math.log(1.0 - math.pow(float(eps), 3)))   # exponent 3, the sample is 4
    d = np.ceil(d)
    if not d >= 1:
        return n_min, 1
    return n_min, int(min(d, max_its))


def setup(kps, matches, match_form, slot_point_row, flags, world, level_sigma2, prob=0.99, min_inliers=10, max_its=300,
          min_set=4, epsilon=0.5, th2=5.991):
    """The constructor (:67-110) and SetRansacParameters.  kps [n] (x, y, octave) = mvKeysUn, matches [n] per slot: point
    indices (MATCH_POINTS) or key-point slots of the candidate row (MATCH_SLOTS, through slot_point_row)."""
    assert min_set == 4
    n = len(kps)
    p2d, p3d, me, ki = [], [], [], []
    for i in range(n):
        m = int(matches[i])
        if m < 0:
            continue
        p = int(slot_point_row[m]) if match_form == MATCH_SLOTS else m
        if p < 0 or not (int(flags[p]) & POINT_PRESENT):
            continue
        p2d.append((f32(kps[i]["x"]), f32(kps[i]["y"])))
        p3d.append(tuple(f32(v) for v in world[p]))
        me.append(f32(f32(level_sigma2[int(kps[i]["octave"])]) * f32(th2)))       # :156, a vector<float>
        ki.append(i)
    N = len(ki)
    n_min, limit = ransac_parameters(N, prob, min_inliers, max_its, min_set, epsilon, th2)
    return dict(p2d=np.array(p2d, f32).reshape(N, 2), p3d=np.array(p3d, f32).reshape(N, 3), max_err=np.array(me, f32),
                kp_index=np.array(ki, np.int32), n_corr=N, n=n, min_inliers=n_min, limit=limit, state=[0, 0],
                best_inliers=None, best_Tcw=None)


def sample(N, draw):
    """:188-201: four indices out of the list of all indices, each taken out by moving the last entry into its place."""
    avail = list(range(N))
    idx = []
    for k in range(4):
        randi = int(draw[k])
        assert 0 <= randi < len(avail)
        idx.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return idx


# ---------------------------------------------------------------------------------------------------------------------
# the stand-ins
def _rot(theta):
    """(c, s, t) of the Jacobi rotation for theta = cot(2 phi)."""
    t = f64(1.0) / (abs(theta) + np.sqrt(theta * theta + f64(1.0)))
    if theta < 0:
        t = -t
    c = f64(1.0) / np.sqrt(t * t + f64(1.0))
    return c, t * c, t


def jacobi_eig(A):
    """Eigenvalues (descending) and eigenvectors (rows of the second result, as CV_SVD_U_T gives them) of the symmetric A."""
    A = np.array(A, f64)
    n = A.shape[0]
    V = np.eye(n, dtype=f64)
    fro = Z
    for i in range(n):
        for j in range(n):
            fro = fro + A[i, j] * A[i, j]
    thresh = EIG_EPS * np.sqrt(fro)
    for _ in range(EIG_SWEEPS):
        changed = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if not abs(apq) > thresh:
                    continue
                changed = True
                app, aqq = A[p, p], A[q, q]
                c, s, t = _rot((aqq - app) / (f64(2.0) * apq))
                ap, aq = A[:, p].copy(), A[:, q].copy()
                new_p, new_q = c * ap - s * aq, s * ap + c * aq
                A[:, p] = new_p
                A[p, :] = new_p
                A[:, q] = new_q
                A[q, :] = new_q
                A[p, p] = app - t * apq
                A[q, q] = aqq + t * apq
                A[p, q] = Z
                A[q, p] = Z
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - s * vq
                V[:, q] = s * vp + c * vq
        if not changed:
            break
    w = [A[i, i] for i in range(n)]
    order, used = [], [False] * n
    for _ in range(n):
        b = -1
        for i in range(n):
            if not used[i] and (b < 0 or w[i] > w[b]):
                b = i
        used[b] = True
        order.append(b)
    return np.array([w[i] for i in order], f64), np.array([V[:, i] for i in order], f64)


def svd_cols(B):
    """One-sided Jacobi on the columns of B [m, n]: returns (W = B V with orthogonal columns, V, s2 = squared column norms)."""
    W = np.array(B, f64)
    m, n = W.shape
    V = np.eye(n, dtype=f64)
    for _ in range(SVD_SWEEPS):
        changed = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                al = be = ga = Z
                for i in range(m):
                    al = al + W[i, p] * W[i, p]
                    be = be + W[i, q] * W[i, q]
                    ga = ga + W[i, p] * W[i, q]
                if not abs(ga) > SVD_EPS * np.sqrt(al * be):
                    continue
                changed = True
                c, s, _ = _rot((be - al) / (f64(2.0) * ga))
                for M, rows in ((W, m), (V, n)):
                    for i in range(rows):
                        xp, xq = M[i, p], M[i, q]
                        M[i, p] = c * xp - s * xq
                        M[i, q] = s * xp + c * xq
        if not changed:
            break
    s2 = []
    for j in range(n):
        a = Z
        for i in range(m):
            a = a + W[i, j] * W[i, j]
        s2.append(a)
    return W, V, s2


def _kept(s2):
    smax = Z
    sig = [np.sqrt(v) for v in s2]
    for v in sig:
        if v > smax:
            smax = v
    return [sig[j] > SVD_CUT * smax for j in range(len(s2))]


def svd_solve(B, b):
    """cvSolve(CV_SVD): the minimum-norm least-squares solution."""
    W, V, s2 = svd_cols(B)
    keep = _kept(s2)
    m, n = W.shape
    coef = []
    for j in range(n):
        d = Z
        for i in range(m):
            d = d + W[i, j] * b[i]
        with np.errstate(all="ignore"):
            coef.append(d / s2[j])
    x = []
    for k in range(n):
        a = Z
        for j in range(n):
            if keep[j]:
                a = a + coef[j] * V[k, j]
        x.append(a)
    return x


def svd_pinv3(Cm):
    """cvInvert(CV_SVD) of a 3x3."""
    W, V, s2 = svd_cols(Cm)
    keep = _kept(s2)
    out = np.zeros((3, 3), f64)
    for k in range(3):
        for i in range(3):
            a = Z
            for j in range(3):
                if keep[j]:
                    a = a + V[k, j] * (W[i, j] / s2[j])
            out[k, i] = a
    return out


def svd_uvt3(Am):
    """U V^T of the 3x3 Am (:608-612).  A zero singular value divides 0 by 0: the NaN propagates."""
    W, V, s2 = svd_cols(Am)
    sig = [np.sqrt(v) for v in s2]
    R = np.zeros((3, 3), f64)
    for i in range(3):
        for j in range(3):
            a = Z
            for k in range(3):
                a = a + (W[i, k] / sig[k]) * V[j, k]
            R[i, j] = a
    return R


def qr_solve(A, b, X, nr, nc):
    """:860-950 on the flat row-major A.  Returns False where the reference returns early (X untouched)."""
    A1, A2 = [Z] * nc, [Z] * nc
    for k in range(nc):
        kk = k * nc + k
        p = kk
        eta = abs(A[p])
        for i in range(k + 1, nr):                                              # :881-885: the pointer lags the index by one row
            elt = abs(A[p])
            if eta < elt:
                eta = elt
            p += nc
        if eta == 0:
            return False
        inv_eta = f64(1.0) / eta
        s = Z
        p = kk
        for i in range(k, nr):
            A[p] = A[p] * inv_eta
            s = s + A[p] * A[p]
            p += nc
        sigma = np.sqrt(s)
        if A[kk] < 0:
            sigma = -sigma
        A[kk] = A[kk] + sigma
        A1[k] = sigma * A[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = Z
            p = kk
            for i in range(k, nr):
                s = s + A[p] * A[p + j - k]
                p += nc
            tau = s / A1[k]
            p = kk
            for i in range(k, nr):
                A[p + j - k] = A[p + j - k] - tau * A[p]
                p += nc
    for j in range(nc):
        tau = Z
        p = j * nc + j
        for i in range(j, nr):
            tau = tau + A[p] * b[i]
            p += nc
        tau = tau / A1[j]
        p = j * nc + j
        for i in range(j, nr):
            b[i] = b[i] - tau * A[p]
            p += nc
    X[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = Z
        for j in range(i + 1, nc):
            s = s + A[i * nc + j] * X[j]
        X[i] = (b[i] - s) / A2[i]
    return True


# ---------------------------------------------------------------------------------------------------------------------
# EPnP (:375-858)
def _alphas(ci, c0, pw):
    d = [pw[j] - c0[j] for j in range(3)]
    a = [None] * 4
    for j in range(3):
        a[1 + j] = ci[j, 0] * d[0] + ci[j, 1] * d[1] + ci[j, 2] * d[2]
    a[0] = f64(1.0) - a[1] - a[2] - a[3]                                         # 1.0f is exact
    return a


def _m_rows(a, u, v, cam):
    M1, M2 = [], []
    for i in range(4):
        M1 += [a[i] * cam["fu"], Z, a[i] * (cam["uc"] - u)]
        M2 += [Z, a[i] * cam["fv"], a[i] * (cam["vc"] - v)]
    return M1, M2


def pca_sign(u):
    """The sign of a principal axis is the solver's choice, and the pose depends on it at the noise level (the control points
    move).  Stated choice: the component of largest magnitude (the first of equals) is made non-negative."""
    b = 0
    for j in (1, 2):
        if abs(u[j]) > abs(u[b]):
            b = j
    return [-x for x in u] if u[b] < 0 else list(u)


def mtm_of(pws, us, cam):
    """choose_control_points, compute_barycentric_coordinates and M^T M (:375-451, :482-492)."""
    n = len(pws)
    c0 = [Z, Z, Z]
    for i in range(n):
        for j in range(3):
            c0[j] = c0[j] + pws[i][j]
    c0 = [c / f64(n) for c in c0]
    P = np.zeros((3, 3), f64)
    for a in range(3):
        for b in range(3):
            s = Z
            for i in range(n):
                s = s + (pws[i][a] - c0[a]) * (pws[i][b] - c0[b])
            P[a, b] = s
    dc, uct = jacobi_eig(P)
    cws = [c0]
    for i in range(1, 4):
        k = np.sqrt(dc[i - 1] / f64(n))
        u = pca_sign(uct[i - 1])
        cws.append([c0[j] + k * u[j] for j in range(3)])
    cc = np.zeros((3, 3), f64)
    for i in range(3):
        for j in range(1, 4):
            cc[i, j - 1] = cws[j][i] - cws[0][i]
    ci = svd_pinv3(cc)
    alphas = [_alphas(ci, c0, pws[i]) for i in range(n)]
    MtM = np.zeros((12, 12), f64)
    rows = [_m_rows(alphas[i], us[i][0], us[i][1], cam) for i in range(n)]
    for a in range(12):
        for b in range(12):
            s = Z
            for M1, M2 in rows:
                s = s + M1[a] * M1[b]
                s = s + M2[a] * M2[b]
            MtM[a, b] = s
    return cws, alphas, MtM


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _dist2(p1, p2):
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2])


def compute_L_6x10(v):
    dv = [[None] * 6 for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            dv[i][j] = [v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
    two = f64(2.0)
    L = []
    for i in range(6):
        L.append([_dot3(dv[0][i], dv[0][i]), two * _dot3(dv[0][i], dv[1][i]), _dot3(dv[1][i], dv[1][i]),
                  two * _dot3(dv[0][i], dv[2][i]), two * _dot3(dv[1][i], dv[2][i]), _dot3(dv[2][i], dv[2][i]),
                  two * _dot3(dv[0][i], dv[3][i]), two * _dot3(dv[1][i], dv[3][i]), two * _dot3(dv[2][i], dv[3][i]),
                  _dot3(dv[3][i], dv[3][i])])
    return L


def find_betas_approx(which, L, rho):
    cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}[which]
    b = svd_solve([[L[i][c] for c in cols] for i in range(6)], rho)
    be = [Z] * 4
    if which == 1:
        if b[0] < 0:
            be[0] = np.sqrt(-b[0])
            be[1], be[2], be[3] = -b[1] / be[0], -b[2] / be[0], -b[3] / be[0]
        else:
            be[0] = np.sqrt(b[0])
            be[1], be[2], be[3] = b[1] / be[0], b[2] / be[0], b[3] / be[0]
        return be
    if b[0] < 0:
        be[0] = np.sqrt(-b[0])
        be[1] = np.sqrt(-b[2]) if b[2] < 0 else Z
    else:
        be[0] = np.sqrt(b[0])
        be[1] = np.sqrt(b[2]) if b[2] > 0 else Z
    if b[1] < 0:
        be[0] = -be[0]
    if which == 3:
        be[2] = b[3] / be[0]
    return be


def gauss_newton(L, rho, be):
    x = [Z] * 4
    two = f64(2.0)
    for _ in range(5):
        A, b = [], []
        for i in range(6):
            r = L[i]
            A += [two * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3],
                  r[1] * be[0] + two * r[2] * be[1] + r[4] * be[2] + r[7] * be[3],
                  r[3] * be[0] + r[4] * be[1] + two * r[5] * be[2] + r[8] * be[3],
                  r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + two * r[9] * be[3]]
            b.append(rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] + r[3] * be[0] * be[2] +
                               r[4] * be[1] * be[2] + r[5] * be[2] * be[2] + r[6] * be[0] * be[3] + r[7] * be[1] * be[3] +
                               r[8] * be[2] * be[3] + r[9] * be[3] * be[3]))
        qr_solve(A, b, x, 6, 4)
        for i in range(4):
            be[i] = be[i] + x[i]
    return be


def compute_R_and_t(v, be, pws, us, alphas, cam):
    n = len(pws)
    ccs = [[Z, Z, Z] for _ in range(4)]
    for i in range(4):
        for j in range(4):
            for k in range(3):
                ccs[j][k] = ccs[j][k] + be[i] * v[i][3 * j + k]

    def pc_of(a):
        return [a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)]
    if pc_of(alphas[0])[2] < 0.0:                                                # solve_for_sign: pcs[2] only
        ccs = [[-x for x in r] for r in ccs]
    pcs = [pc_of(a) for a in alphas]
    pc0, pw0 = [Z, Z, Z], [Z, Z, Z]
    for i in range(n):
        for j in range(3):
            pc0[j] = pc0[j] + pcs[i][j]
            pw0[j] = pw0[j] + pws[i][j]
    pc0 = [x / f64(n) for x in pc0]
    pw0 = [x / f64(n) for x in pw0]
    abt = np.zeros((3, 3), f64)
    for j in range(3):
        for k in range(3):
            s = Z
            for i in range(n):
                s = s + (pcs[i][j] - pc0[j]) * (pws[i][k] - pw0[k])
            abt[j, k] = s
    R = svd_uvt3(abt)
    det = (R[0, 0] * R[1, 1] * R[2, 2] + R[0, 1] * R[1, 2] * R[2, 0] + R[0, 2] * R[1, 0] * R[2, 1] -
           R[0, 2] * R[1, 1] * R[2, 0] - R[0, 1] * R[1, 0] * R[2, 2] - R[0, 0] * R[1, 2] * R[2, 1])
    if det < 0:
        R[2, 0], R[2, 1], R[2, 2] = -R[2, 0], -R[2, 1], -R[2, 2]
    t = [pc0[i] - _dot3(R[i], pw0) for i in range(3)]
    s = Z
    for i in range(n):
        Xc = _dot3(R[0], pws[i]) + t[0]
        Yc = _dot3(R[1], pws[i]) + t[1]
        inv = f64(1.0) / (_dot3(R[2], pws[i]) + t[2])
        ue = cam["uc"] + cam["fu"] * Xc * inv
        ve = cam["vc"] + cam["fv"] * Yc * inv
        u, vv = us[i]
        s = s + np.sqrt((u - ue) * (u - ue) + (vv - ve) * (vv - ve))
    return R, t, s / f64(n)


def compute_pose(pws, us, cam):
    """:477-525.  pws [n][3], us [n][2] doubles; cam = make_cam(...).  Returns (R [3, 3], t [3]) in double."""
    with np.errstate(all="ignore"):
        cws, alphas, MtM = mtm_of(pws, us, cam)
        _, ut = jacobi_eig(MtM)
        v = [ut[11], ut[10], ut[9], ut[8]]
        L = compute_L_6x10(v)
        rho = [_dist2(cws[0], cws[1]), _dist2(cws[0], cws[2]), _dist2(cws[0], cws[3]), _dist2(cws[1], cws[2]),
               _dist2(cws[1], cws[3]), _dist2(cws[2], cws[3])]
        sol = [None]
        for which in (1, 2, 3):
            be = gauss_newton(L, rho, find_betas_approx(which, L, rho))
            sol.append(compute_R_and_t(v, be, pws, us, alphas, cam))
        N = 1
        if sol[2][2] < sol[1][2]:
            N = 2
        if sol[3][2] < sol[N][2]:
            N = 3
        return sol[N][0], sol[N][1]


def make_cam(fx, fy, cx, cy):
    return dict(fu=f64(f32(fx)), fv=f64(f32(fy)), uc=f64(f32(cx)), vc=f64(f32(cy)))


def check_inliers(S, R, t, cam):
    """:308-339."""
    N = S["n_corr"]
    mask = np.zeros(N, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(N):
            X = [f64(v) for v in S["p3d"][i]]
            Xc = f32(R[0][0] * X[0] + R[0][1] * X[1] + R[0][2] * X[2] + t[0])
            Yc = f32(R[1][0] * X[0] + R[1][1] * X[1] + R[1][2] * X[2] + t[1])
            invZc = f32(f64(1.0) / (R[2][0] * X[0] + R[2][1] * X[1] + R[2][2] * X[2] + t[2]))
            ue = cam["uc"] + cam["fu"] * f64(Xc) * f64(invZc)
            ve = cam["vc"] + cam["fv"] * f64(Yc) * f64(invZc)
            dx = f32(f64(S["p2d"][i][0]) - ue)
            dy = f32(f64(S["p2d"][i][1]) - ve)
            err = f32(f32(dx * dx) + f32(dy * dy))
            if err < S["max_err"][i]:
                mask[i] = 1
    return mask


def pose_of(S, idx, cam):
    pws = [[f64(v) for v in S["p3d"][i]] for i in idx]
    us = [[f64(v) for v in S["p2d"][i]] for i in idx]
    return compute_pose(pws, us, cam)


def _tcw(R, t):
    out = np.zeros(12, f32)
    for r in range(3):
        for c in range(3):
            out[4 * r + c] = f32(R[r][c])
        out[4 * r + 3] = f32(t[r])
    return out


def refine(S, cam, cache=None):
    """Refine() (:260-305) of mvbBestInliers: (success, refined mask, refined count, refined Tcw)."""
    key = S["best_inliers"].tobytes()
    if cache is not None and key in cache:
        return cache[key]
    idx = [i for i in range(S["n_corr"]) if S["best_inliers"][i]]
    R, t = pose_of(S, idx, cam)
    mask = check_inliers(S, R, t, cam)
    cnt = int(mask.sum())
    out = (cnt > S["min_inliers"], mask, cnt, _tcw(R, t))                       # :292, strict
    if cache is not None:
        cache[key] = out
    return out


def iterate(S, draws, n_iterations, cam, hypothesis=None, refine_fn=None, cache=None):
    """iterate (:165-258).  draws [rows][4]; row `it` serves iteration number `it`.  Advances S (state, best_inliers,
    best_Tcw) and returns (report [8], Tcw [12] or None, inliers over the n key-point slots or None).  `hypothesis`, when
    given, replaces compute_pose + CheckInliers of iteration `it` by hypothesis(it) -> (mask, Tcw), and refine_fn(best mask) ->
    (success, mask, count, Tcw) replaces Refine(): the state machine alone.  `cache` memoises Refine() per best set."""
    N, n_min, limit = S["n_corr"], S["min_inliers"], S["limit"]

    def report(status, ret_it, n_inl):
        return np.array([status, N, limit, S["state"][0], S["state"][1], ret_it, n_inl, n_min], np.int32)

    def slots(mask):
        out = np.zeros(S["n"], np.uint8)
        for i in range(N):
            if mask[i]:
                out[S["kp_index"][i]] = 1
        return out
    if N < n_min:                                                               # :173
        return report(TOO_FEW, -1, 0), None, None
    cur = 0
    while S["state"][0] < limit or cur < n_iterations:                          # :182, an OR
        cur += 1
        it = S["state"][0]
        S["state"][0] += 1
        if hypothesis is not None:
            mask, tcw = hypothesis(it)
        else:
            R, t = pose_of(S, sample(N, draws[it]), cam)
            mask, tcw = check_inliers(S, R, t, cam), _tcw(R, t)
        cnt = int(np.sum(mask))
        if cnt >= n_min:                                                        # :209
            if cnt > S["state"][1]:                                             # :212
                S["best_inliers"] = np.array(mask, np.uint8)
                S["state"][1] = cnt
                S["best_Tcw"] = np.array(tcw, f32)
            ok, rmask, rcnt, rtcw = refine_fn(S["best_inliers"]) if refine_fn is not None else refine(S, cam, cache)
            if ok:
                return report(REFINED, it, rcnt), rtcw, slots(rmask)
    if S["state"][1] >= n_min:                                                  # :241-255; mnIterations >= limit holds here
        return report(BEST, -1, S["state"][1]), S["best_Tcw"].copy(), slots(S["best_inliers"])
    return report(NO_MORE, -1, 0), None, None
