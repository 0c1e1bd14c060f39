"""Sequential reference of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044), written from the reference text.

One VertexSim3Expmap per key frame that is not bad, EdgeSim3 with the identity as information, g2o's numeric Jacobian
(base_binary_edge.hpp:131-205), g2o's Levenberg-Marquardt with setUserLambdaInit(1e-16), 20 outer iterations, no robust
kernel.  Plain Python floats: every operation is one IEEE double operation, in the order written here.  What the reference
leaves to Eigen, libm, a sparse Cholesky or the order of a std::set of pointers is restated with a stated order (DESIGN.md
section 3):

  - sets and maps of key frames: ascending bank row;
  - std::log, acos: det_log64, det_acos64 (fdlibm's __ieee754_log / __ieee754_acos); exp, sin, cos: det_exp64, det_sincos64;
  - W.lu().solve(t): a 3x3 LU with partial pivoting, the largest |a| of the column, the first of equals;
  - an edge's blocks: sums over the 7 error rows, ascending from 0.0; a vertex's diagonal block and b: its edges in creation
    order from 0.0; an off-diagonal block: the edges between the two vertices in creation order, added onto 0.0;
  - chi2 and computeScale: item t belongs to lane t mod 256, a lane adds ascending from 0.0, the 64 lanes of a wavefront meet
    in an xor butterfly (offsets 1 .. 32), the wavefronts are added in order;
  - the linear system (LinearSolverEigen's sparse Cholesky in the reference): dense over 7 unknowns per free vertex in row
    order, an unpivoted LDLt, every element receives its updates in ascending k, one multiply and one subtract each, ok iff
    every pivot is > 0; L y = b column by column, y / d, L^T x = y from the last column.  No block is skipped.

KeyFrame::GetCovisiblesByWeight(100) is restated as the reference has it (src/KeyFrame.cc:184-199): the prefix of the ordered
list whose weight is at least 100, and NOTHING when no entry of the list is below 100 (upper_bound returns end()).
"""
import math
import struct

import numpy as np

from .poseopt import DBL_MAX, WAVE, det_sincos64, f32, fdiv, fsqrt, mat3, quat_from_R, quat_rot, to_R
from .sim3opt import DELTA, SCALAR, det_exp64, sim3_exp, sim3_inverse, sim3_mul

TEAM = 256
OK, CAPACITY, SINGULAR = range(3)
MAX_KF = 512
MIN_FEAT = 100
POINT_PRESENT = 1
K_LC, K_TREE, K_LOOP, K_COVIS = range(4)

# ---- det_log64: fdlibm's __ieee754_log with the word tests written as doubles ---------------------------------------------
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
LG1, LG2, LG3, LG4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
LG5, LG6, LG7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
LOG_SPLIT = 1.4142112731933594          # 1 + 0x6a09c / 2^20: mantissas from here on are halved
LOG_MID_LO, LOG_MID_HI = 1.3799991607666016, 1.4200000762939453      # 1 + 0x6147a / 2^20, 1 + 0x6b852 / 2^20
LOG_TINY = 9.5367431640625e-07          # 2^-20
TWO54 = 18014398509481984.0
DBL_MIN = 2.2250738585072014e-308


def det_log64(x):
    if x != x:
        return x
    if x < 0:
        return float("nan")
    if x == 0:
        return float("-inf")
    if x == float("inf"):
        return x
    k = 0
    if x < DBL_MIN:
        x = x * TWO54
        k = -54
    m, e = math.frexp(x)                        # x = m 2^e, m in [0.5, 1)
    m = m * 2.0
    k = k + (e - 1)
    mid = LOG_MID_LO <= m < LOG_MID_HI
    if m >= LOG_SPLIT:
        m = m * 0.5
        k = k + 1
    f = m - 1.0
    dk = float(k)
    if abs(f) < LOG_TINY:
        if f == 0:
            if k == 0:
                return 0.0
            return dk * LN2_HI + dk * LN2_LO
        R = f * f * (0.5 - 0.33333333333333333 * f)
        if k == 0:
            return f - R
        return dk * LN2_HI - ((R - dk * LN2_LO) - f)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (LG2 + w * (LG4 + w * LG6))
    t2 = z * (LG1 + w * (LG3 + w * (LG5 + w * LG7)))
    R = t2 + t1
    if mid:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * LN2_HI - ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * LN2_HI - ((s * (f - R) - dk * LN2_LO) - f)


# ---- det_acos64: fdlibm's __ieee754_acos ------------------------------------------------------------------------------------
PIO2_HI, PIO2_LO, PI = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
PS0, PS1, PS2 = 1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01
PS3, PS4, PS5 = -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05
QS1, QS2, QS3, QS4 = -2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02
ACOS_TINY = 6.938893903907228e-18       # 2^-57


def _acos_r(z):
    p = z * (PS0 + z * (PS1 + z * (PS2 + z * (PS3 + z * (PS4 + z * PS5)))))
    q = 1.0 + z * (QS1 + z * (QS2 + z * (QS3 + z * QS4)))
    return p / q


def clear_low_word(x):
    return struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", x))[0] & 0xffffffff00000000))[0]


def det_acos64(x):
    if x != x:
        return x
    ax = abs(x)
    if ax >= 1.0:
        if ax == 1.0:
            return 0.0 if x > 0 else PI + 2.0 * PIO2_LO
        return float("nan")
    if ax < 0.5:
        if ax <= ACOS_TINY:
            return PIO2_HI + PIO2_LO
        r = _acos_r(x * x)
        return PIO2_HI - (x - (PIO2_LO - x * r))
    if x < 0:
        z = (1.0 + x) * 0.5
        r = _acos_r(z)
        s = math.sqrt(z)
        w = r * s - PIO2_LO
        return PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = clear_low_word(s)
    c = (z - df * df) / (s + df)
    r = _acos_r(z)
    w = r * s + c
    return 2.0 * (df + w)


# ---- Sim3::log (sim3.h:148-230) ---------------------------------------------------------------------------------------------
def lu3_solve(W, t):
    """W.lu().solve(t): partial pivoting, the largest |a| of the column, the first of equals; rows eliminated in order."""
    a = [[W[0], W[1], W[2], t[0]], [W[3], W[4], W[5], t[1]], [W[6], W[7], W[8], t[2]]]
    for k in range(2):
        p = k
        for i in range(k + 1, 3):
            if abs(a[i][k]) > abs(a[p][k]):
                p = i
        a[k], a[p] = a[p], a[k]
        for i in range(k + 1, 3):
            l = fdiv(a[i][k], a[k][k])
            for j in range(k + 1, 4):
                a[i][j] = a[i][j] - l * a[k][j]
    x2 = fdiv(a[2][3], a[2][2])
    x1 = fdiv(a[1][3] - a[1][2] * x2, a[1][1])
    x0 = fdiv((a[0][3] - a[0][1] * x1) - a[0][2] * x2, a[0][0])
    return [x0, x1, x2]


def sim3_log(S):
    s = S[7]
    sigma = det_log64(s)
    R = to_R(S[0:4])
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    eps = 0.00001
    near = d > 1 - eps
    if near:
        omega = [0.5 * v for v in dR]
    else:
        theta = det_acos64(d)
        theta2 = theta * theta
        f = fdiv(theta, 2 * fsqrt(1 - d * d))
        omega = [f * v for v in dR]
        sn, cs = det_sincos64(theta)
    if abs(sigma) < eps:
        C = 1.0
        if near:
            A = 1. / 2.
            B = 1. / 6.
        else:
            A = fdiv(1 - cs, theta2)
            B = fdiv(theta - sn, theta2 * theta)
    else:
        C = fdiv(s - 1, sigma)
        if near:
            sigma2 = sigma * sigma
            A = fdiv((sigma - 1) * s + 1, sigma2)
            B = fdiv((0.5 * sigma2 - sigma + 1) * s, sigma2 * sigma)
        else:
            a, b = s * sn, s * cs
            c = theta2 + sigma * sigma
            A = fdiv(a * sigma + (1 - b) * theta, theta * c)
            B = fdiv(C - fdiv((b - 1) * sigma + a * theta, c), theta2)         # "* 1. / (theta2)": the product with 1 is exact
    Om = [0.0, -omega[2], omega[1], omega[2], 0.0, -omega[0], -omega[1], omega[0], 0.0]
    Om2 = mat3(Om, Om)
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    W = [(A * Om[k] + B * Om2[k]) + C * I[k] for k in range(9)]
    return omega + lu3_solve(W, S[4:7]) + [sigma]


def edge_error(meas, Si, Sj):
    """EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): log(C * v1 * v2^-1)."""
    return sim3_log(sim3_mul(sim3_mul(meas, Si), sim3_inverse(Sj)))


def sim3_from_Tcw(T):
    """g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0): the floats widen to double, the quaternion is not normalised."""
    T = [float(v) for v in T]
    return quat_from_R([T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]) + [T[3], T[7], T[11], 1.0]


def sim3_map(S, X):
    r = quat_rot(S[0:4], X)
    return [S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]]


# ---- the graph ----------------------------------------------------------------------------------------------------------------
def covisibles_by_weight(T, r):
    """KeyFrame::GetCovisiblesByWeight(100) as src/KeyFrame.cc:184-199 has it."""
    n = int(T["n_ord"][r])
    k = 0
    while k < n and int(T["ord_w"][r][k]) >= MIN_FEAT:
        k += 1
    if k == n:
        return []
    return [int(T["ord_kf"][r][i]) for i in range(k)]


def build_edges(T, cur, loop_row, vScw):
    """:852-983.  Returns (edges [(row i, row j, measurement, kind)], counts {inserted, weight, null})."""
    rows = len(T["kf_bad"])
    bad = [bool(b) for b in T["kf_bad"]]
    kf_id = [int(v) for v in T["kf_id"]]
    cnt = dict(inserted=0, weight=0, null=0)
    edges = []
    inserted = set()
    nc = lambda r: [float(v) for v in T["non_corrected"][r]]  # noqa: E731
    for i in range(rows):
        for o in range(int(T["lc_start"][i]), int(T["lc_start"][i + 1])):
            j = int(T["lc_kf"][o])
            if bad[i] or j < 0 or j >= rows or bad[j] or i == j:
                cnt["null"] += 1
                continue
            if (i != cur or j != loop_row) and int(T["conn_w"][i][j]) < MIN_FEAT:
                cnt["weight"] += 1
                continue
            edges.append((i, j, sim3_mul(vScw[j], sim3_inverse(vScw[i])), K_LC))
            inserted.add((min(i, j), max(i, j)))
    for i in range(rows):
        if bad[i]:
            continue
        Swi = sim3_inverse(nc(i) if T["in_non_corrected"][i] else vScw[i])
        Sw = lambda j: nc(j) if T["in_non_corrected"][j] else vScw[j]  # noqa: E731
        p = int(T["parent"][i])
        if p >= 0:
            if p >= rows or bad[p] or p == i:
                cnt["null"] += 1
            else:
                edges.append((i, p, sim3_mul(Sw(p), Swi), K_TREE))
        loops = [int(T["loop_kf"][o]) for o in range(int(T["loop_start"][i]), int(T["loop_start"][i + 1]))]
        for l in loops:
            if l < 0 or l >= rows or l == i:
                cnt["null"] += 1
            elif kf_id[l] < kf_id[i]:
                if bad[l]:
                    cnt["null"] += 1
                else:
                    edges.append((i, l, sim3_mul(Sw(l), Swi), K_LOOP))
        for n in covisibles_by_weight(T, i):
            if n < 0 or n >= rows or n == i:
                continue
            if n == p or (int(T["parent"][n]) == i and not bad[n]) or n in loops:
                continue
            if bad[n] or not kf_id[n] < kf_id[i]:
                continue
            if (min(i, n), max(i, n)) in inserted:
                cnt["inserted"] += 1
                continue
            edges.append((i, n, sim3_mul(Sw(n), Swi), K_COVIS))
    return edges, cnt


# ---- the sums over lanes ------------------------------------------------------------------------------------------------------
def team_sum(values):
    lanes = [0.0] * TEAM
    for t, v in enumerate(values):
        lanes[t % TEAM] = lanes[t % TEAM] + v
    total = None
    idx = np.arange(WAVE)
    with np.errstate(invalid="ignore", over="ignore"):
        for w0 in range(0, TEAM, WAVE):
            wave = np.array(lanes[w0:w0 + WAVE], np.float64)
            for off in (1, 2, 4, 8, 16, 32):
                wave = wave + wave[idx ^ off]
            total = wave[0] if total is None else total + wave[0]
    return float(total)


def chi2_of(e):
    c = 0.0
    for k in range(7):
        c = c + e[k] * e[k]
    return c


# ---- the dense system -----------------------------------------------------------------------------------------------------------
def ldlt_solve(A, b):
    """Unpivoted LDLt of the lower triangle of A (float64 [n, n], destroyed), in index order: (ok, x).  Element (i, j)
    receives A[i][j] - (A[i][k] / d_k) * A[j][k] for k ascending: array operations, one IEEE operation per element each."""
    n = len(b)
    with np.errstate(all="ignore"):
        for k in range(n):
            d = A[k, k]
            if not (d > 0):
                return False, None
            c = A[k + 1:, k].copy()
            l = c / d
            A[k + 1:, k + 1:] -= l[:, None] * c[None, :]
            A[k + 1:, k] = l
        y = np.array(b, np.float64)
        for j in range(n):
            y[j + 1:] -= A[j + 1:, j] * y[j]
        y = y / np.diag(A)
        for j in range(n - 1, 0, -1):
            y[:j] -= A[j, :j] * y[j]
    return True, [float(v) for v in y]


def perturbations(fix_scale):
    """Sim3(+-delta e_d) of a linearisation, d = 0 .. 6: oplusImpl zeroes update[6] when the scale is fixed."""
    D = []
    for d in range(7):
        for v in (DELTA, -DELTA):
            u = [0.0] * 7
            u[d] = v
            if fix_scale:
                u[6] = 0.0
            D.append(sim3_exp(u))
    return D


def linearize_edge(meas, Si, Sj, free_i, free_j, D):
    """The error, and per free end the numeric Jacobian [7 rows][7 columns]."""
    err = edge_error(meas, Si, Sj)
    J = [None, None]
    for end, free in ((0, free_i), (1, free_j)):
        if not free:
            continue
        cols = []
        for d in range(7):
            if end == 0:
                ep = edge_error(meas, sim3_mul(D[2 * d], Si), Sj)
                em = edge_error(meas, sim3_mul(D[2 * d + 1], Si), Sj)
            else:
                ep = edge_error(meas, Si, sim3_mul(D[2 * d], Sj))
                em = edge_error(meas, Si, sim3_mul(D[2 * d + 1], Sj))
            cols.append([SCALAR * (ep[k] - em[k]) for k in range(7)])
        J[end] = [[cols[d][k] for d in range(7)] for k in range(7)]
    return err, J[0], J[1]


def jtj(Ja, Jb):
    out = [[0.0] * 7 for _ in range(7)]
    for a in range(7):
        for b in range(7):
            s = 0.0
            for k in range(7):
                s = s + Ja[k][a] * Jb[k][b]
            out[a][b] = s
    return out


def jte(Ja, err):
    out = []
    for a in range(7):
        s = 0.0
        for k in range(7):
            s = s + Ja[k][a] * -err[k]
        out.append(s)
    return out


# ---- the function ---------------------------------------------------------------------------------------------------------------
def optimize_essential_graph(T, cur, loop_row, fix_scale, max_kf=MAX_KF, max_edges=1 << 20, info=None):
    """T: dict of the tables (kf_bad, kf_id, Tcw, parent, conn_w, ord_kf, ord_w, n_ord, loop_start, loop_kf, lc_start, lc_kf,
    corrected, non_corrected, in_corrected, in_non_corrected, world, flags, ref_kf, corrected_by_kf, corrected_ref).  Returns
    dict(report [16], and unless the status is CAPACITY: Tcw {row: [12] float32}, world {point: [3] float32}, point_list,
    Scw {row: [8]}, Swc {row: [8]}).  info (a dict) receives edges, trace [(iteration, trial, accepted)], tried [per trial
    the estimates of all vertices]."""
    rows = len(T["kf_bad"])
    vrows = [r for r in range(rows) if not T["kf_bad"][r]]
    nv = len(vrows)
    report = [0] * 16
    report[1] = nv
    if nv > max_kf:
        report[0] = CAPACITY
        return dict(report=report)
    vScw = {}
    for r in vrows:
        vScw[r] = [float(v) for v in T["corrected"][r]] if T["in_corrected"][r] else sim3_from_Tcw(T["Tcw"][r])
    edges, cnt = build_edges(T, cur, loop_row, vScw)
    free = [r for r in vrows if r != loop_row]
    fidx = {r: f for f, r in enumerate(free)}
    n = 7 * len(free)
    kinds = [sum(1 for e in edges if e[3] == k) for k in range(4)]
    report[2:6] = kinds
    report[6], report[7], report[12] = cnt["inserted"], cnt["weight"], cnt["null"]
    report[10] = n
    if len(edges) > max_edges:
        report[0] = CAPACITY
        return dict(report=report)
    est = dict(vScw)
    x = [0.0] * n
    D = perturbations(fix_scale)
    trace, tried_log = [], []
    lam = ni = 0.0
    n_bad = its = trials = 0
    status = OK
    incident = {r: [j for j, e in enumerate(edges) if e[0] == r or e[1] == r] for r in free}

    def chi_at(E):
        return team_sum([chi2_of(edge_error(m, E[i], E[j])) for (i, j, m, _k) in edges])

    for it in range(20 if edges and n else 0):
        lin = [linearize_edge(m, est[i], est[j], i in fidx, j in fidx, D) for (i, j, m, _k) in edges]
        Hd, bv, Hoff = {}, [0.0] * n, {}
        for r in free:
            f = fidx[r]
            H = [[0.0] * 7 for _ in range(7)]
            b = [0.0] * 7
            for j in incident[r]:
                err, Ji, Jj = lin[j]
                Jm = Ji if edges[j][0] == r else Jj
                blk, g = jtj(Jm, Jm), jte(Jm, err)
                for a in range(7):
                    b[a] = b[a] + g[a]
                    for c in range(7):
                        H[a][c] = H[a][c] + blk[a][c]
                o = edges[j][1] if edges[j][0] == r else edges[j][0]
                if o in fidx and fidx[o] < f:
                    blk = jtj(Jm, Jj if edges[j][0] == r else Ji)
                    acc = Hoff.setdefault((f, fidx[o]), [[0.0] * 7 for _ in range(7)])
                    for a in range(7):
                        for c in range(7):
                            acc[a][c] = acc[a][c] + blk[a][c]
            Hd[f] = H
            bv[7 * f:7 * f + 7] = b
        current = ini = team_sum([chi2_of(l[0]) for l in lin])
        if it == 0:
            lam, ni, n_bad = 1e-16, 2.0, 0
        rho = 0.0
        qmax = 0
        fails = 0
        while True:
            A = np.zeros((n, n), np.float64)
            for f, H in Hd.items():
                for a in range(7):
                    for c in range(a + 1):
                        A[7 * f + a, 7 * f + c] = H[a][c] + lam if a == c else H[a][c]
            for (f, g), blk in Hoff.items():
                A[7 * f:7 * f + 7, 7 * g:7 * g + 7] = np.array(blk, np.float64)
            ok2, sol = ldlt_solve(A, bv)
            if ok2:
                x = sol
            else:
                fails += 1
            if fix_scale:
                for f in range(len(free)):
                    x[7 * f + 6] = 0.0
            tried = dict(est)
            for r in free:
                f = fidx[r]
                tried[r] = sim3_mul(sim3_exp(x[7 * f:7 * f + 7]), est[r])
            tried_log.append([tried[r] for r in vrows])
            temp = chi_at(tried)
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = team_sum([x[t] * (lam * x[t] + bv[t]) for t in range(n)])
            scale = scale + 1e-3
            rho = fdiv(rho, scale)
            good = rho > 0 and math.isfinite(temp)
            trace.append((it, qmax, good))
            if good:
                y = 2 * rho - 1
                alpha = 1.0 - (y * y) * y
                alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
                lam = lam * sf
                ni = 2.0
                current = temp
                est = tried
            else:
                lam = lam * ni
                ni = ni * 2
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        its += 1
        if it == 0 and fails == qmax:
            status = SINGULAR
        if qmax == 10 or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:
            break
    report[0], report[8], report[9] = status, its, trials
    out = dict(Tcw={}, world={}, Scw={}, Swc={}, point_list=[])
    for r in vrows:
        S = est[r]
        out["Scw"][r] = vScw[r]
        out["Swc"][r] = sim3_inverse(S)
        R = to_R(S[0:4])
        m = fdiv(1., S[7])
        row = []
        for a in range(3):
            row += [f32(R[3 * a + c]) for c in range(3)] + [f32(S[4 + a] * m)]
        out["Tcw"][r] = np.array(row, np.float32)
    for p in range(len(T["flags"])):
        if not (int(T["flags"][p]) & POINT_PRESENT):
            continue
        out["point_list"].append(p)
        r = int(T["corrected_ref"][p]) if int(T["corrected_by_kf"][p]) == cur else int(T["ref_kf"][p])
        if r < 0 or r >= rows or T["kf_bad"][r]:
            continue                                                            # default-constructed Sim3s: the identity both ways
        X = [float(v) for v in T["world"][p]]
        Y = sim3_map(out["Swc"][r], sim3_map(vScw[r], X))
        out["world"][p] = np.array([f32(v) for v in Y], np.float32)
    report[11] = len(out["point_list"])
    out["report"] = report
    if info is not None:
        info.update(edges=edges, trace=trace, tried=tried_log, est=est)
    return out
