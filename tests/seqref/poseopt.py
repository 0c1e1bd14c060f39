"""Sequential reference of Optimizer::PoseOptimization (src/Optimizer.cc:239-451), written from the reference text.

One 6-DoF vertex with unary edges, g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp), the dense 6x6 solve,
SE3Quat and the two only-pose edges (types_six_dof_expmap.*), plus the two loops of Tracking that follow the call
(src/Tracking.cc:900-919 and :941-963).  Plain Python floats: every operation is one IEEE double operation, in the order
written here.  What the reference leaves to Eigen, libm or the summation order of a sequential loop is restated with a
stated order:

  - sums over edges: edge j of the compacted list belongs to lane j mod TEAM, a lane adds its edges in ascending j starting
    from 0.0, inactive edges add nothing; the lanes of a wavefront of 64 are combined by an xor butterfly (offsets 1, 2, 4,
    8, 16, 32), the wavefronts of the team are then added in wavefront order;
  - sin / cos: det_sincos64 (fdlibm's kernels, a three-part Cody-Waite reduction);
  - the 6x6 solve: a pivoted LDLt, largest |d| first, the first of equals;
  - Eigen's quaternion formulas, restated.
"""
import math

import numpy as np

TEAM = 256
WAVE = 64
PLAIN, DISCARD, LOCAL_MAP = range(3)
ONLY_TRACKING, STEREO = 1, 2
OK, TOO_FEW, ONE_ROUND = range(3)
POINT_OBSERVED = 2
DBL_MAX = 1.7976931348623157e308


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


# ---- det_sincos64 -------------------------------------------------------------------------------------------------------
S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
INVPIO2 = 6.36619772367581382433e-01
PIO2_1, PIO2_1T = 1.57079632673412561417e+00, 6.07710050650619224932e-11
PIO2_2, PIO2_2T = 6.07710050630396597660e-11, 2.02226624879595063154e-21
PIO2_3, PIO2_3T = 2.02226624871116645580e-21, 8.47842766036889956997e-32
PIO4 = 7.85398163397448278999e-01
SINCOS_RANGE = 1647099.0          # 2^20 * pi / 2: fn * PIO2_1 is exact below it


def kernel_sin(x, y):
    z = x * x
    v = z * x
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def kernel_cos(x, y):
    z = x * x
    w = z * z
    r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6))
    hz = 0.5 * z
    w = 1.0 - hz
    return w + (((1.0 - w) - hz) + (z * r - x * y))


def det_sincos64(x):
    """(sin x, cos x).  |x| <= pi/4: the kernels; up to SINCOS_RANGE: three Cody-Waite steps; beyond (or NaN): NaN, NaN."""
    if not (abs(x) <= SINCOS_RANGE):
        return float("nan"), float("nan")
    if abs(x) <= PIO4:
        return kernel_sin(x, 0.0), kernel_cos(x, 0.0)
    fn = float(math.floor(x * INVPIO2 + 0.5))
    r = x - fn * PIO2_1
    w = fn * PIO2_1T
    t = r
    w = fn * PIO2_2
    r = t - w
    w = fn * PIO2_2T - ((t - r) - w)
    t = r
    w = fn * PIO2_3
    r = t - w
    w = fn * PIO2_3T - ((t - r) - w)
    y0 = r - w
    y1 = (r - y0) - w
    s, c = kernel_sin(y0, y1), kernel_cos(y0, y1)
    q = int(fn) & 3
    if q == 0:
        return s, c
    if q == 1:
        return c, -s
    if q == 2:
        return -s, -c
    return -c, s


# ---- SE3Quat: q = (x, y, z, w), t --------------------------------------------------------------------------------------
def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def fdiv(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)."""
    if b == 0:
        if a != a or a == 0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def fsqrt(a):
    if a != a or a < 0:
        return float("nan")
    return math.sqrt(a)


def quat_case(rii, rjj, rkk, rkj, rjk, rji, rij, rki, rik):
    """The largest-diagonal branch for diagonal entry i: (q_i, q_j, q_k, w)."""
    t = fsqrt(rii - rjj - rkk + 1.0)
    qi = 0.5 * t
    t = fdiv(0.5, t)
    return qi, (rji + rij) * t, (rki + rik) * t, (rkj - rjk) * t


def quat_from_R(R):
    """Eigen's Quaterniond(Matrix3d), R row-major [9]."""
    t = (R[0] + R[4]) + R[8]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return [(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w]
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    if i == 0:
        x, y, z, w = quat_case(R[0], R[4], R[8], R[7], R[5], R[3], R[1], R[6], R[2])
    elif i == 1:
        y, z, x, w = quat_case(R[4], R[8], R[0], R[2], R[6], R[7], R[5], R[1], R[3])
    else:
        z, x, y, w = quat_case(R[8], R[0], R[4], R[3], R[1], R[2], R[6], R[5], R[7])
    return [x, y, z, w]


def normalize(q):
    if q[3] < 0:
        q = [-q[0], -q[1], -q[2], -q[3]]
    n = fsqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [fdiv(q[0], n), fdiv(q[1], n), fdiv(q[2], n), fdiv(q[3], n)]


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def quat_rot(q, v):
    uv = cross(q, v)
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    c = cross(q, uv)
    return [v[0] + q[3] * uv[0] + c[0], v[1] + q[3] * uv[1] + c[1], v[2] + q[3] * uv[2] + c[2]]


def to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def pose_from_Tcw(T):
    """Converter::toSE3Quat: the floats widen to double."""
    T = [float(v) for v in T]
    R = [T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]
    return normalize(quat_from_R(R)), [T[3], T[7], T[11]]


def mat3(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257): u = (omega, upsilon)."""
    o, up = u[0:3], u[3:6]
    theta = fsqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    Om = [0.0, -o[2], o[1], o[2], 0.0, -o[0], -o[1], o[0], 0.0]
    Om2 = mat3(Om, Om)
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if theta < 0.00001:
        R = [(I[k] + Om[k]) + Om2[k] for k in range(9)]
        V = R
    else:
        s, c = det_sincos64(theta)
        a = s / theta
        b = (1.0 - c) / (theta * theta)
        d = (theta - s) / (theta * theta * theta)
        R = [(I[k] + a * Om[k]) + b * Om2[k] for k in range(9)]
        V = [(I[k] + b * Om[k]) + d * Om2[k] for k in range(9)]
    t = [(V[3 * i] * up[0] + V[3 * i + 1] * up[1]) + V[3 * i + 2] * up[2] for i in range(3)]
    return normalize(quat_from_R(R)), t


def se3_mul(a, b):
    """SE3Quat::operator* (:104-110)."""
    r = quat_rot(a[0], b[1])
    t = [a[1][0] + r[0], a[1][1] + r[1], a[1][2] + r[2]]
    return normalize(quat_mul(a[0], b[0])), t


# ---- edges --------------------------------------------------------------------------------------------------------------
class Edge:
    __slots__ = ("slot", "X", "obs", "stereo", "inv", "delta", "dsqr", "thr")


def edge_error(e, pose, cam):
    """computeError + chi2: (error vector, chi2)."""
    fx, fy, cx, cy, bf = cam
    r = quat_rot(pose[0], e.X)
    P = [r[0] + pose[1][0], r[1] + pose[1][1], r[2] + pose[1][2]]
    if e.stereo:
        invz = f32(fdiv(1.0, P[2]))                                   # types_six_dof_expmap.cpp:300: a float
        p0 = P[0] * invz * fx + cx
        p1 = P[1] * invz * fy + cy
        err = [e.obs[0] - p0, e.obs[1] - p1, e.obs[2] - (p0 - bf * invz)]
    else:
        err = [e.obs[0] - (fdiv(P[0], P[2]) * fx + cx), e.obs[1] - (fdiv(P[1], P[2]) * fy + cy)]
    chi2 = 0.0
    for v in err:
        chi2 = chi2 + v * (e.inv * v)
    return err, chi2, P


def robustify(e, chi2, kernel):
    """(rho[0], rho[1]) of RobustKernelHuber::robustify; no kernel: (chi2, 1)."""
    if not kernel or chi2 <= e.dsqr:
        return chi2, 1.0
    s = fsqrt(chi2)
    return 2 * s * e.delta - e.dsqr, fdiv(e.delta, s)


def edge_terms(e, pose, cam, kernel, full):
    """The 28 addends of one edge: 21 of H (upper triangle, row by row), 6 of b, rho[0]."""
    fx, fy, cx, cy, bf = cam
    err, chi2, P = edge_error(e, pose, cam)
    rho0, rho1 = robustify(e, chi2, kernel)
    if not full:
        return [0.0] * 27 + [rho0]
    x, y = P[0], P[1]
    invz = fdiv(1.0, P[2])
    invz_2 = invz * invz
    J = [[x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, 0.0, x * invz_2 * fx],
         [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, 0.0, -invz * fy, y * invz_2 * fy]]
    if e.stereo:
        J.append([J[0][0] - bf * y * invz_2, J[0][1] + bf * x * invz_2, J[0][2], J[0][3], 0.0, J[0][5] - bf * invz_2])
    w = rho1 * e.inv
    out = []
    for a in range(6):
        for b in range(a, 6):
            s = 0.0
            for r in range(len(J)):
                s = s + (J[r][a] * w) * J[r][b]
            out.append(s)
    for a in range(6):
        s = 0.0
        for r in range(len(J)):
            s = s + J[r][a] * (w * err[r])
        out.append(-s)
    out.append(rho0)
    return out


def team_sum(edges, out, fn, team):
    """The stated order: lanes, butterfly inside a wavefront, wavefronts in order."""
    lanes = [[0.0] * 28 for _ in range(team)]
    for j, e in enumerate(edges):
        if out[j]:
            continue
        acc = lanes[j % team]
        for k, v in enumerate(fn(e)):
            acc[k] = acc[k] + v
    total = None
    for w0 in range(0, team, WAVE):
        wave = lanes[w0:w0 + WAVE]
        for off in (1, 2, 4, 8, 16, 32):
            wave = [[wave[l][k] + wave[l ^ off][k] for k in range(28)] for l in range(WAVE)]
        total = wave[0] if total is None else [total[k] + wave[0][k] for k in range(28)]
    return total


# ---- the 6x6 solve ------------------------------------------------------------------------------------------------------
def ldlt_solve(H, b):
    """Pivoted LDLt of the full symmetric 6x6 H (list of rows): (ok, x).  ok iff every pivot > 0."""
    A = [row[:] for row in H]
    tr = [0] * 6
    for k in range(6):
        p = k
        for i in range(k + 1, 6):
            if abs(A[i][i]) > abs(A[p][p]):
                p = i
        tr[k] = p
        if p != k:
            A[k], A[p] = A[p], A[k]
            for r in range(6):
                A[r][k], A[r][p] = A[r][p], A[r][k]
        d = A[k][k]
        if not (d > 0):
            return False, None
        for i in range(k + 1, 6):
            l = A[i][k] / d
            for j in range(k + 1, i + 1):
                A[i][j] = A[i][j] - l * A[j][k]
                A[j][i] = A[i][j]
        for i in range(k + 1, 6):
            A[i][k] = A[i][k] / d
    y = b[:]
    for k in range(6):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(6):
        for j in range(i):
            y[i] = y[i] - A[i][j] * y[j]
    for i in range(6):
        y[i] = y[i] / A[i][i]
    for i in range(5, -1, -1):
        for j in range(i + 1, 6):
            y[i] = y[i] - A[j][i] * y[j]
    for k in range(5, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


def unpack_H(s):
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[a][b] = H[b][a] = s[k]
            k += 1
    return H


# ---- Levenberg-Marquardt: SparseOptimizer::optimize(10) over OptimizationAlgorithmLevenberg::solve ---------------------
class Solver:
    def __init__(self):
        # the solver's x: a failed factorisation leaves it stale.  Before the first success the reference's value is
        # indeterminate (a release build of g2o does not clear the vector); zero is this restatement's choice
        self.x = [0.0] * 6
        self.trace = []             # (round, iteration, trial, accepted) for the tests


def optimize(S, edges, out, pose, cam, kernel, team, rnd):
    """Returns (estimate, last tried estimate, iterations run)."""
    est = pose
    tried = pose
    lam = ni = 0.0
    n_bad = 0
    its = 0
    for it in range(10):
        s = team_sum(edges, out, lambda e: edge_terms(e, est, cam, kernel, True), team)
        H, b = unpack_H(s), s[21:27]
        current = ini = s[27]
        if it == 0:
            mx = 0.0
            for j in range(6):
                a = abs(H[j][j])
                mx = mx if a < mx else a                                # std::max(fabs(h), maxDiagonal)
            lam = 1e-5 * mx
            ni = 2.0
            n_bad = 0
        rho = 0.0
        qmax = 0
        while True:
            backup = est
            A = [row[:] for row in H]
            for j in range(6):
                A[j][j] = H[j][j] + lam
            ok2, x = ldlt_solve(A, b)
            if ok2:
                S.x = x
            est = tried = se3_mul(se3_exp(S.x), est)
            temp = team_sum(edges, out, lambda e: edge_terms(e, est, cam, kernel, False), team)[27]
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(6):
                scale = scale + S.x[j] * (lam * S.x[j] + b[j])
            scale = scale + 1e-3
            rho = fdiv(rho, scale)
            good = rho > 0 and math.isfinite(temp)
            S.trace.append((rnd, it, qmax, good))
            if good:
                y = 2 * rho - 1
                alpha = 1.0 - (y * y) * y
                alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha          # std::min(alpha, 2/3)
                sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0             # std::max(1/3, alpha)
                lam = lam * sf
                ni = 2.0
                current = temp
            else:
                lam = lam * ni
                ni = ni * 2
                est = backup
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        its += 1
        if qmax == 10 or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:
            break
    return est, tried, its


# ---- the function and the loops of Tracking that follow it --------------------------------------------------------------
def build_edges(kx, ky, koct, n, u_right, world, inv_level_sigma2, frame_point):
    """:280-360: the slots i < n with a point, in slot order, monocular and stereo interleaved."""
    d_mono, d_stereo = f32(math.sqrt(5.991)), f32(math.sqrt(7.815))
    edges = []
    for i in range(n):
        p = int(frame_point[i])
        if p < 0:
            continue
        e = Edge()
        e.slot = i
        e.X = [float(world[p][0]), float(world[p][1]), float(world[p][2])]
        e.stereo = u_right is not None and not (float(u_right[i]) < 0)          # :286
        e.obs = [float(kx[i]), float(ky[i])] + ([float(u_right[i])] if e.stereo else [])
        e.inv = float(np.float32(inv_level_sigma2[int(koct[i])]))
        e.delta = d_stereo if e.stereo else d_mono
        e.dsqr = e.delta * e.delta
        e.thr = f32(7.815) if e.stereo else f32(5.991)
        edges.append(e)
    return edges


def classify(edges, out, est, tried, cam):
    """:382-438: an inlier edge keeps the _error the last computeActiveErrors left (the last TRIED estimate, accepted or
    not), an outlier edge is recomputed at the estimate (:390).  chi2 is rounded to float, the comparison is strict."""
    new, n_bad = [], 0
    for j, e in enumerate(edges):
        chi2 = edge_error(e, est if out[j] else tried, cam)[1]
        bad = f32(chi2) > e.thr
        new.append(bad)
        n_bad += 1 if bad else 0
    return new, n_bad


def pose_optimization(kx, ky, koct, n, u_right, world, point_flags, inv_level_sigma2, cam, Tcw, frame_point, outlier,
                      discarded=None, mode=PLAIN, flags=0, team=TEAM, trace=None, pose64=None, history=None, last64=None):
    """One frame.  kx, ky, koct [cap]; u_right [cap] or None; world [pcap][3] and point_flags [pcap]: the frame's world row;
    cam = (fx, fy, cx, cy, bf) as floats.  Tcw [12], frame_point [cap], outlier [cap], discarded [cap] or None are numpy
    arrays modified in place.  Returns report [8].  trace / pose64 / history / last64: lists that receive the trials, the pose
    in double, the outlier flags of the edges after each round, and the last round's estimate and last tried estimate
    (2 x (quaternion x y z w, t))."""
    cam = tuple(float(np.float32(v)) for v in cam)
    edges = build_edges(kx, ky, koct, n, u_right, world, inv_level_sigma2, frame_point)
    for e in edges:
        outlier[e.slot] = 0                                                     # :289, :323
    n_init = len(edges)
    status, n_bad, rounds, its_total = OK, 0, 0, 0
    if n_init < 3:                                                              # :364
        status = TOO_FEW
        ret = 0
    else:
        pose0 = pose_from_Tcw(Tcw)
        out = [False] * n_init
        S = Solver()
        est = pose0
        for rnd in range(4):
            est, tried, its = optimize(S, edges, out, pose0, cam, rnd < 3, team, rnd)   # :377: from the input pose
            its_total += its
            out, n_bad = classify(edges, out, est, tried, cam)
            if history is not None:
                history.append(list(out))
            rounds += 1
            if n_init < 10:                                                     # :440
                status = ONE_ROUND
                break
        for j, e in enumerate(edges):
            outlier[e.slot] = 1 if out[j] else 0
        R = to_R(est[0])
        T = [R[0], R[1], R[2], est[1][0], R[3], R[4], R[5], est[1][1], R[6], R[7], R[8], est[1][2]]
        for k in range(12):
            Tcw[k] = np.float32(T[k])
        ret = n_init - n_bad
        if trace is not None:
            trace.extend(S.trace)
        if pose64 is not None:
            pose64.extend(T)
        if last64 is not None:
            last64.extend(est[0] + est[1] + tried[0] + tried[1])
    count_a = count_b = 0
    if mode != PLAIN:
        for i in range(n):
            p = int(frame_point[i])
            if discarded is not None:
                discarded[i] = -1
            if p < 0:
                continue
            observed = bool(int(point_flags[p]) & POINT_OBSERVED)
            if mode == DISCARD:
                if outlier[i]:
                    frame_point[i] = -1
                    outlier[i] = 0
                    if discarded is not None:
                        discarded[i] = p
                else:
                    count_a += 1
                    if observed:
                        count_b += 1
            else:
                if not outlier[i]:
                    count_b += 1
                    if (flags & ONLY_TRACKING) or observed:
                        count_a += 1
                elif flags & STEREO:
                    frame_point[i] = -1
                    if discarded is not None:
                        discarded[i] = p
    return [status, n_init, n_bad, ret, rounds, its_total, count_a, count_b]
