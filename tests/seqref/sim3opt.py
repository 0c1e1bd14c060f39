"""Sequential reference of Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241), written from the reference text.

One Sim3 vertex, fixed points, a pair of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ per correspondence
(types_seven_dof_expmap.h), g2o::Sim3 (sim3.h), the numeric Jacobian of base_binary_edge.hpp:131-205, g2o's
Levenberg-Marquardt (optimization_algorithm_levenberg.cpp) and the dense 7x7 solve.  Plain Python floats: every operation
is one IEEE double operation, in the order written here.  What the reference leaves to Eigen, libm or the summation order
of a sequential loop is restated with a stated order:

  - sums over pairs: pair j of the compacted list belongs to lane j mod TEAM, within a pair e12 comes before e21, a lane
    adds its pairs in ascending j starting from 0.0, removed pairs add nothing; the lanes of a wavefront of 64 are combined
    by an xor butterfly (offsets 1, 2, 4, 8, 16, 32), the wavefronts of the team are then added in wavefront order;
  - exp: det_exp64 (fdlibm's __ieee754_exp); sin / cos: det_sincos64 of seqref/poseopt.py;
  - the 7x7 solve: a pivoted LDLt, largest |d| first, the first of equals;
  - Eigen's quaternion formulas, as seqref/poseopt.py restates them; g2o::Sim3 never normalises its quaternion.
"""
import math

import numpy as np

from .poseopt import DBL_MAX, WAVE, det_sincos64, f32, fdiv, fsqrt, mat3, quat_from_R, quat_mul, quat_rot, to_R
from .sim3 import MATCH_SLOTS, POINT_PRESENT, _row_dot, index_in_key_frame

TEAM = 256
OK, TOO_FEW, SKIPPED = range(3)
DELTA = 1e-9                                    # base_binary_edge.hpp:147-148
SCALAR = 1.0 / (2 * DELTA)
NSUM = 36

# ---- det_exp64 ----------------------------------------------------------------------------------------------------------
EXP_OVER, EXP_UNDER = 7.09782712893383973096e+02, -7.45133219101941108420e+02
LN2_HI, LN2_LO, INV_LN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
EP1, EP2, EP3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
EP4, EP5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
HALF_LN2, THREE_HALF_LN2 = 3.4657359027997264e-01, 1.0397207708399179e+00
EXP_TINY = 3.7252902984619140625e-09            # 2^-28
TWO_M1000 = 9.33263618503218878990e-302


def det_exp64(x):
    """fdlibm's __ieee754_exp with the thresholds written as doubles."""
    if x != x:
        return x
    if x > EXP_OVER:
        return float("inf")
    if x < EXP_UNDER:
        return 0.0
    hi = lo = 0.0
    k = 0
    ax = abs(x)
    if ax > HALF_LN2:
        if ax < THREE_HALF_LN2:
            if x < 0:
                hi, lo, k = x + LN2_HI, -LN2_LO, -1
            else:
                hi, lo, k = x - LN2_HI, LN2_LO, 1
        else:
            k = int(INV_LN2 * x + (-0.5 if x < 0 else 0.5))
            t = float(k)
            hi = x - t * LN2_HI
            lo = t * LN2_LO
        x = hi - lo
    elif ax < EXP_TINY:
        return 1.0 + x
    t = x * x
    c = x - t * (EP1 + t * (EP2 + t * (EP3 + t * (EP4 + t * EP5))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    if k == 1024:
        return y * 2.0 * math.ldexp(1.0, 1023)
    if k >= -1021:
        return y * math.ldexp(1.0, k)
    return y * math.ldexp(1.0, k + 1000) * TWO_M1000


# ---- g2o::Sim3: S = [qx, qy, qz, qw, tx, ty, tz, s] ---------------------------------------------------------------------
def from_sim3(m):
    """Sim3(toMatrix3d(R), toVector3d(t), s) of the [16] float record: the floats widen to double."""
    m = [float(v) for v in m]
    return quat_from_R(m[0:9]) + m[9:12] + [m[12]]


def sim3_exp(u):
    """Sim3(const Vector7d &update) (sim3.h:70-142): u = (omega, upsilon, sigma)."""
    o, up, sigma = u[0:3], u[3:6], u[6]
    theta = fsqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    Om = [0.0, -o[2], o[1], o[2], 0.0, -o[0], -o[1], o[0], 0.0]
    Om2 = mat3(Om, Om)
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    s = det_exp64(sigma)
    eps = 0.00001
    small = theta < eps
    sn = cs = 0.0
    if small:
        R = [(I[k] + Om[k]) + Om2[k] for k in range(9)]
    else:
        sn, cs = det_sincos64(theta)
        a = fdiv(sn, theta)
        b = fdiv(1.0 - cs, theta * theta)
        R = [(I[k] + a * Om[k]) + b * Om2[k] for k in range(9)]
    if abs(sigma) < eps:
        C = 1.0
        if small:
            A = 1. / 2.
            B = 1. / 6.
        else:
            theta2 = theta * theta
            A = fdiv(1.0 - cs, theta2)
            B = fdiv(theta - sn, theta2 * theta)
    else:
        C = fdiv(s - 1.0, sigma)
        if small:
            sigma2 = sigma * sigma
            A = fdiv((sigma - 1.0) * s + 1.0, sigma2)
            B = fdiv((0.5 * sigma2 - sigma + 1.0) * s, sigma2 * sigma)
        else:
            a, b = s * sn, s * cs
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = fdiv(a * sigma + (1.0 - b) * theta, theta * c)
            B = fdiv(C - fdiv((b - 1.0) * sigma + a * theta, c), theta2)
    W = [(A * Om[k] + B * Om2[k]) + C * I[k] for k in range(9)]
    t = [(W[3 * i] * up[0] + W[3 * i + 1] * up[1]) + W[3 * i + 2] * up[2] for i in range(3)]
    return quat_from_R(R) + t + [s]


def sim3_mul(a, b):
    """operator* (:266-272)."""
    r = quat_rot(a[0:4], b[4:7])
    return quat_mul(a[0:4], b[0:4]) + [a[7] * r[0] + a[4], a[7] * r[1] + a[5], a[7] * r[2] + a[6], a[7] * b[7]]


def sim3_inverse(S):
    """inverse (:233-236)."""
    q = [-S[0], -S[1], -S[2], S[3]]
    m = fdiv(-1., S[7])
    return q + quat_rot(q, [m * S[4], m * S[5], m * S[6]]) + [fdiv(1., S[7])]


# ---- the two edges ------------------------------------------------------------------------------------------------------
def edge_error(S, X, obs, cam):
    """obs - cam_map(project(S.map(X)))."""
    fx, fy, cx, cy = cam
    r = quat_rot(S[0:4], X)
    m0, m1, m2 = S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]
    return [obs[0] - (fdiv(m0, m2) * fx + cx), obs[1] - (fdiv(m1, m2) * fy + cy)]


def chi2_of(e, inv):
    c = 0.0
    c = c + e[0] * (inv * e[0])
    c = c + e[1] * (inv * e[1])
    return c


def huber(chi2, delta, dsqr):
    """(rho[0], rho[1]) of RobustKernelHuber::robustify."""
    if chi2 <= dsqr:
        return chi2, 1.0
    s = fsqrt(chi2)
    return 2 * s * delta - dsqr, fdiv(delta, s)


def edge_terms(E, X, obs, inv, cam, delta, dsqr, acc):
    """Adds the 36 terms of one edge to acc.  E[2d], E[2d + 1]: Sim3(+-delta e_d) * estimate, E[14]: the estimate (for
    e21: their inverses)."""
    e = edge_error(E[14], X, obs, cam)
    rho0, rho1 = huber(chi2_of(e, inv), delta, dsqr)
    acc[35] = acc[35] + rho0
    J0, J1 = [], []
    for d in range(7):
        ep = edge_error(E[2 * d], X, obs, cam)
        em = edge_error(E[2 * d + 1], X, obs, cam)
        J0.append(SCALAR * (ep[0] - em[0]))
        J1.append(SCALAR * (ep[1] - em[1]))
    w = rho1 * inv
    we0, we1 = w * e[0], w * e[1]
    k = 0
    for a in range(7):
        for b in range(a, 7):
            s = 0.0
            s = s + (J0[a] * w) * J0[b]
            s = s + (J1[a] * w) * J1[b]
            acc[k] = acc[k] + s
            k += 1
    for a in range(7):
        s = 0.0
        s = s + J0[a] * we0
        s = s + J1[a] * we1
        acc[28 + a] = acc[28 + a] + -s


class Pair:
    __slots__ = ("slot", "p2", "i2", "P1", "P2", "o1", "o2", "inv1", "inv2")


def team_sum(pairs, out, fn, team):
    """The stated order: lanes, butterfly inside a wavefront, wavefronts in order.  fn(pair, acc) adds a pair's terms."""
    lanes = [[0.0] * NSUM for _ in range(team)]
    for j, p in enumerate(pairs):
        if not out[j]:
            fn(p, lanes[j % team])
    # the butterfly and the pass over the wavefronts as float64 array additions: the same IEEE additions, lane by lane
    total = None
    idx = np.arange(WAVE)
    with np.errstate(invalid="ignore", over="ignore"):
        for w0 in range(0, team, WAVE):
            wave = np.array(lanes[w0:w0 + WAVE], np.float64)
            for off in (1, 2, 4, 8, 16, 32):
                wave = wave + wave[idx ^ off]
            total = wave[0] if total is None else total + wave[0]
    return [float(v) for v in total]


# ---- the 7x7 solve ------------------------------------------------------------------------------------------------------
def ldlt_solve(H, b):
    """Pivoted LDLt of the full symmetric H (list of rows): (ok, x).  ok iff every pivot > 0."""
    N = len(b)
    A = [row[:] for row in H]
    tr = [0] * N
    for k in range(N):
        p = k
        for i in range(k + 1, N):
            if abs(A[i][i]) > abs(A[p][p]):
                p = i
        tr[k] = p
        if p != k:
            A[k], A[p] = A[p], A[k]
            for r in range(N):
                A[r][k], A[r][p] = A[r][p], A[r][k]
        d = A[k][k]
        if not (d > 0):
            return False, None
        for i in range(k + 1, N):
            l = fdiv(A[i][k], d)
            for j in range(k + 1, i + 1):
                A[i][j] = A[i][j] - l * A[j][k]
                A[j][i] = A[i][j]
        for i in range(k + 1, N):
            A[i][k] = fdiv(A[i][k], d)
    y = b[:]
    for k in range(N):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(N):
        for j in range(i):
            y[i] = y[i] - A[i][j] * y[j]
    for i in range(N):
        y[i] = fdiv(y[i], A[i][i])
    for i in range(N - 1, -1, -1):
        for j in range(i + 1, N):
            y[i] = y[i] - A[j][i] * y[j]
    for k in range(N - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


def unpack_H(s):
    H = [[0.0] * 7 for _ in range(7)]
    k = 0
    for a in range(7):
        for b in range(a, 7):
            H[a][b] = H[b][a] = s[k]
            k += 1
    return H


# ---- Levenberg-Marquardt: SparseOptimizer::optimize(max_it) over OptimizationAlgorithmLevenberg::solve ------------------
class Solver:
    def __init__(self):
        # the solver's x: a failed factorisation leaves it stale; zero before the first success (see seqref/poseopt.py)
        self.x = [0.0] * 7
        self.trace = []             # (round, iteration, trial, accepted)


def linearisation(est, fix_scale):
    """The 15 estimates of a linearisation and their inverses: computed once, every edge reads them."""
    E = []
    for d in range(7):
        for v in (DELTA, -DELTA):
            u = [0.0] * 7
            u[d] = v
            if fix_scale:
                u[6] = 0.0                                                      # VertexSim3Expmap::oplusImpl
            E.append(sim3_mul(sim3_exp(u), est))
    E.append(est)
    return E, [sim3_inverse(S) for S in E]


def optimize(S, pairs, out, est, cam, delta, dsqr, fix_scale, team, max_it, rnd):
    """Returns (estimate, last tried estimate, iterations run)."""
    tried = est
    lam = ni = 0.0
    n_bad = 0
    its = 0

    def full(E, Ei):
        def fn(p, acc):
            edge_terms(E, p.P2, p.o1, p.inv1, cam, delta, dsqr, acc)
            edge_terms(Ei, p.P1, p.o2, p.inv2, cam, delta, dsqr, acc)
        return fn

    def trial(T, Ti):
        def fn(p, acc):
            acc[35] = acc[35] + huber(chi2_of(edge_error(T, p.P2, p.o1, cam), p.inv1), delta, dsqr)[0]
            acc[35] = acc[35] + huber(chi2_of(edge_error(Ti, p.P1, p.o2, cam), p.inv2), delta, dsqr)[0]
        return fn

    for it in range(max_it):
        E, Ei = linearisation(est, fix_scale)
        s = team_sum(pairs, out, full(E, Ei), team)
        H, b = unpack_H(s), s[28:35]
        current = ini = s[35]
        if it == 0:
            mx = 0.0
            for j in range(7):
                a = abs(H[j][j])
                mx = mx if a < mx else a                                        # std::max(fabs(h), maxDiagonal)
            lam = 1e-5 * mx
            ni = 2.0
            n_bad = 0
        rho = 0.0
        qmax = 0
        while True:
            backup = est
            A = [row[:] for row in H]
            for j in range(7):
                A[j][j] = H[j][j] + lam
            ok2, x = ldlt_solve(A, b)
            if ok2:
                S.x = x
            if fix_scale:
                S.x[6] = 0.0                                                    # oplusImpl writes into the solver's vector
            est = tried = sim3_mul(sim3_exp(S.x), est)
            temp = team_sum(pairs, out, trial(est, sim3_inverse(est)), team)[35]
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(7):
                scale = scale + S.x[j] * (lam * S.x[j] + b[j])
            scale = scale + 1e-3
            rho = fdiv(rho, scale)
            good = rho > 0 and math.isfinite(temp)
            S.trace.append((rnd, it, qmax, good))
            if good:
                y = 2 * rho - 1
                alpha = 1.0 - (y * y) * y
                alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha              # std::min(alpha, 2/3)
                sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0                 # std::max(1/3, alpha)
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


# ---- the function -------------------------------------------------------------------------------------------------------
def build_pairs(T, cur, kf, matched12, match_form, inv_level_sigma2):
    """:1099-1178: the kept slots i < n[cur] in slot order."""
    T1 = np.asarray(T["Tcw"][cur], np.float32).reshape(3, 4)
    T2 = np.asarray(T["Tcw"][kf], np.float32).reshape(3, 4)
    pairs = []
    for i in range(int(T["n"][cur])):
        m = int(matched12[i])
        if m < 0:
            continue
        p2 = int(T["slot_point"][kf][m]) if match_form == MATCH_SLOTS else m
        p1 = int(T["slot_point"][cur][i])
        if p1 < 0 or p2 < 0:
            continue
        if not (T["flags"][p1] & POINT_PRESENT) or not (T["flags"][p2] & POINT_PRESENT):
            continue
        i2 = index_in_key_frame(T, p2, kf)
        if i2 < 0:
            continue
        p = Pair()
        p.slot, p.p2, p.i2 = i, p2, i2
        with np.errstate(invalid="ignore", over="ignore"):
            p.P1 = [float(_row_dot(T1, r, T["world"][p1])) for r in range(3)]
            p.P2 = [float(_row_dot(T2, r, T["world"][p2])) for r in range(3)]
        k1, k2 = T["kps"][cur][i], T["kps"][kf][i2]
        p.o1 = [float(k1["x"]), float(k1["y"])]
        p.o2 = [float(k2["x"]), float(k2["y"])]
        p.inv1 = float(np.float32(inv_level_sigma2[int(k1["octave"])]))
        p.inv2 = float(np.float32(inv_level_sigma2[int(k2["octave"])]))
        pairs.append(p)
    return pairs


def classify(pairs, out, tried, cam, th2):
    """:1186-1203 / :1220-1234: chi2() reads the _error of the last computeActiveErrors, i.e. at the last TRIED estimate,
    accepted or not.  double > (double)th2, strict; a NaN is not greater.  Returns the indices newly bad."""
    ti = sim3_inverse(tried)
    bad = []
    for j, p in enumerate(pairs):
        if out[j]:
            continue
        c12 = chi2_of(edge_error(tried, p.P2, p.o1, cam), p.inv1)
        c21 = chi2_of(edge_error(ti, p.P1, p.o2, cam), p.inv2)
        if c12 > th2 or c21 > th2:
            bad.append(j)
    return bad


def scw_of(est, Tkf):
    """Converter::toCvMat(gScm * gSmw), gSmw = Sim3(R2w, t2w, 1.0) (src/LoopClosing.cc:333-335): [12] floats."""
    T2 = [float(v) for v in np.asarray(Tkf, np.float32).reshape(12)]
    mw = quat_from_R([T2[0], T2[1], T2[2], T2[4], T2[5], T2[6], T2[8], T2[9], T2[10]]) + [T2[3], T2[7], T2[11], 1.0]
    cw = sim3_mul(est, mw)
    R = to_R(cw[0:4])
    out = []
    for r in range(3):
        out += [f32(cw[7] * R[3 * r + c]) for c in range(3)] + [f32(cw[4 + r])]
    return np.array(out, np.float32)


def optimize_sim3(T, cur, kf, cam, matched12, match_form, inv_level_sigma2, sim3, th2=10.0, fix_scale=False, team=TEAM,
                  info=None):
    """One candidate.  T: the tables of seqref/sim3.py (kps are read for x, y and octave); cam = (fx, fy, cx, cy);
    matched12 [cap] int32 is modified in place; sim3 [16] float32.  Returns (report [8], S12 [8] float64, Scw [12] float32
    or None on the early return).  info (a dict) receives trace, pairs, history, est, tried."""
    cam = tuple(float(np.float32(v)) for v in cam)
    th2f = np.float32(th2)
    delta = float(np.sqrt(th2f))                                                # :1095: const float deltaHuber = sqrt(th2)
    dsqr = delta * delta
    th2d = float(th2f)
    pairs = build_pairs(T, cur, kf, matched12, match_form, inv_level_sigma2)
    ne = len(pairs)
    est0 = from_sim3(sim3)
    est = tried = est0
    out = [False] * ne
    S = Solver()
    n_bad = its1 = its2 = 0
    history = []
    if ne > 0:
        est, tried, its1 = optimize(S, pairs, out, est, cam, delta, dsqr, fix_scale, team, 5, 0)        # :1182
        bad = classify(pairs, out, tried, cam, th2d)
        for j in bad:
            out[j] = True
            matched12[pairs[j].slot] = -1
        n_bad = len(bad)
        history.append(list(out))
    if info is not None:
        info.update(trace=S.trace, pairs=pairs, history=history)
    if ne - n_bad < 10:                                                         # :1211: g2oS12 stays what it was
        if info is not None:
            info.update(est=est, tried=tried)
        return np.array([TOO_FEW, ne, n_bad, 0, its1, 0, 0, 0], np.int32), np.array(est0, np.float64), None
    est, tried, its2 = optimize(S, pairs, out, est, cam, delta, dsqr, fix_scale, team, 10 if n_bad > 0 else 5, 1)
    bad = classify(pairs, out, tried, cam, th2d)
    for j in bad:
        out[j] = True
        matched12[pairs[j].slot] = -1
    history.append(list(out))
    n_in = ne - n_bad - len(bad)
    if info is not None:
        info.update(est=est, tried=tried)
    return (np.array([OK, ne, n_bad, n_in, its1, its2, 0, 0], np.int32), np.array(est, np.float64), scw_of(est, T["Tcw"][kf]))
