"""Sequential reference of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778), written from the reference text.

The three lists, one SE3 vertex per listed key frame, one point vertex per local point, EdgeSE3ProjectXYZ /
EdgeStereoSE3ProjectXYZ with both Jacobians (types_six_dof_expmap.cpp:103-139, :188-234), constructQuadraticForm
(base_binary_edge.hpp:55-120), g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:61-189) over
BlockSolver_6_3::solve (block_solver.hpp:354-486), the level-1 rule, the final check and the write-back.  Plain Python
floats: every operation is one IEEE double operation, in the order written here.  The quaternion algebra, det_sincos64 and
the edge error are tests/seqref/poseopt.py's, imported.  What the reference leaves to Eigen, to a sparse solver or to the
order of a sequential loop is restated with a stated order:

  - a point's Hll and b_l: its edges in creation order, added from 0.0; level-1 edges add nothing;
  - a free pose's Hpp and b_p, and the Schur block of a pair (i1 <= i2): entry k of the pose's edge list (all its edges,
    ascending) belongs to lane k mod 64, a lane adds its entries in ascending k from 0.0, the 64 lanes meet in an xor
    butterfly (offsets 1 .. 32), which for lane 0 is the pairwise tree ((l0 + l1) + (l2 + l3)) + ...;
  - the robust chi2, the largest diagonal and computeScale: item t (edge t; or entry t of the vector of all free poses, then
    all local points, in or out of the system) belongs to lane t mod 256, a lane takes its items in ascending t, a wavefront
    of 64 meets in the same tree, the four wavefronts are combined in order; items outside the system are skipped;
  - Dinv: cofactors over the determinant; the poses of the Schur system in list order; its factorisation an unpivoted LDLt
    in index order, ok iff every pivot is > 0, forward substitution column by column, back substitution from the last
    column; the solver's x is zero when a round begins and stale after a failed factorisation.
"""
import math

import numpy as np

from .poseopt import DBL_MAX, Edge, edge_error, f32, fdiv, pose_from_Tcw, quat_rot, robustify, se3_exp, se3_mul, to_R

MAX_LOCAL = 128
TEAM, WAVE = 256, 64
OK, STOPPED, ONE_ROUND, CAPACITY = range(4)
POINT_PRESENT = 1


def max2(a, b):
    """std::max(a, b)."""
    return b if a < b else a


def tree(vals, op):
    """Lane 0 of the xor butterfly over len(vals) lanes."""
    while len(vals) > 1:
        vals = [op(vals[i], vals[i + 1]) for i in range(0, len(vals), 2)]
    return vals[0]


def add(a, b):
    return a + b


def team_reduce(items, term, op):
    """items: the indices t that take part, ascending; term(t, acc) -> acc.  Lane t mod 256, tree per wavefront, wavefronts
    in order."""
    lanes = [0.0] * TEAM
    for t in items:
        lanes[t % TEAM] = term(t, lanes[t % TEAM])
    total = None
    for w0 in range(0, TEAM, WAVE):
        v = tree(lanes[w0:w0 + WAVE], op)
        total = v if total is None else op(total, v)
    return total


def wave_sum(entries, width):
    """entries: (k, vector) with k the position in the pose's edge list; returns the `width` sums of lane 0."""
    lanes = [[0.0] * width for _ in range(WAVE)]
    for k, vec in entries:
        acc = lanes[k % WAVE]
        for q in range(width):
            acc[q] = acc[q] + vec[q]
    return [tree([lanes[l][q] for l in range(WAVE)], add) for q in range(width)]


class Stop:
    """pbStopFlag: None (null), a value, or the list of values successive samples return (the last one repeats)."""

    def __init__(self, spec):
        self.spec = spec
        self.samples = 0

    def sample(self):
        if self.spec is None:
            return False
        if isinstance(self.spec, (list, tuple)):
            v = self.spec[min(self.samples, len(self.spec) - 1)]
        else:
            v = self.spec
        self.samples += 1
        return bool(v)


def linearize(e, pose, cam, kernel, free):
    """One active edge at the estimate: chi2, rho[0], and its terms: Hll (6, upper), b_l (3), Hpp (21, upper), b_p (6),
    B (6 x 3: pose row, point column)."""
    fx, fy, cx, cy, bf = cam
    err, chi2, P = edge_error(e, pose, cam)
    rho0, rho1 = robustify(e, chi2, kernel)
    R = to_R(pose[0])
    x, y, z = P
    z_2 = z * z
    Jc = [[fdiv(x * y, z_2) * fx, -(1 + fdiv(x * x, z_2)) * fx, fdiv(y, z) * fx, fdiv(-1.0, z) * fx, 0.0, fdiv(x, z_2) * fx],
          [(1 + fdiv(y * y, z_2)) * fy, fdiv(-x * y, z_2) * fy, fdiv(-x, z) * fy, 0.0, fdiv(-1.0, z) * fy, fdiv(y, z_2) * fy]]
    if e.stereo:
        Jc.append([Jc[0][0] - fdiv(bf * y, z_2), Jc[0][1] + fdiv(bf * x, z_2), Jc[0][2], Jc[0][3], 0.0, Jc[0][5] - fdiv(bf, z_2)])
        Jp = [[fdiv(-fx * R[c], z) + fdiv(fx * x * R[6 + c], z_2) for c in range(3)],
              [fdiv(-fy * R[3 + c], z) + fdiv(fy * y * R[6 + c], z_2) for c in range(3)]]
        Jp.append([Jp[0][c] - fdiv(bf * R[6 + c], z_2) for c in range(3)])
    else:
        m = fdiv(-1.0, z)                                                # -1./z * tmp * R, left to right
        m00, m01, m02 = m * fx, m * 0.0, m * (fdiv(-x, z) * fx)
        m10, m11, m12 = m * 0.0, m * fy, m * (fdiv(-y, z) * fy)
        Jp = [[(m00 * R[c] + m01 * R[3 + c]) + m02 * R[6 + c] for c in range(3)],
              [(m10 * R[c] + m11 * R[3 + c]) + m12 * R[6 + c] for c in range(3)]]
    nr = len(Jc)
    w = rho1 * e.inv                                                     # weightedOmega = rho[1] * omega
    o = [-(e.inv * err[r]) * rho1 for r in range(nr)]                    # omega_r
    Hll, bl, Hpp, bp, B = [], [], [], [], []
    for a in range(3):
        for b in range(a, 3):
            s = 0.0
            for r in range(nr):
                s = s + (Jp[r][a] * w) * Jp[r][b]
            Hll.append(s)
    for a in range(3):
        s = 0.0
        for r in range(nr):
            s = s + Jp[r][a] * o[r]
        bl.append(s)
    if free:
        for a in range(6):
            for b in range(a, 6):
                s = 0.0
                for r in range(nr):
                    s = s + (Jc[r][a] * w) * Jc[r][b]
                Hpp.append(s)
        for a in range(6):
            s = 0.0
            for r in range(nr):
                s = s + Jc[r][a] * o[r]
            bp.append(s)
        for a in range(6):
            for b in range(3):
                s = 0.0
                for r in range(nr):
                    s = s + (Jp[r][b] * w) * Jc[r][a]
                B.append(s)
    return chi2, rho0, Hll, bl, Hpp, bp, B


def inv3(H, lam):
    """(H + lam I)^-1 of the packed symmetric H (00 01 02 11 12 22), packed."""
    d00, d01, d02, d11, d12, d22 = H[0] + lam, H[1], H[2], H[3] + lam, H[4], H[5] + lam
    c00, c01, c02 = d11 * d22 - d12 * d12, d02 * d12 - d01 * d22, d01 * d12 - d02 * d11
    c11, c12, c22 = d00 * d22 - d02 * d02, d01 * d02 - d00 * d12, d00 * d11 - d01 * d01
    det = (d00 * c00 + d01 * c01) + d02 * c02
    return [fdiv(c00, det), fdiv(c01, det), fdiv(c02, det), fdiv(c11, det), fdiv(c12, det), fdiv(c22, det)]


def sym3(D, r, c):
    return D[(0, 1, 2, 1, 3, 4, 2, 4, 5)[3 * r + c]]


def upper21(a, b):
    return a * 6 - a * (a - 1) // 2 + (b - a)


def ldlt_solve(A, b):
    """Unpivoted LDLt of the lower triangle of A (list of rows) in index order: (ok, x)."""
    n = len(b)
    A = [row[:] for row in A]
    for k in range(n):
        d = A[k][k]
        if not (d > 0):
            return False, None
        L = [fdiv(A[i][k], d) for i in range(n)]
        for i in range(k + 1, n):
            for j in range(k + 1, i + 1):
                A[i][j] = A[i][j] - L[i] * A[j][k]
        for i in range(k + 1, n):
            A[i][k] = L[i]
    y = b[:]
    for j in range(n):
        for i in range(j + 1, n):
            y[i] = y[i] - A[i][j] * y[j]
    for i in range(n):
        y[i] = fdiv(y[i], A[i][i])
    for j in range(n - 1, 0, -1):
        for i in range(j):
            y[i] = y[i] - A[j][i] * y[j]
    return True, y


def local_bundle_adjustment(cur, id0_row, cam, tables, inv_level_sigma2, max_points, max_edges, stop=None, trace=None):
    """tables: dict of numpy arrays named as orbhip_lba_tables (kf_bad and u_right may be None).  Returns dict(local_kf,
    fixed_kf, local_point, erase, report, Tcw, world): lists, and copies of the two in/out tables after the call; on
    STOPPED / CAPACITY the lists are None.  trace: a dict that receives est / tried (poses then points) of each round, the (chi2, threshold) pairs both
    checks read (check1, check2) and the edges put to level 1."""
    T = tables
    slot_point, n, kf_bad = T["slot_point"], T["n"], T.get("kf_bad")
    obs_start, obs_kf, obs_idx, flags = T["obs_start"], T["obs_kf"], T["obs_idx"], T["flags"]
    kps, u_right, ord_kf, n_ord = T["kps"], T.get("u_right"), T["ord_kf"], T["n_ord"]
    Tcw, world = np.array(T["Tcw"], np.float32).reshape(-1, 12), np.array(T["world"], np.float32).reshape(-1, 3)
    rows, np_ = len(n), len(obs_start) - 1
    cam = tuple(float(np.float32(v)) for v in cam)
    st = Stop(stop)
    bad = lambda r: kf_bad is not None and bool(kf_bad[r])  # noqa: E731
    report = [0] * 16

    # ---- :456-504: the three lists
    stamp = [0] * rows
    lkf = [cur]
    stamp[cur] = 1
    for i in range(int(n_ord[cur])):
        r = int(ord_kf[cur][i])
        if stamp[r]:
            continue
        stamp[r] = 1
        if not bad(r):
            lkf.append(r)
    lpt, seen = [], set()
    for r in lkf:
        for s in range(int(n[r])):
            p = int(slot_point[r][s])
            if p < 0 or p >= np_ or not (int(flags[p]) & POINT_PRESENT) or p in seen:
                continue
            seen.add(p)
            lpt.append(p)
    free_of = {}
    for r in lkf:
        if r != id0_row:
            free_of[r] = len(free_of)
    nfree = len(free_of)
    report[1], report[3] = len(lkf), len(lpt)

    def finish(status):
        report[0] = status
        report[15] = st.samples
        return dict(local_kf=None, fixed_kf=None, local_point=None, erase=None, report=report, Tcw=Tcw, world=world)

    if nfree > MAX_LOCAL or len(lpt) > max_points:
        return finish(CAPACITY)
    fkf = []
    for p in lpt:
        for o in range(int(obs_start[p]), int(obs_start[p + 1])):
            r = int(obs_kf[o])
            if stamp[r]:
                continue
            stamp[r] = 2
            if not bad(r):
                fkf.append(r)
    report[2] = len(fkf)

    # ---- :520-653: vertices and edges
    d_mono, d_stereo = f32(math.sqrt(5.991)), f32(math.sqrt(7.815))
    vtx_rows = lkf + fkf
    vtx_of = {r: v for v, r in enumerate(vtx_rows)}
    edges = []                                                           # (Edge, vertex, point position, key-point index)
    pt_edges = []
    for i, p in enumerate(lpt):
        mine = []
        for o in range(int(obs_start[p]), int(obs_start[p + 1])):
            r, idx = int(obs_kf[o]), int(obs_idx[o])
            if bad(r):
                continue
            e = Edge()
            e.slot = idx
            e.stereo = u_right is not None and not (float(u_right[r][idx]) < 0)          # :594
            e.obs = [float(kps["x"][r][idx]), float(kps["y"][r][idx])] + ([float(u_right[r][idx])] if e.stereo else [])
            e.inv = float(np.float32(inv_level_sigma2[int(kps["octave"][r][idx])]))
            e.delta = d_stereo if e.stereo else d_mono
            e.dsqr = e.delta * e.delta
            e.thr = 7.815 if e.stereo else 5.991
            mine.append(len(edges))
            edges.append((e, vtx_of[r], i, idx))
        pt_edges.append(mine)
    ne = len(edges)
    report[5] = sum(1 for e in edges if e[0].stereo)
    report[4] = ne - report[5]
    if ne > max_edges:
        return finish(CAPACITY)
    vfree = [free_of.get(r, -1) if v < len(lkf) else -1 for v, r in enumerate(vtx_rows)]
    kf_edges = [[] for _ in range(nfree)]
    for j, (e, v, i, idx) in enumerate(edges):
        if vfree[v] >= 0:
            kf_edges[vfree[v]].append(j)
    est_pose = [pose_from_Tcw(Tcw[r]) for r in vtx_rows]
    est_pt = [[float(world[p][0]), float(world[p][1]), float(world[p][2])] for p in lpt]
    tried_pose, tried_pt = list(est_pose), [x[:] for x in est_pt]
    level1 = [False] * ne
    chi2_of = [0.0] * ne            # _error of an edge before any computeActiveErrors: zero is this restatement's choice
    rho_of = [0.0] * ne

    def errors_at(poses, pts, kernel):
        for j, (e, v, i, idx) in enumerate(edges):
            if level1[j]:
                continue
            e.X = pts[i]
            chi2 = edge_error(e, poses[v], cam)[1]
            chi2_of[j], rho_of[j] = chi2, robustify(e, chi2, kernel)[0]

    def depth_positive(j):
        e, v, i, idx = edges[j]
        return quat_rot(est_pose[v][0], est_pt[i])[2] + est_pose[v][1][2] > 0.0

    def edge_bad(j):
        return chi2_of[j] > edges[j][0].thr or not depth_positive(j)

    def snapshot(rnd):
        if trace is not None:
            trace.setdefault("est", {})[rnd] = [q + t for q, t in est_pose] + [x[:] for x in est_pt]
            trace.setdefault("tried", {})[rnd] = [q + t for q, t in tried_pose] + [x[:] for x in tried_pt]

    its, trials, poses_in = [0, 0], [0, 0], [0, 0]

    def optimize(rnd, iterations, kernel):
        """initializeOptimization(level 0) + optimize(iterations)."""
        nonlocal est_pose, est_pt, tried_pose, tried_pt
        pt_active = [any(not level1[j] for j in pt_edges[i]) for i in range(len(lpt))]
        pose_active = [any(not level1[j] for j in kf_edges[f]) for f in range(nfree)]
        poses_in[rnd] = sum(pose_active)
        if all(level1):                                                  # no vertex to optimise: optimize() returns at once
            return
        act = [f for f in range(nfree) if pose_active[f]]
        col = {f: c for c, f in enumerate(act)}
        xp = [0.0] * (6 * nfree)
        xl = [[0.0] * 3 for _ in lpt]
        lam = ni = 0.0
        n_bad = 0
        np6 = 6 * nfree
        items_e = [j for j in range(ne) if not level1[j]]
        items_v = [t for t in range(np6) if pose_active[t // 6]] + \
                  [np6 + 3 * i + a for i in range(len(lpt)) if pt_active[i] for a in range(3)]
        ok = True
        for it in range(iterations):
            if st.sample() or not ok:                                    # i < iterations && !terminate() && ok
                break
            # computeActiveErrors, buildSystem
            rec = {}
            for j in items_e:
                e, v, i, idx = edges[j]
                e.X = est_pt[i]
                rec[j] = linearize(e, est_pose[v], cam, kernel, vfree[v] >= 0)
                chi2_of[j], rho_of[j] = rec[j][0], rec[j][1]
            Hll, bl = {}, {}
            for i in range(len(lpt)):
                if not pt_active[i]:
                    continue
                H, b = [0.0] * 6, [0.0] * 3
                for j in pt_edges[i]:
                    if level1[j]:
                        continue
                    for q in range(6):
                        H[q] = H[q] + rec[j][2][q]
                    for q in range(3):
                        b[q] = b[q] + rec[j][3][q]
                Hll[i], bl[i] = H, b
            Hpp, bp = {}, {}
            for f in act:
                s = wave_sum([(k, rec[j][4] + rec[j][5]) for k, j in enumerate(kf_edges[f]) if not level1[j]], 27)
                Hpp[f], bp[f] = s[:21], s[21:]
            current = ini = team_reduce(items_e, lambda t, acc: acc + rho_of[t], add)

            def diag(t):
                if t < np6:
                    return Hpp[t // 6][upper21(t % 6, t % 6)]
                i, a = divmod(t - np6, 3)
                return Hll[i][(0, 3, 5)[a]]

            def bvec(t):
                if t < np6:
                    return bp[t // 6][t % 6]
                i, a = divmod(t - np6, 3)
                return bl[i][a]

            def xvec(t):
                if t < np6:
                    return xp[t]
                i, a = divmod(t - np6, 3)
                return xl[i][a]

            if it == 0:
                lam = 1e-5 * team_reduce(items_v, lambda t, acc: max2(abs(diag(t)), acc), max2)
                ni = 2.0
                n_bad = 0
            rho = 0.0
            qmax = 0
            while True:
                # BlockSolver::solve with lambda on both diagonals
                Dinv, db = {}, {}
                for i in Hll:
                    D = inv3(Hll[i], lam)
                    Dinv[i] = D
                    db[i] = [(sym3(D, r, 0) * bl[i][0] + sym3(D, r, 1) * bl[i][1]) + sym3(D, r, 2) * bl[i][2] for r in range(3)]
                m = 6 * len(act)
                A = [[0.0] * m for _ in range(m)]
                bs = [0.0] * m
                for i1 in act:
                    for i2 in act:
                        if i2 < i1:
                            continue
                        ent = []
                        for k, j1 in enumerate(kf_edges[i1]):
                            if level1[j1]:
                                continue
                            pi = edges[j1][2]
                            j2 = j1 if i1 == i2 else next((j for j in pt_edges[pi] if not level1[j] and vfree[edges[j][1]] == i2), None)
                            if j2 is None:
                                continue
                            B1, B2, D = rec[j1][6], rec[j2][6], Dinv[pi]
                            vec = []
                            coef = []
                            for a in range(6):
                                p0, p1, p2 = B1[a * 3], B1[a * 3 + 1], B1[a * 3 + 2]
                                g = [(p0 * sym3(D, 0, c) + p1 * sym3(D, 1, c)) + p2 * sym3(D, 2, c) for c in range(3)]
                                for b in range(6):
                                    vec.append((g[0] * B2[b * 3] + g[1] * B2[b * 3 + 1]) + g[2] * B2[b * 3 + 2])
                                coef.append((p0 * db[pi][0] + p1 * db[pi][1]) + p2 * db[pi][2])
                            ent.append((k, vec + (coef if i1 == i2 else [0.0] * 6)))
                        s = wave_sum(ent, 42)
                        c1, c2 = 6 * col[i1], 6 * col[i2]
                        if i1 == i2:
                            for a in range(6):
                                for b in range(a + 1):
                                    h = Hpp[i1][upper21(b, a)]
                                    if a == b:
                                        h = h + lam
                                    A[c1 + a][c1 + b] = h - s[b * 6 + a]
                                bs[c1 + a] = bp[i1][a] - s[36 + a]
                        else:
                            for a in range(6):
                                for b in range(6):
                                    A[c2 + b][c1 + a] = 0.0 - s[a * 6 + b]
                ok2, x = ldlt_solve(A, bs)
                if ok2:
                    for f in act:
                        xp[6 * f:6 * f + 6] = x[6 * col[f]:6 * col[f] + 6]
                    for i in Hll:                                        # :468-481: Dinv (b_l - B^T x_p)
                        c = bl[i][:]
                        for j in pt_edges[i]:
                            f = vfree[edges[j][1]]
                            if level1[j] or f < 0:
                                continue
                            B = rec[j][6]
                            nx = [-xp[6 * f + a] for a in range(6)]
                            for b in range(3):
                                c[b] = c[b] + (((((B[b] * nx[0] + B[3 + b] * nx[1]) + B[6 + b] * nx[2]) + B[9 + b] * nx[3]) +
                                                B[12 + b] * nx[4]) + B[15 + b] * nx[5])
                        D = Dinv[i]
                        xl[i] = [(sym3(D, r, 0) * c[0] + sym3(D, r, 1) * c[1]) + sym3(D, r, 2) * c[2] for r in range(3)]
                # update: a vertex outside the system keeps its bits
                tried_pose = [se3_mul(se3_exp(xp[6 * vfree[v]:6 * vfree[v] + 6]), est_pose[v])
                              if vfree[v] >= 0 and pose_active[vfree[v]] else est_pose[v] for v in range(len(vtx_rows))]
                tried_pt = [[est_pt[i][a] + xl[i][a] for a in range(3)] if pt_active[i] else est_pt[i] for i in range(len(lpt))]
                errors_at(tried_pose, tried_pt, kernel)
                temp = team_reduce(items_e, lambda t, acc: acc + rho_of[t], add)
                if not ok2:
                    temp = DBL_MAX
                rho = current - temp
                scale = team_reduce(items_v, lambda t, acc: acc + xvec(t) * (lam * xvec(t) + bvec(t)), add)
                scale = scale + 1e-3
                rho = fdiv(rho, scale)
                if rho > 0 and math.isfinite(temp):
                    yy = 2 * rho - 1
                    alpha = 1.0 - (yy * yy) * yy
                    alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                    sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
                    lam = lam * sf
                    ni = 2.0
                    current = temp
                    est_pose, est_pt = tried_pose, tried_pt
                else:
                    lam = lam * ni
                    ni = ni * 2
                qmax += 1
                trials[rnd] += 1
                if not (rho < 0 and qmax < 10 and not st.sample()):
                    break
            its[rnd] += 1
            if qmax == 10 or rho == 0:
                ok = False
                continue
            if (ini - current) * 1e3 < ini:
                n_bad += 1
            else:
                n_bad = 0
            if n_bad >= 3:
                ok = False

    status = OK
    if st.sample():                                                      # :655
        return finish(STOPPED)
    optimize(0, 5, True)
    snapshot(0)
    if st.sample():                                                      # :664
        status = ONE_ROUND
    else:
        if trace is not None:
            trace["check1"] = [(chi2_of[j], edges[j][0].thr) for j in range(ne)]
        for j in range(ne):                                              # :672-702
            if edge_bad(j):
                level1[j] = True
        report[6] = sum(level1)
        if trace is not None:                                            # (row, key point, point, chi2, depth positive) at level 1
            trace["level1"] = [(vtx_rows[edges[j][1]], edges[j][3], lpt[edges[j][2]], chi2_of[j], depth_positive(j))
                               for j in range(ne) if level1[j]]
        optimize(1, 10, False)
    snapshot(1)
    if trace is not None:
        trace["check2"] = [(chi2_of[j], edges[j][0].thr) for j in range(ne)]
    erase = []
    for want in (False, True):                                           # :715-743
        for j, (e, v, i, idx) in enumerate(edges):
            if e.stereo == want and edge_bad(j):
                erase.append([vtx_rows[v], idx, lpt[i]])
    for v, r in enumerate(lkf):                                          # :762-768
        R, t = to_R(est_pose[v][0]), est_pose[v][1]
        M = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
        for k in range(12):
            Tcw[r][k] = np.float32(M[k])
    for i, p in enumerate(lpt):                                          # :771-776
        for k in range(3):
            world[p][k] = np.float32(est_pt[i][k])
    report[0] = status
    report[7] = len(erase)
    report[8], report[9], report[10], report[11] = its[0], trials[0], its[1], trials[1]
    report[12], report[13] = poses_in[0], poses_in[1]
    report[15] = st.samples
    return dict(local_kf=lkf, fixed_kf=fkf, local_point=lpt, erase=erase, report=report, Tcw=Tcw, world=world)
