"""Sequential reference of Optimizer::BundleAdjustment (src/Optimizer.cc:49-237; GlobalBundleAdjustemnt :41-46 is the call with
both lists None) and of the map update of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:676-737), written from the
reference text.

The edge terms, the 3x3 inverse, the dense LDLt, the team sums and the stop byte are tests/seqref/lba.py's, imported unchanged;
this file adds what differs from the local bundle adjustment: the vertices and edges of a whole map, one optimize(iterations)
with or without Huber kernels and no level-1 rule, the write-back of the two modes, and the apply step.  Plain Python floats:
every operation is one IEEE double operation in the order written here; the apply step is numpy float32 scalars, one rounding
per operation.  Stated orders and choices:

  - vertices: the listed rows that are not bad, in list order; the rows with kf_id 0 are fixed; the free poses of the reduced
    system are the vertices in that order with the fixed ones left out;
  - a point's edges: its observations in table order whose row is not bad and has kf_id <= maxKFid; an observation whose row
    passes that test but is not listed is a null vertex in the reference: counted and skipped here, or refused (refuse_null);
    a point left without an edge is removed;
  - every sum order, the solver's stale x and the Levenberg-Marquardt rules are lba.py's;
  - the systems beyond 48 unknowns are factorised by ldlt_solve_rows, which is lba.ldlt_solve with the two inner loops handed to
    numpy (one multiply, one subtract per element, k ascending: the same bits; tests/test_gba_cpu.py compares the two);
  - apply step: Twc of a row is Rwc = Rcw^T, Ow = -Rwc tcw per row ((-a0 x + -a1 y) + -a2 z); a 4x4 product is element by
    element ((a0 b0 + a1 b1) + a2 b2) + a3 b3 over the full rows, the last row 0 0 0 1; all in fp32.
"""
import math

import numpy as np

from .lba import Stop, add, inv3, ldlt_solve, linearize, max2, sym3, team_reduce, upper21, wave_sum
from .poseopt import DBL_MAX, Edge, edge_error, f32, fdiv, pose_from_Tcw, robustify, se3_exp, se3_mul, to_R

MAX_KF = 512
IN_PLACE, STAGED = 0, 1
OK, STOPPED, CAPACITY = range(3)
POINT_PRESENT = 1
SMALL = 48


def ldlt_solve_rows(A, b):
    """lba.ldlt_solve, the trailing update of column k done as one numpy expression: (ok, x)."""
    n = len(b)
    A = np.array(A, np.float64)
    for k in range(n):
        d = A[k, k]
        if not (d > 0):
            return False, None
        c = A[k + 1:, k].copy()
        l = c / d
        prod = np.multiply.outer(l, c)                                   # l_i * c_j, rounded
        A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - prod                     # the upper triangle is never read
        A[k + 1:, k] = l
    y = np.array(b, np.float64)
    for j in range(n):
        y[j + 1:] = y[j + 1:] - A[j + 1:, j] * y[j]
    y = y / np.diag(A)
    for j in range(n - 1, 0, -1):
        y[:j] = y[:j] - A[j, :j] * y[j]
    return True, [float(v) for v in y]


def solve(A, b):
    return ldlt_solve(A, b) if len(b) <= SMALL else ldlt_solve_rows(A, b)


def global_bundle_adjustment(cam, tables, inv_level_sigma2, iterations, robust, mode, max_points, max_edges, kf_list=None,
                             pt_list=None, stop=None, out=None, refuse_null=False, trace=None):
    """tables: dict of numpy arrays named as orbhip_gba_tables (kf_bad and u_right may be None).  out: dict with the caller's
    TcwGBA [rows, 12], posGBA [pcap, 3], kf_mark [rows], pt_mark [pcap], point_list [max_points] (any may be absent: zeros).
    Returns dict(Tcw, world, TcwGBA, posGBA, kf_mark, pt_mark, point_list, report): copies after the call.  trace: a dict that
    receives the accept / reject decisions and the final estimates in double."""
    T = tables
    kf_bad, kf_id = T.get("kf_bad"), T["kf_id"]
    obs_start, obs_kf, obs_idx, flags = T["obs_start"], T["obs_kf"], T["obs_idx"], T["flags"]
    kps, u_right = T["kps"], T.get("u_right")
    Tcw, world = np.array(T["Tcw"], np.float32).reshape(-1, 12), np.array(T["world"], np.float32).reshape(-1, 3)
    rows, np_, pcap = len(kf_id), len(obs_start) - 1, len(flags)
    out = out or {}
    TcwGBA = np.array(out["TcwGBA"], np.float32).reshape(rows, 12) if out.get("TcwGBA") is not None else np.zeros((rows, 12), np.float32)
    posGBA = np.array(out["posGBA"], np.float32).reshape(pcap, 3) if out.get("posGBA") is not None else np.zeros((pcap, 3), np.float32)
    kf_mark = np.array(out["kf_mark"], np.uint8) if out.get("kf_mark") is not None else np.zeros(rows, np.uint8)
    pt_mark = np.array(out["pt_mark"], np.uint8) if out.get("pt_mark") is not None else np.zeros(pcap, np.uint8)
    point_list = np.array(out["point_list"], np.int32) if out.get("point_list") is not None else np.zeros(max_points, np.int32)
    cam = tuple(float(np.float32(v)) for v in cam)
    st = Stop(stop)
    bad = lambda r: kf_bad is not None and bool(kf_bad[r])  # noqa: E731
    report = [0] * 16

    def finish(status):
        report[0] = status
        report[15] = st.samples
        return dict(Tcw=Tcw, world=world, TcwGBA=TcwGBA, posGBA=posGBA, kf_mark=kf_mark, pt_mark=pt_mark, point_list=point_list,
                    report=report)

    # ---- :71-83: the vertices
    kfs = range(rows) if kf_list is None else [int(r) for r in kf_list]
    vtx_rows = [r for r in kfs if 0 <= r < rows and not bad(r)]
    max_kfid = 0
    for r in vtx_rows:
        if int(kf_id[r]) > max_kfid:
            max_kfid = int(kf_id[r])
    report[1] = len(vtx_rows)
    if len(vtx_rows) > MAX_KF:
        return finish(CAPACITY)
    vtx_of = {}
    for v, r in enumerate(vtx_rows):
        vtx_of[r] = v
    vfree, nfree = [], 0
    for r in vtx_rows:
        if int(kf_id[r]) == 0:                                           # setFixed(pKF->mnId == 0)
            vfree.append(-1)
        else:
            vfree.append(nfree)
            nfree += 1
    report[2], report[11] = nfree, 6 * nfree

    # ---- :89-184: the points and their edges
    d_mono, d_stereo = f32(math.sqrt(5.99)), f32(math.sqrt(7.815))
    pts = range(np_) if pt_list is None else [int(p) for p in pt_list]
    lpt, edges, pt_edges = [], [], []
    removed = skipped = null = 0
    for p in pts:
        if p < 0 or p >= np_ or not (int(flags[p]) & POINT_PRESENT):
            continue
        mine = []
        for o in range(int(obs_start[p]), int(obs_start[p + 1])):
            r, idx = int(obs_kf[o]), int(obs_idx[o])
            if bad(r) or int(kf_id[r]) > max_kfid:                       # :109
                skipped += 1
                continue
            if r not in vtx_of:
                if refuse_null:
                    raise ValueError("point %d is observed by row %d, which is not listed: a null vertex" % (p, r))
                null += 1
                continue
            e = Edge()
            e.slot = idx
            e.stereo = u_right is not None and not (float(u_right[r][idx]) < 0)          # :116
            e.obs = [float(kps["x"][r][idx]), float(kps["y"][r][idx])] + ([float(u_right[r][idx])] if e.stereo else [])
            e.inv = float(np.float32(inv_level_sigma2[int(kps["octave"][r][idx])]))
            e.delta = d_stereo if e.stereo else d_mono
            e.dsqr = e.delta * e.delta
            mine.append((e, vtx_of[r], idx))
        if not mine:                                                     # :175-179
            removed += 1
            continue
        i = len(lpt)
        lpt.append(p)
        pt_edges.append(list(range(len(edges), len(edges) + len(mine))))
        edges.extend((e, v, i, idx) for e, v, idx in mine)
    ne = len(edges)
    report[3], report[4], report[7], report[8] = len(lpt), removed, skipped, null
    report[6] = sum(1 for e in edges if e[0].stereo)
    report[5] = ne - report[6]
    if len(lpt) > max_points or ne > max_edges:
        return finish(CAPACITY)
    kf_edges = [[] for _ in range(nfree)]
    for j, (e, v, i, idx) in enumerate(edges):
        if vfree[v] >= 0:
            kf_edges[vfree[v]].append(j)
    est_pose = [pose_from_Tcw(Tcw[r]) for r in vtx_rows]
    est_pt = [[float(world[p][0]), float(world[p][1]), float(world[p][2])] for p in lpt]
    kernel = bool(robust)
    rho_of = [0.0] * ne
    decisions = []

    def errors_at(poses, pts_):
        for j, (e, v, i, idx) in enumerate(edges):
            e.X = pts_[i]
            chi2 = edge_error(e, poses[v], cam)[1]
            rho_of[j] = robustify(e, chi2, kernel)[0]

    its = trials = 0
    status = OK
    if ne > 0:                                                           # no edge: no vertex to optimise, optimize() returns at once
        pose_active = [len(kf_edges[f]) > 0 for f in range(nfree)]
        act = [f for f in range(nfree) if pose_active[f]]
        col = {f: c for c, f in enumerate(act)}
        xp = [0.0] * (6 * nfree)
        xl = [[0.0] * 3 for _ in lpt]
        lam = ni = 0.0
        n_bad = 0
        np6 = 6 * nfree
        items_e = list(range(ne))
        items_v = [t for t in range(np6) if pose_active[t // 6]] + [np6 + t for t in range(3 * len(lpt))]
        ok = True
        for it in range(iterations):
            if st.sample() or not ok:                                    # i < iterations && !terminate() && ok
                if it == 0:
                    status = STOPPED
                break
            rec = {}
            for j in items_e:
                e, v, i, idx = edges[j]
                e.X = est_pt[i]
                rec[j] = linearize(e, est_pose[v], cam, kernel, vfree[v] >= 0)
                rho_of[j] = rec[j][1]
            Hll, bl = [], []
            for i in range(len(lpt)):
                H, b = [0.0] * 6, [0.0] * 3
                for j in pt_edges[i]:
                    for q in range(6):
                        H[q] = H[q] + rec[j][2][q]
                    for q in range(3):
                        b[q] = b[q] + rec[j][3][q]
                Hll.append(H)
                bl.append(b)
            Hpp, bp = {}, {}
            for f in act:
                s = wave_sum([(k, rec[j][4] + rec[j][5]) for k, j in enumerate(kf_edges[f])], 27)
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
                Dinv, db = [], []
                for i in range(len(lpt)):
                    D = inv3(Hll[i], lam)
                    Dinv.append(D)
                    db.append([(sym3(D, r, 0) * bl[i][0] + sym3(D, r, 1) * bl[i][1]) + sym3(D, r, 2) * bl[i][2] for r in range(3)])
                m = 6 * len(act)
                A = [[0.0] * m for _ in range(m)]
                bs = [0.0] * m
                for i1 in act:
                    ent = {i1: []}                                       # partner pose -> (k, vector); a pair without a shared point sums to 0.0
                    for k, j1 in enumerate(kf_edges[i1]):
                        pi = edges[j1][2]
                        B1, D = rec[j1][6], Dinv[pi]
                        g = []
                        for a in range(6):
                            p0, p1, p2 = B1[a * 3], B1[a * 3 + 1], B1[a * 3 + 2]
                            g.append([(p0 * sym3(D, 0, c) + p1 * sym3(D, 1, c)) + p2 * sym3(D, 2, c) for c in range(3)])
                        seen = set()
                        for j2 in [j1] + pt_edges[pi]:                   # the diagonal takes the edge itself, a partner pose its
                            i2 = i1 if not seen else vfree[edges[j2][1]]  # first edge of the point
                            if seen and (i2 <= i1 or i2 in seen):
                                continue
                            seen.add(i2)
                            B2 = rec[j2][6]
                            vec = []
                            for a in range(6):
                                for b in range(6):
                                    vec.append((g[a][0] * B2[b * 3] + g[a][1] * B2[b * 3 + 1]) + g[a][2] * B2[b * 3 + 2])
                            if i2 == i1:
                                for a in range(6):
                                    p0, p1, p2 = B1[a * 3], B1[a * 3 + 1], B1[a * 3 + 2]
                                    vec.append((p0 * db[pi][0] + p1 * db[pi][1]) + p2 * db[pi][2])
                            else:
                                vec += [0.0] * 6
                            ent.setdefault(i2, []).append((k, vec))
                    c1 = 6 * col[i1]
                    for i2, lst in ent.items():
                        s = wave_sum(lst, 42)
                        if i1 == i2:
                            for a in range(6):
                                for b in range(a + 1):
                                    h = Hpp[i1][upper21(b, a)]
                                    if a == b:
                                        h = h + lam
                                    A[c1 + a][c1 + b] = h - s[b * 6 + a]
                                bs[c1 + a] = bp[i1][a] - s[36 + a]
                        else:
                            c2 = 6 * col[i2]
                            for a in range(6):
                                for b in range(6):
                                    A[c2 + b][c1 + a] = 0.0 - s[a * 6 + b]
                ok2, x = solve(A, bs)
                if ok2:
                    for f in act:
                        xp[6 * f:6 * f + 6] = x[6 * col[f]:6 * col[f] + 6]
                    for i in range(len(lpt)):                            # Dinv (b_l - B^T x_p)
                        c = bl[i][:]
                        for j in pt_edges[i]:
                            f = vfree[edges[j][1]]
                            if f < 0:
                                continue
                            B = rec[j][6]
                            nx = [-xp[6 * f + a] for a in range(6)]
                            for b in range(3):
                                c[b] = c[b] + (((((B[b] * nx[0] + B[3 + b] * nx[1]) + B[6 + b] * nx[2]) + B[9 + b] * nx[3]) +
                                                B[12 + b] * nx[4]) + B[15 + b] * nx[5])
                        D = Dinv[i]
                        xl[i] = [(sym3(D, r, 0) * c[0] + sym3(D, r, 1) * c[1]) + sym3(D, r, 2) * c[2] for r in range(3)]
                tried_pose = [se3_mul(se3_exp(xp[6 * vfree[v]:6 * vfree[v] + 6]), est_pose[v])
                              if vfree[v] >= 0 and pose_active[vfree[v]] else est_pose[v] for v in range(len(vtx_rows))]
                tried_pt = [[est_pt[i][a] + xl[i][a] for a in range(3)] for i in range(len(lpt))]
                errors_at(tried_pose, tried_pt)
                temp = team_reduce(items_e, lambda t, acc: acc + rho_of[t], add)
                if not ok2:
                    temp = DBL_MAX
                rho = current - temp
                scale = team_reduce(items_v, lambda t, acc: acc + xvec(t) * (lam * xvec(t) + bvec(t)), add)
                scale = scale + 1e-3
                rho = fdiv(rho, scale)
                accepted = rho > 0 and math.isfinite(temp)
                decisions.append((accepted, rho, current, temp))
                if accepted:
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
                trials += 1
                if not (rho < 0 and qmax < 10 and not st.sample()):
                    break
            its += 1
            if qmax == 10 or rho == 0:
                ok = False
                continue
            if (ini - current) * 1e3 < ini:
                n_bad += 1
            else:
                n_bad = 0
            if n_bad >= 3:
                ok = False

    # ---- :193-235: the write-back
    for v, r in enumerate(vtx_rows):
        R, t = to_R(est_pose[v][0]), est_pose[v][1]
        M = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
        dst = Tcw if mode == IN_PLACE else TcwGBA
        for k in range(12):
            dst[r][k] = np.float32(M[k])
        if mode == STAGED:
            kf_mark[r] = 1
    for i, p in enumerate(lpt):
        dst = world if mode == IN_PLACE else posGBA
        for k in range(3):
            dst[p][k] = np.float32(est_pt[i][k])
        if mode == STAGED:
            pt_mark[p] = 1
        else:
            point_list[i] = p
    report[9], report[10] = its, trials
    report[12] = len(lpt) if mode == IN_PLACE else 0
    if trace is not None:
        trace["decisions"] = decisions
        trace["vtx_rows"], trace["points"] = vtx_rows, lpt
        trace["pose"] = [q + t for q, t in est_pose]
        trace["pt"] = [x[:] for x in est_pt]
    return finish(status)


# ---- the apply step ------------------------------------------------------------------------------------------------------------
F = np.float32


def inverse(T):
    """KeyFrame::SetPose: [Rwc | Ow] of the 12 floats of Tcw."""
    T = [F(v) for v in T]
    out = []
    for r in range(3):
        a0, a1, a2 = T[r], T[4 + r], T[8 + r]
        out += [a0, a1, a2, F(F(F(-a0) * T[3]) + F(F(-a1) * T[7])) + F(F(-a2) * T[11])]
    return [F(v) for v in out]


def mul44(a, b):
    """[R | t; 0 0 0 1] times the same, the first three rows."""
    a, b = [F(v) for v in a], [F(v) for v in b]
    c = []
    for i in range(3):
        for j in range(4):
            b3 = F(1.0) if j == 3 else F(0.0)
            c.append(F(F(F(F(a[i * 4] * b[j]) + F(a[i * 4 + 1] * b[4 + j])) + F(a[i * 4 + 2] * b[8 + j])) + F(a[i * 4 + 3] * b3)))
    return c


def apply_global_ba(arrays, refuse=False):
    """arrays: dict with origins, parent [rows], kf_bad [rows] or None, kf_mark, TcwGBA, Tcw, pt_mark, posGBA, flags, ref_kf,
    world, and optionally the caller's TcwBefGBA.  Returns dict(kf_mark, TcwGBA, Tcw, world, TcwBefGBA, report [8]): copies."""
    parent, kf_bad = arrays["parent"], arrays.get("kf_bad")
    rows, pcap = len(parent), len(arrays["flags"])
    kf_mark = np.array(arrays["kf_mark"], np.uint8)
    TcwGBA, Tcw = np.array(arrays["TcwGBA"], F).reshape(rows, 12), np.array(arrays["Tcw"], F).reshape(rows, 12)
    world = np.array(arrays["world"], F).reshape(pcap, 3)
    bef = np.array(arrays["TcwBefGBA"], F).reshape(rows, 12) if arrays.get("TcwBefGBA") is not None else np.zeros((rows, 12), F)
    good = lambda r: 0 <= r < rows and not (kf_bad is not None and kf_bad[r])  # noqa: E731
    visited = [False] * rows
    queue = []
    for o in arrays["origins"]:
        o = int(o)
        if good(o) and kf_mark[o]:
            if len(queue) < rows:
                queue.append(o)
        elif refuse:
            raise ValueError("origin %d must be a marked row of the map" % o)
    head = propagated = 0
    while head < len(queue):                                             # at most `rows` pops: the queue holds no more
        k = queue[head]
        head += 1
        Twc = inverse(Tcw[k])                                            # before this row's SetPose
        for c in range(rows):                                            # GetChilds(): ascending row
            if int(parent[c]) != k or not good(c):
                continue
            if not kf_mark[c]:
                TcwGBA[c] = mul44(mul44(Tcw[c], Twc), TcwGBA[k])
                kf_mark[c] = 1
                propagated += 1
            if len(queue) < rows:
                queue.append(c)
        bef[k] = Tcw[k]
        Tcw[k] = TcwGBA[k]
        visited[k] = True
    cnt = [head, propagated, 0, 0, 0, 0, 0, 0]
    for p in range(pcap):
        if not (int(arrays["flags"][p]) & POINT_PRESENT):
            continue
        cnt[5] += 1
        if arrays["pt_mark"][p]:
            world[p] = np.array(arrays["posGBA"], F).reshape(pcap, 3)[p]
            cnt[2] += 1
            continue
        r = int(arrays["ref_kf"][p])
        if r < 0 or r >= rows or not kf_mark[r] or not visited[r]:
            cnt[4] += 1
            continue
        B, X = bef[r], [F(v) for v in world[p]]
        Xc = [F(F(F(F(B[i * 4] * X[0]) + F(B[i * 4 + 1] * X[1])) + F(B[i * 4 + 2] * X[2])) + B[i * 4 + 3]) for i in range(3)]
        W = inverse(Tcw[r])
        world[p] = [F(F(F(F(W[i * 4] * Xc[0]) + F(W[i * 4 + 1] * Xc[1])) + F(W[i * 4 + 2] * Xc[2])) + W[i * 4 + 3]) for i in range(3)]
        cnt[3] += 1
    return dict(kf_mark=kf_mark, TcwGBA=TcwGBA, Tcw=Tcw, world=world, TcwBefGBA=bef, report=cnt)
