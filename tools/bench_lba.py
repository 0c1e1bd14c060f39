#!/usr/bin/env python3
"""Cost of Optimizer::LocalBundleAdjustment on the device and of the host round trip it replaces, same process, same inputs.

The workload has the sizes of tools/bench_localmap.py: key frames of 1241 x 376 with 1000 key points (cap 1000), 60 bank
rows, a map of 9000 points, each observed by 2 .. 8 rows of a window of 12 rows around its own; here the rows stand on a
line, the points in front of it, and every key point is the projection of its point plus noise, with 3 % gross outliers.  The
current key frame is the last row, its covisible list the 20 rows before it; the rows further back that see local points
are the fixed cameras.

  (a) LocalBundleAdjustmentDevice, one call: the fixed sequence of 950 launches.  Warm, HIP-event time on the matcher's
      stream, median over --reps; the timed call includes the device copies that restore Tcw and world.
  (a1) the same call with the stop byte set: the setup runs and every later launch leaves at once; what the fixed sequence
      costs when it does nothing.
  (a2) LocalBundleAdjustment, the host form (one staged copy, the call, one read-back).  Wall clock.
  (b) what a caller had to do without the entry: D2H of the tables, the same rules in vectorised numpy (Schur complement over
      points, numpy.linalg.solve for the poses), H2D of Tcw and world.  Wall clock.  This host route is numpy, NOT g2o: g2o
      needs Eigen, which is not available to this project's build, so b / a is no claim against the reference's C++.  (b) is
      checked for sanity: it must erase the same observations as the device.
  (c) optionally the log of a headline A/B (lines "[label] value ...", parent and new interleaved in one call on one box).

  python tools/bench_lba.py [--reps 10] [--warmup 2] [--ab-log FILE] [--out profiles/lba_stage.json]
  python tools/bench_lba.py --host-only     # no GPU: builds the scene and runs route (b)'s arithmetic once

The launches that did work are counted from the report: 1 (setup) + 3 per outer iteration + 6 per trial + 2 (level-1 rule)
+ 2 (epilogue); the rest of the 950 read the state record and leave.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
i32, u8, f32, f64 = np.int32, np.uint8, np.float32, np.float64
ROWS, NPTS, CAP, WINDOW, LOCAL, MAX_EDGES = 60, 9000, 1000, 12, 20, 65536
ENQUEUED = 1 + 15 * (3 + 10 * 6) + 2 + 2


def scene():
    import test_lba_cpu as K
    sc = K.Scene(ROWS, CAP, NPTS, 7)
    K._line_of_cameras(sc, range(ROWS), step=0.4)
    rng = sc.rng
    centre = rng.integers(0, ROWS, NPTS)
    for p in range(NPTS):
        sc.point([0.4 * centre[p] + rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(5, 25)])
    for p in range(NPTS):
        rs = np.sort(np.clip(centre[p] - WINDOW // 2 + rng.choice(WINDOW, rng.integers(2, 9), replace=False), 0, ROWS - 1))
        for r in np.unique(rs):
            if sc.n[r] >= CAP:
                continue
            gross = rng.random() < 0.03
            ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(15, 40)
            sc.observe(p, int(r), stereo=rng.random() < 0.5, offset=(mag * math.cos(ang), mag * math.sin(ang)) if gross else (0.0, 0.0))
    cur = ROWS - 1
    t = sc.tables(cur, list(range(cur - 1, cur - 1 - LOCAL, -1)))
    return K, K._case(t, cur, 0, NPTS, MAX_EDGES)


def _skew(V):
    Z = np.zeros(len(V))
    return np.stack([np.stack([Z, -V[:, 2], V[:, 1]], 1), np.stack([V[:, 2], Z, -V[:, 0]], 1), np.stack([-V[:, 1], V[:, 0], Z], 1)], 1)


def _exp(u):
    w, up = u[:3], u[3:]
    th = np.linalg.norm(w)
    Om = _skew(w[None])[0]
    if th < 1e-5:
        R = np.eye(3) + Om + Om @ Om
        return R, R @ up
    R = np.eye(3) + math.sin(th) / th * Om + (1 - math.cos(th)) / th ** 2 * Om @ Om
    V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * Om + (th - math.sin(th)) / th ** 3 * Om @ Om
    return R, V @ up


def host_rules(K, b, t):
    """The rules of tests/seqref/lba.py in vectorised numpy.  Returns (Tcw, world, erase rows as a set, edges)."""
    fx, fy, cx, cy, bf = (float(f32(v)) for v in K.CAM)
    rows, cap = t["slot_point"].shape
    cur, id0 = b["cur"], b["id0_row"]
    bad = t["kf_bad"].astype(bool)
    lkf = [cur] + [int(r) for r in t["ord_kf"][cur][:int(t["n_ord"][cur])] if not bad[r]]
    sp = np.concatenate([t["slot_point"][r][:int(t["n"][r])] for r in lkf])
    sp = sp[sp >= 0]
    sp = sp[(t["flags"][sp] & 1) != 0]
    _, first = np.unique(sp, return_index=True)
    lpt = sp[np.sort(first)]
    pos = np.full(len(t["flags"]), -1)
    pos[lpt] = np.arange(len(lpt))
    o_pt = np.repeat(np.arange(len(t["obs_start"]) - 1), np.diff(t["obs_start"]))
    total = int(t["obs_start"][-1])
    okf, oidx = t["obs_kf"][:total], t["obs_idx"][:total]
    sel = (pos[o_pt] >= 0) & ~bad[okf]
    e_kf, e_idx, e_pt = okf[sel], oidx[sel], pos[o_pt[sel]]
    local = np.zeros(rows, bool)
    local[lkf] = True
    free_rows = [r for r in lkf if r != id0]
    col = np.full(rows, -1)
    col[free_rows] = np.arange(len(free_rows))
    e_col = col[e_kf]
    ur = t["u_right"][e_kf, e_idx].astype(f64)
    st = ~(ur < 0)
    obs = np.c_[t["kps"]["x"][e_kf, e_idx], t["kps"]["y"][e_kf, e_idx], np.where(st, ur, 0.0)].astype(f64)
    inv = K.INV_SIGMA2[t["kps"]["octave"][e_kf, e_idx]].astype(f64)
    delta = np.where(st, float(f32(math.sqrt(7.815))), float(f32(math.sqrt(5.991))))
    thr = np.where(st, 7.815, 5.991)
    T = t["Tcw"].astype(f64).reshape(rows, 3, 4)
    Rs, ts = T[:, :, :3].copy(), T[:, :, 3].copy()
    X = t["world"][lpt].astype(f64)
    ne, npt, nf = len(e_kf), len(lpt), len(free_rows)
    act = np.ones(ne, bool)

    def errors(Rs, ts, X):
        P = np.einsum("eij,ej->ei", Rs[e_kf], X[e_pt]) + ts[e_kf]
        invz = np.where(st, (1.0 / P[:, 2]).astype(f32).astype(f64), 1.0 / P[:, 2])
        u, v = P[:, 0] * invz * fx + cx, P[:, 1] * invz * fy + cy
        err = obs - np.c_[u, v, np.where(st, u - bf * invz, 0.0)]
        return err, P

    def robust(err, kernel):
        c2 = inv * (err * err).sum(1)
        big = kernel & (c2 > delta * delta)
        sq = np.sqrt(np.where(big, c2, 1.0))
        return c2, np.where(big, 2 * sq * delta - delta * delta, c2), np.where(big, delta / sq, 1.0)

    def optimize(iters, kernel):
        nonlocal Rs, ts, X
        chi2 = np.zeros(ne)
        if not act.any():
            return chi2
        lam = ni = 0.0
        nbad = 0
        for it in range(iters):
            err, P = errors(Rs, ts, X)
            c2, rho0, rho1 = robust(err, kernel)
            chi2 = c2
            cur_ = ini = rho0[act].sum()
            x, y, z = P[:, 0], P[:, 1], P[:, 2]
            z2 = z * z
            Z = np.zeros(ne)
            Jc = np.stack([np.stack([x * y / z2 * fx, -(1 + x * x / z2) * fx, y / z * fx, -fx / z, Z, x / z2 * fx], 1),
                           np.stack([(1 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy, Z, -fy / z, y / z2 * fy], 1),
                           np.stack([x * y / z2 * fx - bf * y / z2, -(1 + x * x / z2) * fx + bf * x / z2, y / z * fx, -fx / z, Z,
                                     x / z2 * fx - bf / z2], 1)], 1)
            dp = np.zeros((ne, 3, 3))
            dp[:, 0, 0], dp[:, 0, 2] = fx / z, -fx * x / z2
            dp[:, 1, 1], dp[:, 1, 2] = fy / z, -fy * y / z2
            dp[:, 2, 0], dp[:, 2, 2] = fx / z, -fx * x / z2 + bf / z2
            Jp = -np.einsum("eij,ejk->eik", dp, Rs[e_kf])
            Jc[~st, 2], Jp[~st, 2] = 0.0, 0.0
            w = rho1 * inv * act
            Hll = np.zeros((npt, 3, 3))
            np.add.at(Hll, e_pt, np.einsum("erk,e,erl->ekl", Jp, w, Jp))
            bl = np.zeros((npt, 3))
            np.add.at(bl, e_pt, -np.einsum("erk,e,er->ek", Jp, w, err))
            fe = e_col >= 0
            Hpp = np.zeros((nf, 6, 6))
            np.add.at(Hpp, e_col[fe], np.einsum("erk,e,erl->ekl", Jc[fe], w[fe], Jc[fe]))
            bp = np.zeros((nf, 6))
            np.add.at(bp, e_col[fe], -np.einsum("erk,e,er->ek", Jc[fe], w[fe], err[fe]))
            B = np.einsum("erk,e,erl->ekl", Jc, w, Jp)                               # [edge][6][3]
            pa = np.zeros(npt, bool)
            pa[e_pt[act]] = True
            ca = np.zeros(nf, bool)
            ca[e_col[act & fe]] = True
            if it == 0:
                mx = max(np.abs(np.einsum("pii->pi", Hll)[pa]).max(initial=0.0), np.abs(np.einsum("pii->pi", Hpp)[ca]).max(initial=0.0))
                lam, ni, nbad = 1e-5 * mx, 2.0, 0
            q = 0
            while True:
                D = Hll + lam * np.eye(3)
                D[~pa] = np.eye(3)
                Dinv = np.linalg.inv(D)
                S = np.zeros((nf, nf, 6, 6))
                S[np.arange(nf), np.arange(nf)] = Hpp + lam * np.eye(6)
                BD = np.einsum("eij,ejk->eik", B, Dinv[e_pt])
                bs = bp.copy()
                np.add.at(bs, e_col[fe & act], -np.einsum("eij,ej->ei", BD[fe & act], bl[e_pt[fe & act]]))
                idx = np.flatnonzero(fe & act)
                order = idx[np.argsort(e_pt[idx], kind="stable")]
                starts = np.flatnonzero(np.r_[True, np.diff(e_pt[order]) != 0, True])
                for s0, s1 in zip(starts[:-1], starts[1:]):                         # the edges of one point: all pairs of its poses
                    es = order[s0:s1]
                    c = e_col[es]
                    S[c[:, None], c[None, :]] -= np.einsum("aij,bkj->abik", BD[es], B[es])
                keep = np.flatnonzero(ca)
                Sm = S[np.ix_(keep, keep)].transpose(0, 2, 1, 3).reshape(6 * len(keep), 6 * len(keep))
                xp = np.zeros((nf, 6))
                ok2 = True
                try:
                    np.linalg.cholesky(Sm)
                    xp[keep] = np.linalg.solve(Sm, bs[keep].reshape(-1)).reshape(-1, 6)
                except np.linalg.LinAlgError:
                    ok2 = False
                cl = bl.copy()
                np.add.at(cl, e_pt[fe & act], -np.einsum("eij,ei->ej", B[fe & act], xp[e_col[fe & act]]))
                xl = np.einsum("pij,pj->pi", Dinv, cl) * pa[:, None]
                Rn, tn = Rs.copy(), ts.copy()
                for k in keep:
                    r = free_rows[k]
                    dR, dt = _exp(xp[k])
                    Rn[r], tn[r] = dR @ Rs[r], dR @ ts[r] + dt
                Xn = X + xl
                err2, _ = errors(Rn, tn, Xn)
                c2, rho0, _ = robust(err2, kernel)
                chi2 = np.where(act, c2, chi2)
                tmp = rho0[act].sum() if ok2 else 1.7976931348623157e308
                scale = (xp[ca] * (lam * xp[ca] + bp[ca])).sum() + (xl[pa] * (lam * xl[pa] + bl[pa])).sum() + 1e-3
                rho = (cur_ - tmp) / scale
                if rho > 0 and math.isfinite(tmp):
                    lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                    ni, cur_ = 2.0, tmp
                    Rs, ts, X = Rn, tn, Xn
                else:
                    lam *= ni
                    ni *= 2
                q += 1
                if not (rho < 0 and q < 10):
                    break
            if q == 10 or rho == 0:
                break
            nbad = nbad + 1 if (ini - cur_) * 1e3 < ini else 0
            if nbad >= 3:
                break
        return chi2

    def check(chi2):
        P = np.einsum("eij,ej->ei", Rs[e_kf], X[e_pt]) + ts[e_kf]
        return (chi2 > thr) | ~(P[:, 2] > 0)

    chi2 = optimize(5, True)
    act &= ~check(chi2)
    chi2 = np.where(act, optimize(10, False), chi2)
    out = check(chi2)
    Tcw, world = t["Tcw"].copy(), t["world"].copy()
    for r in lkf:
        Tcw[r] = np.c_[Rs[r], ts[r]].reshape(12).astype(f32)
    world[lpt] = X.astype(f32)
    return Tcw, world, set(zip(e_kf[out].tolist(), e_idx[out].tolist(), lpt[e_pt[out]].tolist())), ne


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--ab-log")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_stage.json"))
    args = ap.parse_args()
    K, b = scene()
    t = b["tables"]
    if args.host_only:
        t0 = time.perf_counter()
        _, _, erase, ne = host_rules(K, b, t)
        print("host rules: %.1f ms, %d edges, %d erase rows" % ((time.perf_counter() - t0) * 1e3, ne, len(erase)))
        return
    import torch
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    cam = make_camera(*K.CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=K.CAM[4])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731
    keys = ("slot_point", "n", "kf_bad", "obs_start", "obs_kf", "obs_idx", "flags", "kps", "u_right", "ord_kf", "n_ord", "Tcw", "world")
    d_t = {k: up(t[k]) for k in keys}
    d_T0, d_w0 = up(t["Tcw"]), up(t["world"])
    o = K.prefilled(b)
    d_o = {k: up(o[k]) for k in o}

    def device_call():
        d_t["Tcw"].copy_(d_T0, non_blocking=True)
        d_t["world"].copy_(d_w0, non_blocking=True)
        m.LocalBundleAdjustmentDevice(b["cur"], b["id0_row"], cam, b["rows"], b["cap"], b["np"], b["pcap"], d_t, K.INV_SIGMA2,
                                      b["max_points"], b["max_edges"], d_o)

    d_stop = up(np.array([1], u8))

    def stopped_call():
        m.LocalBundleAdjustmentDevice(b["cur"], b["id0_row"], cam, b["rows"], b["cap"], b["np"], b["pcap"], d_t, K.INV_SIGMA2,
                                      b["max_points"], b["max_edges"], d_o, d_stop=d_stop)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def timed_wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    def host_form():
        return m.LocalBundleAdjustment(t, b["cur"], b["id0_row"], cam, K.INV_SIGMA2, b["max_points"], b["max_edges"])

    def round_trip():
        down = {k: d_t[k].cpu().numpy().view(np.asarray(t[k]).dtype).reshape(np.asarray(t[k]).shape) for k in keys if k not in ("Tcw", "world")}
        down["Tcw"], down["world"] = d_T0.cpu().numpy().view(f32).reshape(-1, 12), d_w0.cpu().numpy().view(f32).reshape(-1, 3)
        res = host_rules(K, b, down)
        up(res[0]); up(res[1])
        torch.cuda.synchronize()
        return res

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        device_call()
    m.sync()
    rep = d_o["report"].cpu().numpy().view(i32).tolist()
    erase = d_o["erase"].cpu().numpy().view(i32).reshape(-1, 3)[:rep[7]]
    res = round_trip()
    same_erase = set(map(tuple, erase.tolist())) == res[2]
    dist = float(np.abs(d_t["world"].cpu().numpy().view(f32).reshape(-1, 3) - res[1]).max())
    for _ in range(args.warmup):
        with torch.cuda.stream(stream):
            device_call()
        host_form()
    m.sync()
    a, a2, bb, idle = [], [], [], []
    for _ in range(args.reps):
        a.append(timed_events(device_call))
        a2.append(timed_wall(host_form))
        idle.append(timed_events(stopped_call))
    for _ in range(max(1, args.reps // 5)):
        bb.append(timed_wall(round_trip))
    med = lambda v: float(np.median(v))  # noqa: E731
    worked = 1 + 3 * (rep[8] + rep[10]) + 6 * (rep[9] + rep[11]) + 2 + 2
    doc = {"what": "Optimizer::LocalBundleAdjustment, one call: %d bank rows at cap %d (1241 x 376 @1000), a map of %d points, the last row "
                   "current, %d covisible rows; the timed call includes the device copies that restore Tcw and world" % (ROWS, CAP, NPTS, LOCAL),
           "status": "measured", "reps": args.reps, "report": dict(zip(pkg.capi.LBA_REPORT, rep)),
           "launches": {"enqueued": ENQUEUED, "did_work": worked,
                        "how": "from the report: setup + 3 per outer iteration + 6 per trial + 2 (level-1 rule) + 2 (epilogue)"},
           "a_device": {"us_median": med(a), "us_min": float(min(a)), "us_max": float(max(a))},
           "a_stopped": {"us_median": med(idle), "us_min": float(min(idle)),
                         "what": "the same call with the stop byte set: the setup runs, the 949 launches after it read the state record "
                                 "and leave; the floor the fixed sequence costs"},
           "a2_host_form_us_median": med(a2), "a2_host_form_us_min": float(min(a2)),
           "b_host_round_trip_us_median": med(bb), "b_host_round_trip_us_min": float(min(bb)), "b_reps": len(bb),
           "b_is": "download of the tables + the same rules in vectorised numpy (Schur complement, LAPACK) + upload; numpy, NOT g2o: g2o "
                   "cannot be built without Eigen, so b_over_a is no claim against the reference's C++",
           "b_erases_the_same_observations": bool(same_erase), "b_max_point_distance_from_a_m": dist,
           "clocks": "a: HIP events on the matcher's stream; a2, b: wall clock of synchronous host work",
           "b_over_a": med(bb) / med(a)}
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["c_headline"] = {"how": "bench.py --gpus 1, one call on one box, interleaved parent / new for as many rounds as the log holds; the "
                                    "parent is the parent commit's whole tree with its own library",
                             "unit": "frames/s, higher is better", "parent_runs": runs["parent"], "new_runs": runs["new"],
                             "parent_spread": [lo, hi],
                             "new_within_parent_spread": [bool(lo <= v <= hi) for v in runs["new"]] if lo is not None else None,
                             "new_below_parent_min": [bool(v < lo) for v in runs["new"]] if lo is not None else None}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    m.close()


if __name__ == "__main__":
    main()
