#!/usr/bin/env python3
"""Cost of Optimizer::OptimizeSim3 on the device and of the host round trip it replaces, same process, same inputs.

  (a) OptimizeSim3Device for 5 loop candidates of 100 pairs each (70 under one Sim3, 30 random partners) at cap 512, the
      start turned by 0.01 rad, moved by 2 cm and scaled by 1 %.  Warm, HIP-event time on the matcher's stream, median over
      --reps; the timed call includes the device copy that restores the in/out matches.
  (a2) OptimizeSim3, the host form of the same call (one staged copy, the launch, one read-back).  Wall clock.
  (b) what a caller had to do without the entry: D2H of the matches and the Sim3s, the same rules in vectorised numpy
      (rotation matrices, analytic Jacobians, numpy.linalg.solve), H2D of the matches and the results.  Wall clock.  This host
      route is numpy, NOT g2o: g2o needs Eigen, which is not available to this project's build, so b / a is no claim against
      the reference's C++.  (b) is checked for sanity: it must keep the same matches as the device.
  (c) optionally the log of a headline A/B (lines "[label] value ...", parent and new interleaved in one call on one box).

  python tools/bench_sim3opt.py [--reps 30] [--warmup 3] [--lib PATH --team 64] [--ab-log FILE] [--out profiles/sim3opt_stage.json]
  python tools/bench_sim3opt.py --host-only     # no GPU: builds the scene and runs route (b)'s arithmetic once

--lib times another build of the library (make EXTRA=-DORBHIP_SIM3OPT_TEAM=64: the one-wavefront team) and merges its
device times into the JSON under "team_<n>"; that build sums in another order, so only its kept matches are compared.
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
CANDS, GOOD, RANDOM, N1, CAP = 5, 70, 30, 300, 512


def scene():
    import test_sim3_cpu as S
    import test_sim3opt_cpu as K
    sc = K.scene(((GOOD, RANDOM),) * CANDS, N1, CAP, 90)
    return S, K, sc, K.sim3_record(S.SIM3_A, 0.01, 0.02, 1.01, CANDS)


def _skew(V):
    Z = np.zeros(len(V))
    return np.stack([np.stack([Z, -V[:, 2], V[:, 1]], 1), np.stack([V[:, 2], Z, -V[:, 0]], 1), np.stack([-V[:, 1], V[:, 0], Z], 1)], 1)


def host_rules(K, Q, sc, c, matched, rec, fix_scale=False):
    """The rules of tests/seqref/sim3opt.py for one candidate in vectorised numpy; returns (matched [cap], R, t, s, nIn)."""
    T = sc["T"]
    cur, kf = sc["cur"], int(sc["kf_index"][c])
    fx, fy, cx, cy = (float(f32(v)) for v in K.CAM)
    n1 = int(T["n"][cur])
    m = matched[:n1]
    p1 = T["slot_point"][cur][:n1]
    ok = (m >= 0) & (p1 >= 0)
    idx = np.flatnonzero(ok)
    p2 = m[idx]
    keep = ((T["flags"][p1[idx]] & 1) != 0) & ((T["flags"][p2] & 1) != 0)
    first = T["obs_start"][p2]
    keep &= (T["obs_start"][p2 + 1] > first) & (T["obs_kf"][np.minimum(first, len(T["obs_kf"]) - 1)] == kf)   # one observation per point here
    idx, p2 = idx[keep], p2[keep]
    i2 = T["obs_idx"][T["obs_start"][p2]]
    T1, T2 = T["Tcw"][cur].astype(f64).reshape(3, 4), T["Tcw"][kf].astype(f64).reshape(3, 4)
    P1 = (T["world"][p1[idx]].astype(f64) @ T1[:, :3].T + T1[:, 3]).astype(f32).astype(f64)
    P2 = (T["world"][p2].astype(f64) @ T2[:, :3].T + T2[:, 3]).astype(f32).astype(f64)
    k1, k2 = T["kps"][cur][idx], T["kps"][kf][i2]
    o1, o2 = np.c_[k1["x"], k1["y"]].astype(f64), np.c_[k2["x"], k2["y"]].astype(f64)
    w1, w2 = K.INV_SIGMA2[k1["octave"]].astype(f64), K.INV_SIGMA2[k2["octave"]].astype(f64)
    out = matched.copy()
    if len(idx) == 0:
        return out, None, None, None, 0
    r = rec.astype(f64)
    R, t, s = r[:9].reshape(3, 3), r[9:12], r[12]
    delta, th2 = float(np.sqrt(f32(K.TH2))), float(f32(K.TH2))
    act = np.ones(len(idx), bool)

    def proj(Y):
        return np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy]

    def errs(R, t, s):
        Y1, Y2 = s * P2 @ R.T + t, (P1 - t) @ R / s
        return o1 - proj(Y1), o2 - proj(Y2), Y1, Y2

    def rob(e, w):
        c2 = w * (e * e).sum(1)
        big = c2 > delta * delta
        sq = np.sqrt(np.where(big, c2, 1.0))
        return c2, np.where(big, 2 * sq * delta - delta * delta, c2), np.where(big, delta / sq, 1.0)

    def cost(R, t, s):
        e12, e21, _, _ = errs(R, t, s)
        return rob(e12, w1)[1][act].sum() + rob(e21, w2)[1][act].sum()

    def system(R, t, s):
        e12, e21, Y1, Y2 = errs(R, t, s)
        H, g = np.zeros((7, 7)), np.zeros(7)
        I3 = np.broadcast_to(np.eye(3), (len(idx), 3, 3))
        D12 = np.concatenate([-_skew(Y1), I3, Y1[:, :, None]], 2)
        D21 = np.einsum("ij,ejk->eik", R.T / s, np.concatenate([_skew(P1), -I3, -P1[:, :, None]], 2))
        for e, Y, D, w in ((e12, Y1, D12, w1), (e21, Y2, D21, w2)):
            dp = np.zeros((len(idx), 2, 3))
            dp[:, 0, 0], dp[:, 0, 2] = fx / Y[:, 2], -fx * Y[:, 0] / Y[:, 2] ** 2
            dp[:, 1, 1], dp[:, 1, 2] = fy / Y[:, 2], -fy * Y[:, 1] / Y[:, 2] ** 2
            J = -np.einsum("eij,ejk->eik", dp, D)
            if fix_scale:
                J[:, :, 6] = 0.0
            ww = (rob(e, w)[2] * w * act)
            H += np.einsum("erk,e,erl->kl", J, ww, J)
            g += -np.einsum("erk,e,er->k", J, ww, e)
        return H, g

    def exp(u):
        G = np.zeros((4, 4))
        G[:3, :3] = _skew(u[None, 0:3])[0] + u[6] * np.eye(3)
        G[:3, 3] = u[3:6]
        G = G / 256.0
        M, term = np.eye(4), np.eye(4)
        for i in range(1, 12):
            term = term @ G / i
            M = M + term
        for _ in range(8):
            M = M @ M
        sc_ = np.cbrt(np.linalg.det(M[:3, :3]))
        return M[:3, :3] / sc_, M[:3, 3], sc_

    def optimize(R, t, s, max_it):
        tried = (R, t, s)
        lam = ni = 0.0
        nbad = 0
        for it in range(max_it):
            H, g = system(R, t, s)
            cur_ = ini = cost(R, t, s)
            if it == 0:
                lam, ni, nbad = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
            q = 0
            while True:
                x = np.linalg.solve(H + lam * np.eye(7), g)
                if fix_scale:
                    x[6] = 0.0
                dR, dt, ds = exp(x)
                tried = (dR @ R, ds * dR @ t + dt, ds * s)
                tmp = cost(*tried)
                rho = (cur_ - tmp) / (x @ (lam * x + g) + 1e-3)
                if rho > 0 and math.isfinite(tmp):
                    lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                    ni, cur_ = 2.0, tmp
                    R, t, s = tried
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
        return (R, t, s), tried

    def check(tried):
        e12, e21, _, _ = errs(*tried)
        return act & ((rob(e12, w1)[0] > th2) | (rob(e21, w2)[0] > th2))

    (R, t, s), tried = optimize(R, t, s, 5)
    bad = check(tried)
    out[idx[bad]] = -1
    act &= ~bad
    if len(idx) - int(bad.sum()) < 10:
        return out, None, None, None, 0
    (R, t, s), tried = optimize(R, t, s, 10 if bad.any() else 5)
    bad2 = check(tried)
    out[idx[bad2]] = -1
    return out, R, t, s, int((act & ~bad2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--team", type=int, default=256)
    ap.add_argument("--ab-log")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_stage.json"))
    args = ap.parse_args()
    S, K, sc, sim3 = scene()
    from seqref import sim3 as S3
    from seqref import sim3opt as Q
    if args.host_only:
        for c in range(CANDS):
            t0 = time.perf_counter()
            out, R, t, s, n_in = host_rules(K, Q, sc, c, sc["m_points"][c], sim3[c])
            print("host rules, candidate %d: %.1f ms, nIn %d, s %.6f" % (c, (time.perf_counter() - t0) * 1e3, n_in, s))
        return
    import torch
    from orb_slam2_comment_amd import capi
    if args.lib:
        capi.use_library(os.path.abspath(args.lib))
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    cam = make_camera(K.CAM[0], K.CAM[1], K.CAM[2], K.CAM[3], (0.0, 0.0, 640.0, 480.0), [1.2 ** l for l in range(8)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731
    T, rows, cap, n_pts, pcap = m._sim3_tables(sc["T"])
    dT = {k: up(v) for k, v in T.items()}
    d_kf, d_m0, d_m, d_sim3 = up(sc["kf_index"]), up(sc["m_points"]), up(sc["m_points"]), up(sim3)
    d_S12, d_Scw, d_rep = up(np.zeros((CANDS, 8), f64)), up(np.zeros((CANDS, 12), f32)), up(np.zeros((CANDS, 8), i32))

    def device_call():
        d_m.copy_(d_m0, non_blocking=True)
        m.OptimizeSim3Device(CANDS, sc["cur"], d_kf, cam, rows, cap, n_pts, pcap, dT, S3.MATCH_POINTS, K.INV_SIGMA2, d_m, d_sim3, d_S12,
                             d_Scw, d_rep, K.TH2, False)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def timed_wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    def host_form():
        m.OptimizeSim3(sc["T"], sc["cur"], sc["kf_index"], cam, sc["m_points"], S3.MATCH_POINTS, K.INV_SIGMA2, sim3, K.TH2, False)

    def round_trip():
        matched = d_m0.cpu().numpy().view(i32).reshape(CANDS, cap)
        rec = d_sim3.cpu().numpy().view(f32).reshape(CANDS, 16)
        res = [host_rules(K, Q, sc, c, matched[c], rec[c]) for c in range(CANDS)]
        up(np.stack([r[0] for r in res]))
        up(np.array([np.r_[r[1].ravel(), r[2], r[3]] for r in res], f64))
        torch.cuda.synchronize()
        return res

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        device_call()
    m.sync()
    rep = d_rep.cpu().numpy().view(i32).reshape(CANDS, 8)
    kept = d_m.cpu().numpy().view(i32).reshape(CANDS, cap) >= 0
    S12 = d_S12.cpu().numpy().view(f64).reshape(CANDS, 8)
    res = round_trip()
    agree = [bool(np.array_equal(kept[c], res[c][0] >= 0)) for c in range(CANDS)]
    assert all(agree) or args.lib, agree                                        # the sanity check of route (b)
    dist_s = max(abs(S12[c][7] - res[c][3]) for c in range(CANDS))
    for _ in range(args.warmup):
        with torch.cuda.stream(stream):
            device_call()
        host_form()
    m.sync()
    a, a2, b = [], [], []
    for _ in range(args.reps):
        a.append(timed_events(device_call))
        if not args.lib:
            a2.append(timed_wall(host_form))
            b.append(timed_wall(round_trip))
    med = lambda v: float(np.median(v))  # noqa: E731
    dev = {"us_median": med(a), "us_min": float(min(a)), "us_max": float(max(a)), "reports": rep.tolist(), "kept_as_route_b": agree}
    if args.lib:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["team_%d" % args.team] = {"how": "the same call against a build with -DORBHIP_SIM3OPT_TEAM=%d, a process of its own in the "
                                             "same call on the same box" % args.team, "a_device": dev}
    else:
        doc = {"what": "Optimizer::OptimizeSim3 for %d candidates of %d pairs (%d under one Sim3, %d random partners) at cap %d; the timed "
                       "call includes the device copy that restores the in/out matches.  One workgroup of %d lanes per candidate, one "
                       "launch." % (CANDS, GOOD + RANDOM, GOOD, RANDOM, CAP, args.team),
               "status": "measured", "reps": args.reps, "team": args.team, "a_device": dev,
               "a2_host_form_us_median": med(a2), "a2_host_form_us_min": float(min(a2)),
               "b_host_round_trip_us_median": med(b), "b_host_round_trip_us_min": float(min(b)),
               "b_is": "download + the same rules in vectorised numpy (LAPACK) + upload; numpy, NOT g2o: g2o cannot be built without "
                       "Eigen, so b_over_a is no claim against the reference's C++",
               "b_scale_distance_from_a": dist_s,
               "clocks": "a: HIP events on the matcher's stream; a2, b: wall clock of synchronous host work",
               "b_over_a": med(b) / med(a)}
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["c_headline"] = {"how": "bench.py --full --no-cpu-baseline --no-secondary, one call on one box, interleaved parent / new for as "
                                    "many rounds as the log holds; the parent is the parent commit's whole tree with its own library, because "
                                    "its binding declares fewer symbols",
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
