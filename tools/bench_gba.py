#!/usr/bin/env python3
"""Stage benchmark of global bundle adjustment (orbhip_global_bundle_adjustment_device, ORBHIP_GBA_STAGED) plus the apply step
(orbhip_apply_global_ba_device) -> profiles/gba_stage.json.

One MI355X.  The scene: a ring of 400 key frames (the ring map of tools/bench_essgraph.py, here with observations), 20 000 map
points, each seen by 8 consecutive key frames (160 000 edges, half of them stereo), iterations 10, robust 0; the spanning tree is
the chain of rows.  Measured warm, median of --reps:
  a   the device call plus the apply step (the call synchronises, so HIP events around both and the wall clock agree but for the
      host's share); the launch and synchronisation counters of the call
  b   the host route, wall clock: D2H of the tables, the same rules in vectorised numpy (Schur complement by scatter-adds, the
      reduced system through numpy.linalg.solve, i.e. LAPACK; numpy, NOT g2o, which cannot be built here), the apply step in
      numpy, H2D of the poses and points
  the split of a over setup, linearisation, Schur complement, factorisation, substitution and the rest comes from a kernel trace
  taken in a run of its own (--kernel-stats <csv of rocprofv3 --kernel-trace --stats>, the traced run is `--once`)
  --ab-log: the bench.py headline of parent and new from one interleaved call (lines "[label] <frames/s> ...")
With --unmeasured the schema is written with "status": "unmeasured" and nothing is run.
"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
ROWS, NPTS, SEEN, CAP, ITERATIONS = 400, 20000, 8, 512, 10
CAM = (718.856, 718.856, 607.19, 185.2, 386.1)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
INV_SIGMA2 = np.array([1.0 / 1.2 ** (2 * l) for l in range(8)], f32)


def scene(seed=5):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = CAM
    th = 2 * np.pi * np.arange(ROWS) / ROWS
    radius = 30.0
    R = np.zeros((ROWS, 3, 3))
    C = np.stack([radius * np.cos(th), np.zeros(ROWS), radius * np.sin(th)], 1)
    R[:, 2] = np.stack([np.cos(th), np.zeros(ROWS), np.sin(th)], 1)            # the camera looks outwards
    R[:, 0] = np.stack([-np.sin(th), np.zeros(ROWS), np.cos(th)], 1)
    R[:, 1] = np.cross(R[:, 2], R[:, 0])
    t = -np.einsum("rij,rj->ri", R, C)
    anchor = (np.arange(NPTS) * ROWS) // NPTS
    Xc = np.stack([rng.uniform(-2, 2, NPTS), rng.uniform(-1.5, 1.5, NPTS), rng.uniform(8, 16, NPTS)], 1)
    X = np.einsum("pji,pj->pi", R[anchor], Xc - t[anchor])
    kps = np.zeros((ROWS, CAP), KP_DTYPE)
    ur = np.full((ROWS, CAP), -1.0, f32)
    n = np.zeros(ROWS, i32)
    obs_kf, obs_idx = np.zeros((NPTS, SEEN), i32), np.zeros((NPTS, SEEN), i32)
    for k in range(SEEN):
        rows = (anchor + k - SEEN // 2) % ROWS
        order = np.argsort(rows, kind="stable")
        slot = np.zeros(NPTS, i32)
        counts = np.bincount(rows, minlength=ROWS)
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        slot[order] = n[rows[order]] + (np.arange(NPTS) - starts[rows[order]])
        n += counts.astype(i32)
        P = np.einsum("pij,pj->pi", R[rows], X) + t[rows]
        octave = rng.integers(0, 8, NPTS)
        sig = 1.2 ** octave
        u = fx * P[:, 0] / P[:, 2] + cx + rng.normal(0, 0.3, NPTS) * sig
        v = fy * P[:, 1] / P[:, 2] + cy + rng.normal(0, 0.3, NPTS) * sig
        stereo = rng.random(NPTS) < 0.5
        kps["x"][rows, slot], kps["y"][rows, slot], kps["octave"][rows, slot] = u, v, octave
        ur[rows, slot] = np.where(stereo, u - bf / P[:, 2], -1.0)
        obs_kf[:, k], obs_idx[:, k] = rows, slot
    assert n.max() <= CAP
    Tcw = np.zeros((ROWS, 12), f32)
    for r in range(ROWS):
        w = rng.normal(0, 0.002, 3)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Rn = (np.eye(3) + K + 0.5 * K @ K) @ R[r]
        Tcw[r] = np.c_[Rn, t[r] + rng.normal(0, 0.02, 3)].reshape(12)
    world = (X + rng.normal(0, 0.05, X.shape)).astype(f32)
    tables = dict(kf_bad=np.zeros(ROWS, u8), kf_id=np.arange(ROWS, dtype=i32), obs_start=(np.arange(NPTS + 1) * SEEN).astype(i32),
                  obs_kf=obs_kf.reshape(-1), obs_idx=obs_idx.reshape(-1), flags=np.ones(NPTS, u8), kps=kps, u_right=ur, Tcw=Tcw,
                  world=world)
    apply = dict(origins=np.array([0], i32), parent=np.arange(-1, ROWS - 1, dtype=i32), ref_kf=obs_kf[:, 0].copy())
    return tables, apply


# ---- the host route: the same rules in vectorised numpy ----------------------------------------------------------------------------
def exp_se3(u):
    w, up = u[:, :3], u[:, 3:]
    th = np.linalg.norm(w, axis=1)
    Om = np.zeros((len(u), 3, 3))
    Om[:, 0, 1], Om[:, 0, 2], Om[:, 1, 0], Om[:, 1, 2], Om[:, 2, 0], Om[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    Om2 = Om @ Om
    small = th < 1e-5
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(ths) / ths)[:, None, None]
    b = np.where(small, 1.0, (1 - np.cos(ths)) / ths ** 2)[:, None, None]
    c = np.where(small, 1.0, (ths - np.sin(ths)) / ths ** 3)[:, None, None]
    I = np.eye(3)[None]
    R = I + a * Om + b * Om2
    V = np.where(small[:, None, None], R, I + b * Om + c * Om2)
    return R, np.einsum("nij,nj->ni", V, up)


def numpy_gba(t, iterations):
    """Optimizer::BundleAdjustment without kernel over every row and point (row 0 fixed): returns Tcw [rows, 12], world, trials."""
    fx, fy, cx, cy, bf = (float(f32(v)) for v in CAM)
    rows, npts = len(t["kf_id"]), len(t["flags"])
    T = t["Tcw"].astype(f64).reshape(rows, 3, 4)
    Rs, ts, X = T[:, :, :3].copy(), T[:, :, 3].copy(), t["world"].astype(f64)
    ekf, eidx = t["obs_kf"].astype(np.int64), t["obs_idx"].astype(np.int64)
    ept = np.repeat(np.arange(npts), np.diff(t["obs_start"]))
    ne = len(ekf)
    u, v, r_ = t["kps"]["x"][ekf, eidx].astype(f64), t["kps"]["y"][ekf, eidx].astype(f64), t["u_right"][ekf, eidx].astype(f64)
    st = ~(r_ < 0)
    inv = INV_SIGMA2[t["kps"]["octave"][ekf, eidx]].astype(f64)
    free = ekf - 1                                                              # row 0 is fixed: free pose f = row - 1
    nf = rows - 1
    slot = np.arange(ne) - t["obs_start"][ept]
    S_max = int(slot.max()) + 1

    def errors(Rs, ts, X):
        P = np.einsum("eij,ej->ei", Rs[ekf], X[ept]) + ts[ekf]
        invz = 1.0 / P[:, 2]
        e = np.stack([u - (P[:, 0] * invz * fx + cx), v - (P[:, 1] * invz * fy + cy),
                      np.where(st, r_ - (P[:, 0] * invz * fx + cx - bf * invz), 0.0)], 1)
        return e, P

    lam = ni = 0.0
    nbad = trials = 0
    for it in range(iterations):
        e, P = errors(Rs, ts, X)
        cur = float((inv * (e * e).sum(1)).sum())
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        z2 = z * z
        Jc = np.zeros((ne, 3, 6))
        Jc[:, 0] = np.stack([x * y / z2 * fx, -(1 + x * x / z2) * fx, y / z * fx, -fx / z, 0 * z, x / z2 * fx], 1)
        Jc[:, 1] = np.stack([(1 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy, 0 * z, -fy / z, y / z2 * fy], 1)
        Jc[:, 2] = Jc[:, 0] + np.stack([-bf * y / z2, bf * x / z2, 0 * z, 0 * z, 0 * z, -bf / z2], 1)
        A = np.zeros((ne, 3, 3))
        A[:, 0, 0], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2] = fx / z, -x / z2 * fx, fy / z, -y / z2 * fy
        A[:, 2] = A[:, 0]
        A[:, 2, 2] += bf / z2
        Jp = -A @ Rs[ekf]
        Jc[~st, 2], Jp[~st, 2] = 0.0, 0.0
        w = inv[:, None, None]
        Hpp_e, Hll_e, B_e = np.einsum("eri,erj->eij", Jc * w, Jc), np.einsum("eri,erj->eij", Jp * w, Jp), np.einsum("eri,erj->eij", Jc * w, Jp)
        bp_e, bl_e = -np.einsum("eri,er->ei", Jc * w, e), -np.einsum("eri,er->ei", Jp * w, e)
        isf = free >= 0
        Hpp, bp = np.zeros((nf, 6, 6)), np.zeros((nf, 6))
        np.add.at(Hpp, free[isf], Hpp_e[isf]); np.add.at(bp, free[isf], bp_e[isf])
        Hll, bl = np.zeros((npts, 3, 3)), np.zeros((npts, 3))
        np.add.at(Hll, ept, Hll_e); np.add.at(bl, ept, bl_e)
        if it == 0:
            lam = 1e-5 * max(np.abs(np.einsum("fii->fi", Hpp)).max(), np.abs(np.einsum("pii->pi", Hll)).max())
            ni, nbad = 2.0, 0
        ini, q, rho = cur, 0, 0.0
        # the edges of a point by slot, padded: Bs[s] is the block of slot s (zero where the point has no such edge or it is fixed)
        Bs, fs = np.zeros((S_max, npts, 6, 3)), np.full((S_max, npts), -1, np.int64)
        Bs[slot[isf], ept[isf]] = B_e[isf]
        fs[slot[isf], ept[isf]] = free[isf]
        while True:
            Dinv = np.linalg.inv(Hll + lam * np.eye(3)[None])
            S = np.zeros((nf, 6, nf, 6))
            S[np.arange(nf), :, np.arange(nf), :] = Hpp + lam * np.eye(6)[None]
            bs = bp.copy()
            for a in range(S_max):
                BD = Bs[a] @ Dinv
                ok_a = fs[a] >= 0
                np.add.at(bs, fs[a][ok_a], -np.einsum("pij,pj->pi", BD[ok_a], bl[ok_a]))
                for c in range(S_max):
                    ok = ok_a & (fs[c] >= 0)
                    Y = BD[ok] @ np.transpose(Bs[c][ok], (0, 2, 1))
                    np.subtract.at(S, (fs[a][ok][:, None, None], np.arange(6)[None, :, None], fs[c][ok][:, None, None], np.arange(6)[None, None, :]), Y)
            ok2 = True
            try:
                xp = np.linalg.solve(S.reshape(6 * nf, 6 * nf), bs.reshape(-1)).reshape(nf, 6)
            except np.linalg.LinAlgError:
                ok2, xp = False, np.zeros((nf, 6))
            c = bl.copy()
            np.add.at(c, ept[isf], -np.einsum("eij,ei->ej", B_e[isf], xp[free[isf]]))
            xl = np.einsum("pij,pj->pi", Dinv, c)
            dR, dt = exp_se3(xp)
            Rn, tn = Rs.copy(), ts.copy()
            Rn[1:], tn[1:] = dR @ Rs[1:], np.einsum("fij,fj->fi", dR, ts[1:]) + dt
            Xn = X + xl
            e2, _ = errors(Rn, tn, Xn)
            tmp = float((inv * (e2 * e2).sum(1)).sum()) if ok2 else 1.7976931348623157e308
            scale = float((xp * (lam * xp + bp)).sum() + (xl * (lam * xl + bl)).sum()) + 1e-3
            rho = (cur - tmp) / scale
            trials += 1
            if rho > 0 and math.isfinite(tmp):
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                ni, cur = 2.0, tmp
                Rs, ts, X = Rn, tn, Xn
            else:
                lam *= ni
                ni *= 2
            q += 1
            if not (rho < 0 and q < 10):
                break
        if q == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    return np.concatenate([Rs, ts[:, :, None]], 2).reshape(rows, 12).astype(f32), X.astype(f32), trials


KERNEL_GROUPS = dict(setup=("k_gba_setup", "k_gba_index", "k_gba_covis"), linearisation=("k_gba_linearize", "k_gba_blocks", "k_gba_begin"),
                     schur=("k_gba_dinv", "k_gba_schur"), factorisation=("k_factor_diag", "k_factor_panel", "k_factor_trail"),
                     substitution=("k_fwd_diag", "k_fwd_upd", "k_dscale", "k_bwd_diag", "k_bwd_upd"),
                     rest=("k_gba_x", "k_gba_update", "k_gba_trial", "k_gba_judge", "k_gba_finish"),
                     apply=("k_gba_apply_walk", "k_gba_apply_points"))


def kernel_split(path):
    per = {}
    if path.endswith(".db"):                                                    # rocprofv3's default output: the top_kernels view, in us
        import sqlite3
        rows = [{"Name": n, "Calls": c, "TotalDurationNs": float(us) * 1e3}
                for n, c, us in sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels")]
    else:
        rows = list(csv.DictReader(open(path)))
    for row in rows:
        name = row.get("Name") or row.get("KernelName") or ""
        total = row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or row.get("TotalDurationNS")
        calls = row.get("Calls") or row.get("Count")
        for k in sum(KERNEL_GROUPS.values(), ()):
            if k + "<" in name or k + "E" in name or k + "(" in name or name.endswith(k) or ("::" + k + "I") in name or (k + "I") in name:
                per.setdefault(k, {"calls": 0, "us": 0.0})
                per[k]["calls"] += int(calls); per[k]["us"] += float(total) / 1e3
    groups = {g: {"us": sum(per[k]["us"] for k in ks if k in per), "launches": sum(per[k]["calls"] for k in ks if k in per)}
              for g, ks in KERNEL_GROUPS.items()}
    return {"per_kernel": per, "groups": groups, "from": "rocprofv3 --kernel-trace --stats of one call in a run of its own (tracing slows "
                                                         "the host; kernel durations only)"}


def headline(path, parent_label):
    runs = {"parent": [], "new": []}
    for ln in open(path):
        if ln.startswith("["):
            label, rest = ln[1:].split("]", 1)
            runs["parent" if parent_label in label else "new"].append(float(rest.split()[0]))
    lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
    return {"how": "bench.py --gpus 1 --steps 30 --warmup 5, interleaved parent / new for as many rounds as the log holds (the log may join "
                   "several calls, each on one box: compare a round's pair, and the spreads); the parent is the parent commit's whole tree "
                   "with its own library; the headline does not run this path",
            "unit": "frames/s, higher is better", "parent_runs": runs["parent"], "new_runs": runs["new"], "parent_spread": [lo, hi],
            "new_within_parent_spread": [bool(lo <= v <= hi) for v in runs["new"]] if lo is not None else None}


SCHEMA = ("what", "status", "reps", "report", "apply_report", "panel_poses", "synchronisations", "launches", "a_device", "b_host_route_us",
          "b_reps", "b_is", "b_trials", "b_max_pose_distance_from_a", "b_max_point_distance_from_a_m", "clocks", "b_over_a", "kernel_split",
          "c_headline")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true", help="one device call plus apply and nothing else: the run a kernel trace is taken of")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--unmeasured", action="store_true")
    ap.add_argument("--from-measured", help="a document this tool wrote on the GPU: add --kernel-stats / --ab-log to it, measure nothing")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--ab-log")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gba_stage.json"))
    args = ap.parse_args()
    what = ("Optimizer::GlobalBundleAdjustemnt (STAGED, %d iterations, no kernel) plus the map update of RunGlobalBundleAdjustment, one "
            "call each: a ring of %d key frames, %d map points seen by %d key frames each" % (ITERATIONS, ROWS, NPTS, SEEN))
    if args.unmeasured:
        doc = {k: None for k in SCHEMA}
        doc.update(what=what, status="unmeasured")
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    if args.from_measured:                                                      # no GPU: add the trace split and the headline log
        doc = json.load(open(args.from_measured))
        if args.kernel_stats:
            doc["kernel_split"] = kernel_split(args.kernel_stats)
        if args.ab_log:
            doc["c_headline"] = headline(args.ab_log, args.parent_label)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    t, ap_ = scene()
    import torch
    from orb_slam2_comment_amd import capi
    from orb_slam2_comment_amd.matcher import make_camera
    import orb_slam2_comment_amd as pkg
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(*CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=CAM[4])
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731
    d_t = {k: up(v) for k, v in t.items()}
    d_T0, d_w0 = up(t["Tcw"]), up(t["world"])
    d_o = dict(TcwGBA=up(np.zeros((ROWS, 12), f32)), posGBA=up(np.zeros((NPTS, 3), f32)), kf_mark=up(np.zeros(ROWS, u8)),
               pt_mark=up(np.zeros(NPTS, u8)), report=up(np.zeros(16, i32)))
    d_a = dict(origins=up(ap_["origins"]), parent=up(ap_["parent"]), kf_bad=d_t["kf_bad"], kf_mark=d_o["kf_mark"], TcwGBA=d_o["TcwGBA"],
               Tcw=d_t["Tcw"], pt_mark=d_o["pt_mark"], posGBA=d_o["posGBA"], flags=d_t["flags"], ref_kf=up(ap_["ref_kf"]), world=d_t["world"],
               TcwBefGBA=up(np.zeros((ROWS, 12), f32)), report=up(np.zeros(8, i32)))
    ne = int(t["obs_start"][-1])

    def device_call():
        d_t["Tcw"].copy_(d_T0, non_blocking=True)
        d_t["world"].copy_(d_w0, non_blocking=True)
        d_o["kf_mark"].zero_(); d_o["pt_mark"].zero_()
        m.GlobalBundleAdjustmentDevice(cam, ROWS, CAP, NPTS, NPTS, d_t, INV_SIGMA2, ITERATIONS, 0, capi.GBA_STAGED, NPTS, ne, d_o)
        m.ApplyGlobalBADevice(1, ROWS, NPTS, d_a)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        device_call()
    m.sync()
    rep = d_o["report"].cpu().numpy().view(i32).tolist()
    arep = d_a["report"].cpu().numpy().view(i32).tolist()
    syncs, launches = m.GlobalBACounters()
    if args.once:
        print(json.dumps({"report": rep, "apply_report": arep, "syncs": syncs, "launches": launches}))
        m.close()
        return
    for _ in range(args.warmup):
        with torch.cuda.stream(stream):
            device_call()
    a, aw = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        a.append(timed_events(device_call))
        aw.append((time.perf_counter() - t0) * 1e6)
    med = lambda v: float(np.median(v))  # noqa: E731
    dev = {"us_median": med(a), "us_min": float(min(a)), "us_max": float(max(a)), "wall_us_median": med(aw)}
    got_T = d_t["Tcw"].cpu().numpy().view(f32).reshape(-1, 12)
    got_w = d_t["world"].cpu().numpy().view(f32).reshape(-1, 3)
    doc = {k: None for k in SCHEMA}
    doc.update(what=what + "; the timed call includes the device copies that restore Tcw and world and clear the marks", status="measured",
               reps=args.reps, report=dict(zip(capi.GBA_REPORT, rep)), apply_report=dict(zip(capi.GBA_APPLY_REPORT, arep)), panel_poses=4,
               synchronisations=syncs, launches=launches, a_device=dev,
               clocks="a: HIP events on the matcher's stream around the synchronising call and the apply step, and the wall clock; b: wall clock")
    if not args.no_host_route:
        t0 = time.perf_counter()
        down = {k: d_t[k].cpu().numpy().view(np.asarray(t[k]).dtype).reshape(np.asarray(t[k]).shape) for k in t if k not in ("Tcw", "world")}
        down["Tcw"], down["world"] = d_T0.cpu().numpy().view(f32).reshape(-1, 12), d_w0.cpu().numpy().view(f32).reshape(-1, 3)
        Tn, Xn, trials = numpy_gba(down, ITERATIONS)                            # every row and point is optimised: the apply step is
        up(Tn); up(Xn)                                                          # Tcw = TcwGBA, world = posGBA
        torch.cuda.synchronize()
        bb = (time.perf_counter() - t0) * 1e6
        doc.update(b_host_route_us=bb, b_reps=1, b_trials=trials,
                   b_is="D2H of the tables + the same rules in vectorised numpy (Schur complement by scatter-adds, the reduced system "
                        "through numpy.linalg.solve, LAPACK) + H2D of the poses and points; numpy, NOT g2o: the reference's C++ is not "
                        "measured, so b_over_a is no claim against it",
                   b_max_pose_distance_from_a=float(np.abs(got_T - Tn).max()), b_max_point_distance_from_a_m=float(np.abs(got_w - Xn).max()),
                   b_over_a=bb / med(a))
    if args.kernel_stats:
        doc["kernel_split"] = kernel_split(args.kernel_stats)
    if args.ab_log:
        doc["c_headline"] = headline(args.ab_log, args.parent_label)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    m.close()


if __name__ == "__main__":
    main()
