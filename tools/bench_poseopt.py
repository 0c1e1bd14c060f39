#!/usr/bin/env python3
"""Cost of Optimizer::PoseOptimization on the device and of the host round trip it replaces, same process, same inputs.

  (a) PoseOptimizationDevice(DISCARD) for one 1241 x 376 frame of 1000 slots (cap 1024) with 300 edges and with 600 edges
      (a fifth displaced, half stereo), and for a batch of 64 such frames of 300 edges.  The figure of merit is the latency
      of one frame: the function is a serial chain of small reductions.  Warm, HIP-event time on the matcher's stream,
      median over --reps.
  (a2) PoseOptimization, the host form of the 300-edge call (one staged copy, the launch, one read-back).  Wall clock.
  (b) what a caller had to do without the entry: D2H of frame_point, the touched world row and the key points, then the
      same rules in vectorised numpy (rotation matrices, numpy.linalg.solve), H2D of the pose and the flags.  Wall clock.
      This host route is numpy, NOT g2o: g2o needs Eigen, which is not available to this project's build, so b / a is no
      claim against the reference's C++.  (b) is checked for sanity: it must flag the same slots as the device.
  (c) optionally the log of a headline A/B (lines "[label] value ...", parent and new interleaved in one call on one box).

  python tools/bench_poseopt.py [--reps 30] [--warmup 3] [--lib PATH --team 64] [--ab-log FILE] [--out profiles/poseopt_stage.json]
  python tools/bench_poseopt.py --host-only     # no GPU: builds the scenes and runs route (b)'s arithmetic once

--lib times another build of the library (make EXTRA=-DORBHIP_POSEOPT_TEAM=64: the one-wavefront team) and merges its
device times into the JSON under "team_<n>"; that build sums in another order, so only its flags are compared.
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
N, CAP, BATCH = 1000, 1024, 64


def scenes():
    import test_poseopt_cpu as K
    one300 = K.batch_of([K.make_frame(41, 300, 60, 0.5, CAP, n=N)], CAP, shared=True, mode=1)
    one600 = K.batch_of([K.make_frame(42, 600, 120, 0.5, CAP, n=N)], CAP, shared=True, mode=1)
    many = K.batch_of([K.make_frame(100 + k, 300, 60, 0.5, CAP, n=N) for k in range(BATCH)], CAP, mode=1)
    return K, one300, one600, many


def host_rules(K, kps, n, u_right, world, fp, Tcw):
    """The rules of tests/seqref/poseopt.py for one frame in vectorised numpy; returns (Tcw [12] float32, outlier [cap])."""
    fx, fy, cx, cy, bf = (float(f32(v)) for v in K.CAM)
    idx = np.flatnonzero(fp[:n] >= 0)
    X = world[fp[idx]].astype(f64)
    ur = u_right[idx].astype(f64)
    st = ~(ur < 0)
    obs = np.c_[kps["x"][idx], kps["y"][idx], ur].astype(f64)
    inv = K.INV_SIGMA2[kps["octave"][idx]].astype(f64)
    delta = np.where(st, float(f32(math.sqrt(7.815))), float(f32(math.sqrt(5.991))))
    thr = np.where(st, f32(7.815), f32(5.991))
    T0 = Tcw.astype(f64).reshape(3, 4)
    u_, _, vt = np.linalg.svd(T0[:, :3])
    R0, t0 = u_ @ vt, T0[:, 3]

    def errs(R, t):
        P = X @ R.T + t
        invz = np.where(st, (1.0 / P[:, 2]).astype(f32).astype(f64), 1.0 / P[:, 2])
        p0, p1 = P[:, 0] * invz * fx + cx, P[:, 1] * invz * fy + cy
        e = np.c_[obs[:, 0] - p0, obs[:, 1] - p1, np.where(st, obs[:, 2] - (p0 - bf * invz), 0.0)]
        return e, (e * e).sum(1) * inv, P

    def rob(c, kernel):
        if not kernel:
            return c, np.ones_like(c)
        s = np.sqrt(np.maximum(c, 1e-300))
        big = c > delta * delta
        return np.where(big, 2 * s * delta - delta * delta, c), np.where(big, delta / s, 1.0)

    def exp(u):
        om, up = u[:3], u[3:]
        th = math.sqrt(om @ om)
        O = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
        if th < 1e-5:
            R = np.eye(3) + O + O @ O
            return R, R @ up
        R = np.eye(3) + math.sin(th) / th * O + (1 - math.cos(th)) / th ** 2 * O @ O
        V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * O + (th - math.sin(th)) / th ** 3 * O @ O
        return R, V @ up

    def system(R, t, act, kernel):
        e, c, P = errs(R, t)
        rho0, rho1 = rob(c, kernel)
        x, y, iz = P[:, 0], P[:, 1], 1.0 / P[:, 2]
        z0 = np.zeros_like(x)
        J0 = np.stack([x * y * iz * iz * fx, -(1 + x * x * iz * iz) * fx, y * iz * fx, -iz * fx, z0, x * iz * iz * fx], 1)
        J1 = np.stack([(1 + y * y * iz * iz) * fy, -x * y * iz * iz * fy, -x * iz * fy, z0, -iz * fy, y * iz * iz * fy], 1)
        J2 = np.stack([J0[:, 0] - bf * y * iz * iz, J0[:, 1] + bf * x * iz * iz, J0[:, 2], J0[:, 3], z0, J0[:, 5] - bf * iz * iz], 1)
        J = np.stack([J0, J1, J2 * st[:, None]], 1)[act]
        w = (rho1 * inv)[act]
        H = np.einsum("erk,e,erl->kl", J, w, J)
        g = -np.einsum("erk,e,er->k", J, w, e[act])
        return H, g, rho0[act].sum()

    out = np.zeros(len(idx), bool)
    x = np.zeros(6)
    R, t = R0, t0
    for rnd in range(4):
        R, t = R0, t0
        Rt, tt = R, t
        kernel, act = rnd < 3, ~out
        lam = ni = 0.0
        nbad = 0
        for it in range(10):
            H, g, cur = system(R, t, act, kernel)
            ini = cur
            if it == 0:
                lam, ni, nbad = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
            q = 0
            while True:
                try:
                    L = np.linalg.cholesky(H + lam * np.eye(6))
                    x = np.linalg.solve(L.T, np.linalg.solve(L, g))
                    ok = True
                except np.linalg.LinAlgError:
                    ok = False
                dR, dtv = exp(x)
                Rt, tt = dR @ R, dR @ t + dtv
                tmp = rob(errs(Rt, tt)[1], kernel)[0][act].sum() if ok else 1.7976931348623157e308
                rho = (cur - tmp) / (x @ (lam * x + g) + 1e-3)
                if rho > 0 and math.isfinite(tmp):
                    lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                    ni, cur, R, t = 2.0, tmp, Rt, tt
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
        c = np.where(out, errs(R, t)[1], errs(Rt, tt)[1])
        out = c.astype(f32) > thr
        if len(idx) < 10:
            break
    flags = np.zeros(len(fp), u8)
    flags[idx[out]] = 1
    return np.c_[R, t].astype(f32).ravel(), flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--team", type=int, default=256)
    ap.add_argument("--ab-log")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseopt_stage.json"))
    args = ap.parse_args()
    K, one300, one600, many = scenes()
    if args.host_only:
        for b in (one300, one600):
            t0 = time.perf_counter()
            T, fl = host_rules(K, b["kps"][0], int(b["n"][0]), b["u_right"][0], b["world"][0], b["frame_point"][0], b["Tcw"][0])
            print("host rules once: %.1f ms, %d flagged" % ((time.perf_counter() - t0) * 1e3, int(fl.sum())))
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
    cam = make_camera(*K.CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=K.CAM[4])
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731

    def prepare(b):
        d = {k: up(b[k]) for k in ("kps", "n", "u_right", "world", "point_flags", "world_row")}
        o = K.prefilled(b)
        d.update({k: up(o[k]) for k in o})
        d["Tcw0"], d["fp0"] = up(b["Tcw"]), up(b["frame_point"])
        return d

    def device_call(b, d):
        d["Tcw"].copy_(d["Tcw0"], non_blocking=True)
        d["frame_point"].copy_(d["fp0"], non_blocking=True)
        m.PoseOptimizationDevice(b["frames"], d["kps"], d["n"], b["cap"], d["u_right"], d["world"], d["point_flags"], b["wrows"], b["pcap"],
                                 d["world_row"], cam, K.INV_SIGMA2, d["Tcw"], d["frame_point"], d["outlier"], d["discarded"], d["report"],
                                 mode=b["mode"], flags=b["flags"])

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def timed_wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    sets = [("one_frame_300_edges", one300, prepare(one300)), ("one_frame_600_edges", one600, prepare(one600)),
            ("batch_64_frames_300_edges", many, prepare(many))]
    torch.cuda.synchronize()
    # sanity: the device flags the displaced slots route (b) flags
    reports = {}
    for name, b, d in sets:
        with torch.cuda.stream(stream):
            device_call(b, d)
        m.sync()
        rep = d["report"].cpu().numpy().view(i32).reshape(-1, 8)
        dis = d["discarded"].cpu().numpy().view(i32).reshape(b["frames"], b["cap"])
        T, fl = host_rules(K, b["kps"][0], int(b["n"][0]), b["u_right"][0], b["world"][int(b["world_row"][0]) if b["world_row"] is not None else 0],
                           b["frame_point"][0], b["Tcw"][0])
        assert np.array_equal(np.flatnonzero(dis[0][:N] >= 0), np.flatnonzero(fl)), name
        assert np.abs(T - d["Tcw"].cpu().numpy().view(f32)[:12]).max() < 1e-4, name
        reports[name] = rep[0].tolist()

    def host_form():
        b = one300
        m.PoseOptimization(b["kps"], b["n"], b["u_right"], b["world"], b["point_flags"], b["world_row"], cam, K.INV_SIGMA2, b["Tcw"],
                           b["frame_point"], mode=b["mode"], flags=b["flags"])

    def round_trip(b, d):
        fp = d["fp0"].cpu().numpy().view(i32).reshape(b["frames"], b["cap"])
        world = d["world"].cpu().numpy().view(f32).reshape(b["wrows"], b["pcap"], 3)
        kps = d["kps"].cpu().numpy().view(K.KP_DTYPE).reshape(b["frames"], b["cap"])
        ur = d["u_right"].cpu().numpy().view(f32).reshape(b["frames"], b["cap"])
        T, fl = host_rules(K, kps[0], int(b["n"][0]), ur[0], world[0], fp[0], b["Tcw"][0])
        up(T); up(fl)
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        for name, b, d in sets:
            with torch.cuda.stream(stream):
                device_call(b, d)
        host_form()
    m.sync()
    times = {name: [] for name, _, _ in sets}
    a2, b300, b600 = [], [], []
    for _ in range(args.reps):
        for name, b, d in sets:
            times[name].append(timed_events(lambda: device_call(b, d)))
        if not args.lib:
            a2.append(timed_wall(host_form))
            b300.append(timed_wall(lambda: round_trip(one300, sets[0][2])))
            b600.append(timed_wall(lambda: round_trip(one600, sets[1][2])))
    med = lambda v: float(np.median(v))  # noqa: E731
    dev = {name: {"us_median": med(v), "us_min": float(min(v)), "us_max": float(max(v)), "report": reports[name]} for name, v in times.items()}
    if args.lib:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["team_%d" % args.team] = {"how": "the same calls against a build with -DORBHIP_POSEOPT_TEAM=%d" % args.team, "a_device": dev}
    else:
        doc = {"what": "Optimizer::PoseOptimization with the DISCARD epilogue: a frame of 1000 slots at cap 1024, 300 or 600 edges, a fifth "
                       "displaced by 12-30 px * sigma, half stereo; the timed call includes the two device copies that restore the "
                       "in/out pose and frame_point.  One workgroup of %d lanes per frame, one launch." % args.team,
               "status": "measured", "reps": args.reps, "team": args.team, "a_device": dev,
               "a2_host_form_300_edges_us_median": med(a2), "a2_host_form_300_edges_us_min": float(min(a2)),
               "b_host_round_trip_300_edges_us_median": med(b300), "b_host_round_trip_300_edges_us_min": float(min(b300)),
               "b_host_round_trip_600_edges_us_median": med(b600), "b_host_round_trip_600_edges_us_min": float(min(b600)),
               "b_is": "download + the same rules in vectorised numpy (LAPACK) + upload; numpy, NOT g2o: g2o cannot be built without "
                       "Eigen, so b_over_a is no claim against the reference's C++",
               "clocks": "a: HIP events on the matcher's stream; a2, b: wall clock of synchronous host work",
               "b_over_a_300_edges": med(b300) / dev["one_frame_300_edges"]["us_median"],
               "b_over_a_600_edges": med(b600) / dev["one_frame_600_edges"]["us_median"]}
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
