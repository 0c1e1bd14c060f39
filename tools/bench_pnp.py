#!/usr/bin/env python3
"""Cost of the PnP RANSAC of Tracking::Relocalization on the device and of the host round trip it replaces, same process,
same inputs.

  (a) PnpSetupDevice + PnpIterateDevice for C = 5 candidates of 100 correspondences each (70 under one pose with 0.5 px of
      noise, 30 random), a frame of 1000 slots at cap 1024, the matches as the slots orbhip_search_by_bow_device writes,
      SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), iterate(5) on fresh solvers as Relocalization calls it: the OR of
      the loop condition makes that the 35 iterations of the limit.  Warm, HIP-event time on the matcher's stream, median
      over --reps.  (a300) the same with iterate(300), i.e. PnPsolver::find: 300 iterations per candidate are computed.
  (a2) PnpRansac, the host form of (a) (one staged copy, the two calls, one read-back).  Wall clock.
  (b) what a caller had to do without the entries: D2H of the matches, then the logic of tests/seqref/pnp.py vectorised
      in numpy over the hypotheses of a candidate (fp64, numpy.linalg in place of the Jacobi routines), Refine() on the
      record-setters, H2D of the poses and the inlier marks.  Wall clock, median over --reps.  The four-point hypotheses
      of the two routes differ in the null-space basis, so (b) is checked for sanity only: every candidate must return a
      refined pose whose inlier set holds at least 60 of the 70 clean matches.
  (c) optionally the log of a headline A/B (lines "[label] value ...", parent and new interleaved in one call on one box);
      the numbers are copied into the JSON.  The parent runs from its own tree: its binding declares fewer symbols.

  python tools/bench_pnp.py [--reps 20] [--warmup 3] [--ab-log FILE --parent-label SUBSTR] [--out profiles/pnp_stage.json]
  python tools/bench_pnp.py --host-only     # no GPU: builds the scene and runs route (b)'s arithmetic once
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C_, NCORR, NGOOD, N, CAP, ROWS = 5, 100, 70, 1000, 1024, 5
PRM = dict(prob=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991)
FX, FY, CX, CY = 718.856, 718.856, 607.1928, 185.2157
i32, u8, f32, f64 = np.int32, np.uint8, np.float32, np.float64
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], f32)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])


def rot(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_scene(seed=1):
    rng = np.random.default_rng(seed)
    R, t = rot([0.3, 1.0, 0.2], 0.25), np.array([0.3, -0.1, 0.5])
    kps = np.zeros(N, KP_DTYPE)
    kps["octave"] = rng.integers(0, 8, N)
    z = rng.uniform(4.0, 40.0, N)
    Xc = np.stack([rng.uniform(-0.6, 0.6, N) * z, rng.uniform(-0.2, 0.2, N) * z, z], 1)
    kps["x"], kps["y"] = FX * Xc[:, 0] / z + CX, FY * Xc[:, 1] / z + CY
    world, good = [], np.zeros((C_, N), bool)
    m_slots, slot_point = np.full((C_, CAP), -1, i32), np.full((ROWS, CAP), -1, i32)
    for c in range(C_):
        slots = np.sort(rng.choice(N, NCORR, replace=False))
        bad = set(rng.choice(NCORR, NCORR - NGOOD, replace=False).tolist())
        bank = rng.permutation(CAP)
        for k, s in enumerate(slots):
            x = Xc[s] + np.r_[rng.normal(0, 0.5, 2) * z[s] / FX, 0]
            w = rng.uniform(-30, 30, 3) if k in bad else (x - t) @ R
            good[c, s] = k not in bad
            m_slots[c, s], slot_point[c, bank[k]] = bank[k], len(world)
            world.append(w)
    pmap = dict(flags=np.ones(len(world), u8), world=np.array(world, f32), slot_point=slot_point)
    return dict(kps=kps, m_slots=m_slots, kf_index=np.arange(C_, dtype=i32), map=pmap, good=good, R=R, t=t)


# ---- route (b): the seqref's logic in vectorised numpy, LAPACK in place of the Jacobi routines ------------------------------
def epnp(pw, us):
    """EPnP for a batch: pw [H, n, 3], us [H, n, 2] -> R [H, 3, 3], t [H, 3]."""
    H, n = pw.shape[:2]
    c0 = pw.mean(1)
    P0 = pw - c0[:, None]
    w, v = np.linalg.eigh(np.einsum("hni,hnj->hij", P0, P0))
    w, v = w[:, ::-1], v[:, :, ::-1]
    big = np.abs(v).argmax(1)
    sgn = np.where(np.take_along_axis(v, big[:, None, :], 1)[:, 0] < 0, -1.0, 1.0)
    v = v * sgn[:, None, :]
    with np.errstate(all="ignore"):
        cws = np.concatenate([c0[:, None], c0[:, None] + (np.sqrt(w / n)[:, :, None] * v.transpose(0, 2, 1))], 1)   # [H, 4, 3]
        cc = (cws[:, 1:] - cws[:, :1]).transpose(0, 2, 1)
        a123 = np.einsum("hij,hnj->hni", np.linalg.pinv(cc), P0)
        al = np.concatenate([1.0 - a123.sum(2, keepdims=True), a123], 2)                                            # [H, n, 4]
        M = np.zeros((H, n, 2, 4, 3))
        M[:, :, 0, :, 0], M[:, :, 0, :, 2] = al * FX, al * (CX - us[:, :, 0:1])
        M[:, :, 1, :, 1], M[:, :, 1, :, 2] = al * FY, al * (CY - us[:, :, 1:2])
        M = M.reshape(H, 2 * n, 12)
        _, ev = np.linalg.eigh(M.transpose(0, 2, 1) @ M)
        V = ev[:, :, :4].transpose(0, 2, 1).reshape(H, 4, 4, 3)                                                     # v[i] = i-th smallest
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = np.stack([V[:, :, a] - V[:, :, b] for a, b in pairs], 2)                                               # [H, 4, 6, 3]
        d = lambda i, j: np.einsum("hpk,hpk->hp", dv[:, i], dv[:, j])                                               # noqa: E731
        L = np.stack([d(0, 0), 2 * d(0, 1), d(1, 1), 2 * d(0, 2), 2 * d(1, 2), d(2, 2), 2 * d(0, 3), 2 * d(1, 3), 2 * d(2, 3), d(3, 3)], 2)
        rho = np.stack([((cws[:, a] - cws[:, b]) ** 2).sum(1) for a, b in pairs], 1)
        best = None
        for which, cols in ((1, (0, 1, 3, 6)), (2, (0, 1, 2)), (3, (0, 1, 2, 3, 4))):
            b = np.einsum("hij,hj->hi", np.linalg.pinv(L[:, :, cols]), rho)
            be = np.zeros((H, 4))
            neg = b[:, 0] < 0
            be[:, 0] = np.sqrt(np.abs(b[:, 0]))
            if which == 1:
                be[:, 1:] = np.where(neg[:, None], -b[:, 1:], b[:, 1:]) / be[:, :1]
            else:
                be[:, 1] = np.where(neg, np.sqrt(np.maximum(-b[:, 2], 0)), np.sqrt(np.maximum(b[:, 2], 0)))
                be[:, 0] = np.where(b[:, 1] < 0, -be[:, 0], be[:, 0])
                if which == 3:
                    be[:, 2] = b[:, 3] / be[:, 0]
            for _ in range(5):                                                                                       # gauss_newton
                b0, b1, b2, b3 = (be[:, i:i + 1] for i in range(4))
                A = np.stack([2 * L[:, :, 0] * b0 + L[:, :, 1] * b1 + L[:, :, 3] * b2 + L[:, :, 6] * b3,
                              L[:, :, 1] * b0 + 2 * L[:, :, 2] * b1 + L[:, :, 4] * b2 + L[:, :, 7] * b3,
                              L[:, :, 3] * b0 + L[:, :, 4] * b1 + 2 * L[:, :, 5] * b2 + L[:, :, 8] * b3,
                              L[:, :, 6] * b0 + L[:, :, 7] * b1 + L[:, :, 8] * b2 + 2 * L[:, :, 9] * b3], 2)
                quad = np.stack([b0 * b0, b0 * b1, b1 * b1, b0 * b2, b1 * b2, b2 * b2, b0 * b3, b1 * b3, b2 * b3, b3 * b3], 2)[:, 0]
                r = rho - np.einsum("hpk,hk->hp", L, quad)
                ok = np.isfinite(A).all((1, 2)) & np.isfinite(r).all(1)
                x = np.zeros((H, 4))
                if ok.any():
                    x[ok] = np.einsum("hij,hj->hi", np.linalg.pinv(A[ok]), r[ok])
                be = be + x
            ccs = np.einsum("hi,hijk->hjk", be, V)
            pcs = np.einsum("hni,hik->hnk", al, ccs)
            flip = np.where(pcs[:, 0, 2] < 0, -1.0, 1.0)
            pcs = pcs * flip[:, None, None]
            pc0, pw0 = pcs.mean(1), pw.mean(1)
            abt = np.einsum("hnj,hnk->hjk", pcs - pc0[:, None], pw - pw0[:, None])
            ok = np.isfinite(abt).all((1, 2))
            R = np.full((H, 3, 3), np.nan)
            if ok.any():
                u, _, vt = np.linalg.svd(abt[ok])
                R[ok] = u @ vt
            R[:, 2] *= np.where(np.linalg.det(np.nan_to_num(R)) < 0, -1.0, 1.0)[:, None]
            t = pc0 - np.einsum("hij,hj->hi", R, pw0)
            X = np.einsum("hij,hnj->hni", R, pw) + t[:, None]
            ue, ve = CX + FX * X[:, :, 0] / X[:, :, 2], CY + FY * X[:, :, 1] / X[:, :, 2]
            err = np.sqrt((us[:, :, 0] - ue) ** 2 + (us[:, :, 1] - ve) ** 2).mean(1)
            if best is None:
                best = [R, t, err]
            else:
                take = err < best[2]
                best = [np.where(take[:, None, None], R, best[0]), np.where(take[:, None], t, best[1]), np.where(take, err, best[2])]
    return best[0], best[1]


def inliers_of(R, t, p3d, p2d, max_err):
    """CheckInliers for a batch of poses over one candidate's correspondences: [H, N] bool."""
    with np.errstate(all="ignore"):
        X = np.einsum("hij,nj->hni", R, p3d.astype(f64)) + t[:, None]
        Xc, Yc, inv = X[:, :, 0].astype(f32), X[:, :, 1].astype(f32), (1.0 / X[:, :, 2]).astype(f32)
        ue, ve = CX + FX * Xc.astype(f64) * inv, CY + FY * Yc.astype(f64) * inv
        dx, dy = (p2d[:, 0].astype(f64) - ue).astype(f32), (p2d[:, 1].astype(f64) - ve).astype(f32)
        return dx * dx + dy * dy < max_err


def host_route(sc, matches, draws):
    """setup + iterate(300) of every candidate in numpy; returns [(status, iteration, inlier slots, Tcw)]."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from seqref import pnp as P
    out = []
    for c in range(C_):
        S = fast_setup(sc, matches[c], c)
        Nc, n_min, limit = S["n_corr"], S["min_inliers"], S["limit"]
        idx = np.empty((limit, 4), np.int64)
        for it in range(limit):
            idx[it] = P.sample(Nc, draws[c][it])
        R, t = epnp(S["p3d"][idx].astype(f64), S["p2d"][idx].astype(f64))
        masks = inliers_of(R, t, S["p3d"], S["p2d"], S["max_err"])
        cnt, best, res = masks.sum(1), 0, (P.NO_MORE, -1, None, None)
        for it in range(limit):
            if cnt[it] >= n_min and cnt[it] > best:
                best = cnt[it]
                sel = np.flatnonzero(masks[it])
                Rr, tr = epnp(S["p3d"][sel][None].astype(f64), S["p2d"][sel][None].astype(f64))
                rm = inliers_of(Rr, tr, S["p3d"], S["p2d"], S["max_err"])[0]
                if rm.sum() > n_min:
                    res = (P.REFINED, it, S["kp_index"][rm], np.c_[Rr[0], tr[0]].astype(f32))
                    break
        out.append(res)
    return out


def fast_setup(sc, matches, c):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from seqref import pnp as P
    slots = np.flatnonzero(matches[:N] >= 0)
    p = sc["map"]["slot_point"][sc["kf_index"][c]][matches[slots]]
    keep = (p >= 0) & ((sc["map"]["flags"][np.maximum(p, 0)] & 1) != 0)
    slots, p = slots[keep], p[keep]
    n_min, limit = P.ransac_parameters(len(slots), **PRM)
    return dict(p2d=np.stack([sc["kps"]["x"][slots], sc["kps"]["y"][slots]], 1), p3d=sc["map"]["world"][p],
                max_err=SIGMA2[sc["kps"]["octave"][slots]] * f32(PRM["th2"]), kp_index=slots, n_corr=len(slots), min_inliers=n_min,
                limit=limit)


def check_host(sc, res):
    for c, (status, it, slots, T) in enumerate(res):
        assert status == 0, ("candidate %d did not return a refined pose" % c)
        assert sc["good"][c][slots].sum() >= 60, (c, int(sc["good"][c][slots].sum()))
        assert np.abs(T[:, :3] - sc["R"]).max() < 5e-3 and np.abs(T[:, 3] - sc["t"]).max() < 5e-2, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--ab-log")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_stage.json"))
    args = ap.parse_args()
    sc = make_scene()
    from orb_slam2_comment_amd.matcher import pnp_draws
    draws = pnp_draws([NCORR] * C_, PRM["max_its"], 7)
    if args.host_only:
        t0 = time.perf_counter()
        res = host_route(sc, sc["m_slots"], draws)
        check_host(sc, res)
        print("host route once: %.1f ms, returned iterations %s" % ((time.perf_counter() - t0) * 1e3, [r[1] for r in res]))
        return
    import torch
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    cam = make_camera(FX, FY, CX, CY, (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)])
    params = m.pnp_params(**PRM)
    solver = m.PnpSetup(sc["kps"], sc["m_slots"], 1, sc["kf_index"], sc["map"], cam, SIGMA2, params)
    rep, tcw, inl = m.PnpIterate(solver, draws, PRM["max_its"])
    assert (rep[:, 0] == 0).all(), rep
    for c in range(C_):
        slots = np.flatnonzero(inl[c][:N])
        assert sc["good"][c][slots].sum() >= 60 and np.abs(tcw[c].reshape(3, 4)[:, :3] - sc["R"]).max() < 5e-3, c
    res = host_route(sc, sc["m_slots"], draws)
    check_host(sc, res)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731
    d_draws, d_T, d_inl, d_rep = up(draws), up(np.zeros((C_, 12), f32)), up(np.zeros((C_, CAP), u8)), up(np.zeros((C_, 8), i32))
    d_k, d_m, d_kf = solver["keep"]
    n_pts = len(sc["map"]["flags"])

    def device_calls(n_iterations=5):
        m.PnpSetupDevice(C_, d_k, N, CAP, d_m, 1, d_kf, ROWS, n_pts, n_pts, solver["map"], cam, SIGMA2, params, solver["solvers"])
        m.PnpIterateDevice(C_, N, CAP, cam, params, solver["solvers"], d_draws, PRM["max_its"], n_iterations, d_T, d_inl, d_rep)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def timed_wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    def host_form():
        m.PnpRansac(sc["kps"], sc["m_slots"], 1, sc["kf_index"], sc["map"], cam, SIGMA2, draws, params, n_iterations=5)

    def round_trip():
        mt = d_m.cpu().numpy().view(i32).reshape(C_, CAP)
        r = host_route(sc, mt, draws)
        T = np.stack([x[3] for x in r])
        marks = np.zeros((C_, CAP), u8)
        for c, x in enumerate(r):
            marks[c, x[2]] = 1
        up(T); up(marks)
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        device_calls(); host_form()
    m.sync()
    a, a300, a2, b = [], [], [], []
    for _ in range(args.reps):
        a300.append(timed_events(lambda: device_calls(PRM["max_its"])))
        a.append(timed_events(device_calls))
        a2.append(timed_wall(host_form))
        b.append(timed_wall(round_trip))
    rep = d_rep.cpu().numpy().view(i32).reshape(C_, 8)
    med = lambda v: float(np.median(v))  # noqa: E731
    doc = {"what": "PnP RANSAC of Tracking::Relocalization: C = 5 candidates of 100 correspondences (70 clean at 0.5 px, 30 random), "
                   "frame of 1000 slots, cap 1024, SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), fresh solvers.  a, a2: iterate(5) as "
                   "Relocalization calls it, which the OR of the loop condition turns into the 35 iterations of the limit, all "
                   "computed; a300: iterate(300) = PnPsolver::find, 300 iterations computed per candidate; b: the 35 iterations "
                   "of the limit, stopping at the first refined return",
           "status": "measured", "candidates": C_, "cap": CAP, "reps": args.reps, "n_corr": rep[:, 1].tolist(), "limit": rep[:, 2].tolist(),
           "returned_iteration": rep[:, 5].tolist(), "n_inliers": rep[:, 6].tolist(), "launches_per_call": 6,
           "a_device_calls_us_median": med(a), "a_device_calls_us_min": float(min(a)), "a_device_calls_us_max": float(max(a)),
           "a300_device_calls_us_median": med(a300), "a300_device_calls_us_min": float(min(a300)),
           "a2_host_form_us_median": med(a2), "a2_host_form_us_min": float(min(a2)),
           "b_host_round_trip_us_median": med(b), "b_host_round_trip_us_min": float(min(b)),
           "b_returned_iteration": [int(x[1]) for x in res],
           "clocks": "a: HIP events on the matcher's stream; a2, b: wall clock of synchronous host work",
           "b_over_a": med(b) / med(a), "a_not_slower_than_b": bool(med(a) <= med(b))}
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
