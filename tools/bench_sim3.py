#!/usr/bin/env python3
"""Cost of the Sim3 RANSAC of LoopClosing::ComputeSim3 on the device and of the host round trip it replaces, same process,
same tables.

  (a) Sim3SetupDevice + Sim3IterateDevice(max_its = 300) for C = 5 loop candidates of about 100 correspondences each (70
      under one Sim3 of scale 1.7, 30 random), a current key frame of 1000 slots in a bank of cap 1024, matched12 as the
      slots orbhip_search_by_bow_device writes.  Warm, HIP-event time on the matcher's stream, median over --reps.
  (a2) Sim3Ransac, the host form of the same (one staged copy, the two calls, one read-back).  Wall clock.
  (b) what a caller had to do without the entries: D2H of matched12, the two slot tables, the observation table, flags and
      positions; the algorithm of tests/seqref/sim3.py in vectorised numpy (all hypotheses of a candidate at once, fp64,
      numpy.linalg.eigh), checked against the device result (same returned iteration, same inlier set) before anything is
      timed; H2D of the Sim3 and the inlier marks.  Wall clock, median over --reps.
  (c) optionally the log of a headline A/B (lines "[label] value ...", parent and new interleaved in one call on one box);
      the numbers are copied into the JSON.  The parent runs from its own tree: its binding declares fewer symbols.

  python tools/bench_sim3.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR] [--out profiles/sim3_stage.json]
  python tools/bench_sim3.py --host-only     # no GPU: builds the scene and runs route (b)'s arithmetic once
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C_, NCORR, NGOOD, N1, CAP, ROWS, MIN_INL, MAX_ITS, PROB = 5, 100, 70, 1000, 1024, 6, 20, 300, 0.99
FX, FY, CX, CY = 718.856, 718.856, 607.19, 185.22
i32, u8, f32, f64 = np.int32, np.uint8, np.float32, np.float64
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], f32)


def rot(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_scene(seed=1):
    """Bank row 0 is the current key frame, rows 1 .. 5 the candidates; every key frame point is observed by its own row
    (and by one other row first, so that the observation lists are searched)."""
    rng = np.random.default_rng(seed)
    s12, R12, t12 = 1.7, rot([0.3, 1.0, 0.2], 0.4), np.array([0.5, -0.2, 0.3])
    Tcw = np.zeros((ROWS, 3, 4))
    for r in range(ROWS):
        Tcw[r, :, :3], Tcw[r, :, 3] = rot(rng.uniform(-1, 1, 3), rng.uniform(0, 0.5)), rng.uniform(-2, 2, 3)
    z = rng.uniform(4.0, 40.0, N1)
    X1 = np.stack([rng.uniform(-0.6, 0.6, N1) * z, rng.uniform(-0.2, 0.2, N1) * z, z], 1)
    inv = lambda T, X: (X - T[:, 3]) @ T[:, :3]          # noqa: E731  (R^T (X - t), row vectors)
    world, obs = [inv(Tcw[0], X1)], [[(1 + i % 5, 0), (0, i)] for i in range(N1)]
    slot_point = np.full((ROWS, CAP), -1, i32)
    slot_point[0, :N1] = np.arange(N1)
    matched = np.full((C_, CAP), -1, i32)
    n_pts = N1
    for c in range(C_):
        kf = c + 1
        i1 = np.sort(rng.choice(N1, NCORR, replace=False))
        X2 = (X1[i1] - t12) @ R12 / s12                  # R12^T (X1 - t12) / s12
        bad = rng.permutation(NCORR)[NGOOD:]
        zz = rng.uniform(4.0, 40.0, len(bad))
        X2[bad] = np.stack([rng.uniform(-0.6, 0.6, len(bad)) * zz, rng.uniform(-0.2, 0.2, len(bad)) * zz, zz], 1)
        slots = rng.permutation(CAP)[:NCORR]
        world.append(inv(Tcw[kf], X2))
        for k in range(NCORR):
            obs.append([(0, 5), (kf, int(slots[k]))])
            slot_point[kf, slots[k]] = n_pts + k
            matched[c, i1[k]] = slots[k]
        n_pts += NCORR
    flat = [e for o in obs for e in o]
    from orb_slam2_comment_amd import capi
    kps = np.zeros((ROWS, CAP), capi.KP_DTYPE)
    kps["octave"] = rng.integers(0, 8, (ROWS, CAP))
    n = np.full(ROWS, CAP, i32)
    n[0] = N1
    start = np.zeros(n_pts + 1, i32)
    start[1:] = np.cumsum([len(o) for o in obs])
    return dict(slot_point=slot_point, n=n, obs_start=start, obs_kf=np.array([e[0] for e in flat], i32),
                obs_idx=np.array([e[1] for e in flat], i32), flags=np.ones(n_pts, u8), world=np.concatenate(world).astype(f32),
                Tcw=Tcw.reshape(ROWS, 12).astype(f32), kps=kps), np.arange(1, ROWS, dtype=i32), matched


def limit_of(N):
    if N < MIN_INL:
        return 0
    if N == MIN_INL:
        return 1
    eps = float(f32(f32(MIN_INL) / f32(N)))
    return int(max(1, min(np.ceil(np.log(1 - PROB) / np.log(1 - eps ** 3)), MAX_ITS)))


def first_index(T, pts, row):
    """GetIndexInKeyFrame of every point of pts for one row: the first entry of the list that names the row, or -1."""
    s, e = T["obs_start"][pts], T["obs_start"][pts + 1]
    lens = e - s
    owner = np.repeat(np.arange(len(pts)), lens)
    pos = np.repeat(s, lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
    hit = T["obs_kf"][pos] == row
    out = np.full(len(pts), -1, i32)
    # the first hit of each owner: walk the hits backwards so that the earliest assignment wins
    out[owner[hit][::-1]] = T["obs_idx"][pos[hit]][::-1]
    return out


def host_sim3(T, cur, kf, matched, draws, fix_scale=False):
    """Sim3Solver for one candidate in numpy, all hypotheses at once, fp64.  Returns (returned iteration or -1, sim3 [16],
    inliers [n1] uint8)."""
    n1 = int(T["n"][cur])
    i1 = np.nonzero(matched[:n1] >= 0)[0]
    p2 = T["slot_point"][kf][matched[i1]]
    p1 = T["slot_point"][cur][i1]
    ok = (p1 >= 0) & (p2 >= 0)
    i1, p1, p2 = i1[ok], p1[ok], p2[ok]
    ok = ((T["flags"][p1] & 1) != 0) & ((T["flags"][p2] & 1) != 0)
    i1, p1, p2 = i1[ok], p1[ok], p2[ok]
    idx1, idx2 = first_index(T, p1, cur), first_index(T, p2, kf)
    ok = (idx1 >= 0) & (idx2 >= 0)
    i1, p1, p2, idx1, idx2 = i1[ok], p1[ok], p2[ok], idx1[ok], idx2[ok]
    N = len(i1)
    inl_out, sim3 = np.zeros(n1, u8), np.zeros(16, f32)
    L = limit_of(N)
    if L == 0:
        return -1, sim3, inl_out
    max1 = np.floor(9.210 * SIGMA2[T["kps"]["octave"][cur][idx1]].astype(f64))
    max2 = np.floor(9.210 * SIGMA2[T["kps"]["octave"][kf][idx2]].astype(f64))
    T1, T2 = T["Tcw"][cur].reshape(3, 4).astype(f64), T["Tcw"][kf].reshape(3, 4).astype(f64)
    X1 = T["world"][p1].astype(f64) @ T1[:, :3].T + T1[:, 3]
    X2 = T["world"][p2].astype(f64) @ T2[:, :3].T + T2[:, 3]
    K = np.array([FX, FY]), np.array([CX, CY])
    im1, im2 = X1[:, :2] / X1[:, 2:] * K[0] + K[1], X2[:, :2] / X2[:, 2:] * K[0] + K[1]
    # the draw replay, vectorised over the iterations (three different positions: see include/orbhip.h)
    d = draws[:L].astype(np.int64)
    r0, r1, r2 = d[:, 0], d[:, 1], d[:, 2]
    back1 = np.where(r0 == N - 2, N - 1, N - 2)
    idx = np.stack([r0, np.where(r1 == r0, N - 1, r1), np.where(r2 == r1, back1, np.where(r2 == r0, N - 1, r2))], 1)
    P1, P2 = X1[idx], X2[idx]                                       # [L, 3 points, 3]
    O1, O2 = P1.mean(1), P2.mean(1)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.einsum("lkr,lkc->lrc", Pr2, Pr1)
    Nm = np.zeros((L, 4, 4))
    Nm[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    Nm[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]
    Nm[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]
    Nm[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]
    Nm[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    Nm[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]
    Nm[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]
    Nm[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    Nm[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    Nm[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    Nm = Nm + np.transpose(np.triu(Nm, 1), (0, 2, 1))
    _, V = np.linalg.eigh(Nm)
    q = V[:, :, 3]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(L, 3, 3)
    P3 = np.einsum("lrc,lkc->lkr", R, Pr2)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.ones(L) if fix_scale else (Pr1 * P3).sum((1, 2)) / (P3 * P3).sum((1, 2))
        t = O1 - s[:, None] * np.einsum("lrc,lc->lr", R, O2)
        sR, sRinv = s[:, None, None] * R, np.transpose(R, (0, 2, 1)) / s[:, None, None]
        tinv = -np.einsum("lrc,lc->lr", sRinv, t)
        A = np.einsum("lrc,nc->lnr", sR, X2) + t[:, None]           # set 2 in camera 1
        B = np.einsum("lrc,nc->lnr", sRinv, X1) + tinv[:, None]     # set 1 in camera 2
        e1 = ((A[:, :, :2] / A[:, :, 2:] * K[0] + K[1] - im1) ** 2).sum(2)
        e2 = ((B[:, :, :2] / B[:, :, 2:] * K[0] + K[1] - im2) ** 2).sum(2)
        inl = (e1 < max1) & (e2 < max2)
    cnt = inl.sum(1)
    before = np.maximum.accumulate(np.concatenate([[0], cnt[:-1]]))
    hit = np.nonzero((cnt >= before) & (cnt > MIN_INL))[0]
    if len(hit) == 0:
        return -1, sim3, inl_out
    h = int(hit[0])
    sim3[:9], sim3[9:12], sim3[12] = R[h].reshape(9), t[h], s[h]
    inl_out[i1[inl[h]]] = 1
    return h, sim3, inl_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-log", default="")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from orb_slam2_comment_amd import sim3_draws
    T, kf_index, matched = make_scene()
    draws = sim3_draws(C_, MAX_ITS, [NCORR] * C_, 2)
    if args.host_only:
        for c in range(C_):
            h, sim3, inl = host_sim3(T, 0, int(kf_index[c]), matched[c], draws[c])
            print("candidate %d: returned iteration %d, %d inliers, s = %.6f" % (c, h, int(inl.sum()), sim3[12]))
        return
    import torch
    from orb_slam2_comment_amd import ORBmatcher, capi
    from orb_slam2_comment_amd.matcher import make_camera
    stream = torch.cuda.Stream()
    m = ORBmatcher(0.75, True)
    m.set_stream(stream.cuda_stream)
    cam = make_camera(FX, FY, CX, CY, (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)])
    n_pts = len(T["flags"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731
    dT = {k: up(v) for k, v in T.items()}
    d_kf, d_m12, d_draws = up(kf_index), up(matched), up(draws)
    sizes = dict(x1=12, x2=12, p1=8, p2=8, max_err1=4, max_err2=4, slot1=4)
    dS = {k: torch.zeros(C_ * CAP * b, dtype=torch.uint8, device="cuda") for k, b in sizes.items()}
    dS.update({k: torch.zeros(C_ * 8, dtype=torch.uint8, device="cuda") for k in ("n_corr", "n1", "limit", "state")})
    d_sim3 = torch.zeros(C_ * 16, dtype=torch.float32, device="cuda")
    d_inl = torch.zeros(C_ * CAP, dtype=torch.uint8, device="cuda")
    d_rep = torch.zeros(C_ * 8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def run_device():
        m.Sim3SetupDevice(C_, 0, d_kf, cam, ROWS, CAP, n_pts, n_pts, dT, d_m12, capi.SIM3_MATCH_SLOTS, SIGMA2, dS, PROB, MIN_INL,
                          MAX_ITS)
        m.Sim3IterateDevice(C_, CAP, cam, dS, d_draws, MAX_ITS, MAX_ITS, MIN_INL, False, d_sim3, d_inl, d_rep)

    def run_host_form():
        return m.Sim3Ransac(T, 0, kf_index, cam, matched, capi.SIM3_MATCH_SLOTS, SIGMA2, draws, False, PROB, MIN_INL, MAX_ITS)

    # (b): page-locked buffers made once, like a caller's would be
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).pin_memory()  # noqa: E731
    down = ("slot_point", "obs_start", "obs_kf", "obs_idx", "flags", "world")
    h_tab = {k: pin(T[k]) for k in down}
    h_m12 = pin(matched)
    h_sim3, h_inl = torch.zeros(C_ * 16, dtype=torch.float32).pin_memory(), torch.zeros(C_ * CAP, dtype=torch.uint8).pin_memory()
    d_sim3b, d_inlb = torch.zeros_like(d_sim3), torch.zeros_like(d_inl)

    def run_host():
        with torch.cuda.stream(stream):
            for k in down:
                h_tab[k].copy_(dT[k], non_blocking=True)
            h_m12.copy_(d_m12, non_blocking=True)
        stream.synchronize()
        Th = dict(T)                                        # poses, key points and counts are host data of the caller anyway
        for k in down:
            Th[k] = h_tab[k].numpy().view(T[k].dtype).reshape(T[k].shape)
        mt = h_m12.numpy().view(i32).reshape(C_, CAP)
        out = []
        for c in range(C_):
            h, sim3, inl = host_sim3(Th, 0, int(kf_index[c]), mt[c], draws[c])
            h_sim3.numpy()[16 * c:16 * c + 16] = sim3
            h_inl.numpy()[CAP * c:CAP * c + len(inl)] = inl
            out.append(h)
        with torch.cuda.stream(stream):
            d_sim3b.copy_(h_sim3, non_blocking=True)
            d_inlb.copy_(h_inl, non_blocking=True)
        stream.synchronize()
        return out

    run_device(); m.sync()
    rep = d_rep.cpu().numpy().reshape(C_, 8)
    dev_sim3, dev_inl = d_sim3.cpu().numpy().reshape(C_, 16), d_inl.cpu().numpy().reshape(C_, CAP)
    got = run_host()
    assert (rep[:, 0] == capi.SIM3_RETURNED).all(), rep.tolist()
    assert got == rep[:, 5].tolist(), (got, rep[:, 5].tolist())
    assert np.array_equal(d_inlb.cpu().numpy().reshape(C_, CAP)[:, :N1], dev_inl[:, :N1]), "host route disagrees on the inliers"
    assert np.abs(d_sim3b.cpu().numpy().reshape(C_, 16) - dev_sim3).max() < 1e-3
    hf = run_host_form()
    assert np.array_equal(hf["report"], rep) and hf["sim3"].tobytes() == dev_sim3.tobytes()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        run_device(); run_host(); run_host_form()
    torch.cuda.synchronize()
    td, thost, tform = [], [], []
    for _ in range(args.reps):          # interleaved, so that drift hits all alike
        torch.cuda.synchronize()
        td.append(timed(run_device))
        t0 = time.perf_counter(); run_host(); thost.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter(); run_host_form(); tform.append((time.perf_counter() - t0) * 1e6)
    a, b, a2 = float(np.median(td)), float(np.median(thost)), float(np.median(tform))
    doc = {"what": "Sim3SetupDevice + Sim3IterateDevice(%d) for %d loop candidates of %d correspondences (%d under one Sim3) vs the "
                   "host round trip they replace" % (MAX_ITS, C_, NCORR, NGOOD),
           "status": "measured", "candidates": C_, "cap": CAP, "current_slots": N1, "map_points": int(n_pts), "reps": args.reps,
           "n_corr": rep[:, 1].tolist(), "limit": rep[:, 2].tolist(), "returned_iteration": rep[:, 5].tolist(),
           "n_inliers": rep[:, 6].tolist(), "launches_per_call": "setup 1 kernel, iterate 3 kernels",
           "a_device_calls_us_median": round(a, 1), "a_device_calls_us_min": round(float(np.min(td)), 1),
           "a_device_calls_us_max": round(float(np.max(td)), 1),
           "a2_host_form_us_median": round(a2, 1), "a2_host_form_us_min": round(float(np.min(tform)), 1),
           "b_host_round_trip_us_median": round(b, 1), "b_host_round_trip_us_min": round(float(np.min(thost)), 1),
           "b_over_a": round(b / a, 1), "a_not_slower_than_b": bool(a <= b)}
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["c_headline"] = {"how": "bench.py --full --no-cpu-baseline --no-secondary as tools/ab_lib.sh runs it in headline mode, one call on "
                                    "one box, interleaved parent / new for as many rounds as the log holds; the parent is the parent commit's "
                                    "whole tree with its own library, because its binding declares fewer symbols",
                             "parent_runs": runs["parent"], "new_runs": runs["new"], "parent_spread": [lo, hi],
                             "new_within_parent_spread": [bool(lo <= v <= hi) for v in runs["new"]] if runs["parent"] else None,
                             "new_below_parent_min": [bool(v < lo) for v in runs["new"]] if runs["parent"] else None}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
