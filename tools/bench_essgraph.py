#!/usr/bin/env python3
"""Stage benchmark of the essential-graph optimisation (orbhip_optimize_essential_graph_device) -> profiles/essgraph_stage.json.

One MI355X.  The scene: a ring of 400 key frames with a covisibility band of 20 (weights 288 .. 60, at least 100 up to distance
16), one loop between the last row and row 0, CorrectedSim3 / NonCorrectedSim3 covering the current key frame and its 15
predecessors, 20 000 map points.  Measured warm, median of --reps:
  a   the device call (it synchronises, so HIP events around it and the wall clock agree but for the host's share)
  a2  the host form (one staging copy, the call, one read-back), wall clock
  b   the host route, wall clock: D2H of the tables, the textbook restatement of tests/test_essgraph_cpu.py (numpy, libm, LAPACK
      through numpy.linalg.solve; numpy, NOT g2o), H2D of the poses and points
  the split of a between linearisation, building the system, factorisation, substitution and the rest comes from a kernel trace
  taken in a run of its own (--kernel-stats <csv of rocprofv3 --kernel-trace --stats>, the traced run is `--once`)
  --panel-lib W=PATH  times a again in a child process with a library built with -DORBHIP_EG_PANEL=W (make egpanel8)
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
ROWS, BAND, GROUP, NPTS, MAX_EDGES = 400, 20, 15, 20000, 16384


def scene():
    import test_essgraph_cpu as K
    b = K.ring(ROWS, 7, band=2, group=GROUP, npts=NPTS, drift=(0.0004, -0.0003, 0.0006, 0.001), max_edges=MAX_EDGES)
    T = b["tables"]
    cur = b["cur"]
    conn_w = np.zeros((ROWS, ROWS), i32)
    for a in range(ROWS):
        for c in range(max(0, a - BAND - 2), a):
            d = a - c
            conn_w[a][c] = conn_w[c][a] = 300 - 12 * d if d <= BAND else 30
    for (a, c, w) in ((cur, 0, 60), (cur, 1, 120), (cur - 1, 0, 110), (cur - 1, 1, 70)):
        conn_w[a][c] = conn_w[c][a] = w
    T["conn_w"] = conn_w
    T["ord_kf"], T["ord_w"], T["n_ord"] = K._ordered(conn_w)
    return K, b


def kernel_split(path):
    groups = dict(linearisation=("k_eg_eval", "k_eg_blocks", "k_eg_vertex", "k_eg_lm_begin"), system=("k_eg_zero", "k_eg_scatter"),
                  factorisation=("k_factor_diag", "k_factor_panel", "k_factor_trail"),          # orbhip_ldlt.h, instantiated over EgView
                  substitution=("k_fwd_diag", "k_fwd_upd", "k_dscale", "k_bwd_diag", "k_bwd_upd"),
                  rest=("k_eg_setup", "k_eg_update", "k_eg_trial", "k_eg_judge", "k_eg_finish"))
    per = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        total = row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or row.get("TotalDurationNS")
        calls = row.get("Calls") or row.get("Count")
        for k in sum(groups.values(), ()):
            if k + "E" in name or k + "(" in name or k + "<" in name or k + "I" in name or name.endswith(k):
                per[k] = {"calls": int(calls), "us": float(total) / 1e3}
    out = {g: {"us": sum(per[k]["us"] for k in ks if k in per), "launches": sum(per[k]["calls"] for k in ks if k in per)} for g, ks in groups.items()}
    return {"per_kernel": per, "groups": out, "from": "rocprofv3 --kernel-trace --stats of one call in a run of its own (tracing slows the host; "
                                                     "kernel durations only)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one device call and nothing else: the run a kernel trace is taken of")
    ap.add_argument("--device-only", action="store_true", help="time the device call only and print one JSON line (the --panel-lib child)")
    ap.add_argument("--lib")
    ap.add_argument("--panel-lib", action="append", default=[])
    ap.add_argument("--kernel-stats")
    ap.add_argument("--ab-log")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essgraph_stage.json"))
    args = ap.parse_args()
    K, b = scene()
    t = b["tables"]
    import torch
    from orb_slam2_comment_amd import capi
    if args.lib:
        capi.use_library(os.path.abspath(args.lib))
    import orb_slam2_comment_amd as pkg
    m = pkg.ORBmatcher(0.6, True)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).cuda()  # noqa: E731
    d_t = {k: up(t[k]) for k in K.TABLE_KEYS}
    d_T0, d_w0 = up(t["Tcw"]), up(t["world"])
    o = K.prefilled(b)
    d_o = {k: up(o[k]) for k in o}

    def device_call():
        d_t["Tcw"].copy_(d_T0, non_blocking=True)
        d_t["world"].copy_(d_w0, non_blocking=True)
        m.OptimizeEssentialGraphDevice(b["cur"], b["loop_row"], b["rows"], b["pcap"], d_t, b["fix_scale"], b["max_edges"], d_o)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def timed_wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        device_call()
    m.sync()
    rep = d_o["report"].cpu().numpy().view(i32).tolist()
    syncs, launches = m.EssentialGraphCounters()
    if args.once:
        print(json.dumps({"report": rep, "syncs": syncs, "launches": launches}))
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
    if args.device_only:
        print(json.dumps({"device": dev, "report": rep, "syncs": syncs, "launches": launches}))
        m.close()
        return

    def host_form():
        return m.OptimizeEssentialGraph(t, b["cur"], b["loop_row"], b["fix_scale"], b["max_edges"])

    from seqref import essgraph as E

    def round_trip():
        down = {k: d_t[k].cpu().numpy().view(np.asarray(t[k]).dtype).reshape(np.asarray(t[k]).shape) for k in K.TABLE_KEYS if k not in ("Tcw", "world")}
        down["Tcw"], down["world"] = d_T0.cpu().numpy().view(f32).reshape(-1, 12), d_w0.cpu().numpy().view(f32).reshape(-1, 3)
        vScw = {r: ([float(v) for v in down["corrected"][r]] if down["in_corrected"][r] else E.sim3_from_Tcw(down["Tcw"][r])) for r in range(ROWS)}
        edges, _ = E.build_edges(down, b["cur"], b["loop_row"], vScw)
        ref = {"info": {"edges": edges}, "raw": {"Scw": vScw}}
        est, trace, its = K._textbook(b, ref)
        Tcw = down["Tcw"].copy()
        for r, (R, tt, s) in est.items():
            Tcw[r] = np.c_[R, tt / s].reshape(12).astype(f32)
        world = down["world"].copy()
        for p in range(len(world)):
            if not down["flags"][p] & 1:
                continue
            r = int(down["corrected_ref"][p]) if down["corrected_by_kf"][p] == b["cur"] else int(down["ref_kf"][p])
            if r < 0:
                continue
            R0, t0_, s0 = K._tb_from(vScw[r])
            R1, t1, s1 = K._tb_inv(est[r])
            world[p] = (s1 * (R1 @ (s0 * (R0 @ world[p].astype(f64)) + t0_)) + t1).astype(f32)
        up(Tcw); up(world)
        torch.cuda.synchronize()
        return Tcw, world, trace

    host_form()
    a2 = [timed_wall(host_form) for _ in range(args.reps)]
    t0 = time.perf_counter()
    res = round_trip()
    bb = [(time.perf_counter() - t0) * 1e6]
    with torch.cuda.stream(stream):
        device_call()
    m.sync()
    got_T = d_t["Tcw"].cpu().numpy().view(f32).reshape(-1, 12)
    got_w = d_t["world"].cpu().numpy().view(f32).reshape(-1, 3)
    doc = {"what": "Optimizer::OptimizeEssentialGraph, one call: a ring of %d key frames, covisibility band %d, one loop, %d rows in "
                   "CorrectedSim3, %d map points; the timed call includes the device copies that restore Tcw and world" % (ROWS, BAND, GROUP + 1, NPTS),
           "status": "measured", "reps": args.reps, "report": dict(zip(capi.EG_REPORT, rep)),
           "panel_poses": 4, "synchronisations": syncs, "launches": launches,
           "a_device": dev, "a2_host_form_us_median": med(a2), "a2_host_form_us_min": float(min(a2)),
           "b_host_route_us": bb[0], "b_reps": 1,
           "b_is": "D2H of the tables + the textbook restatement (numpy, libm, numpy.linalg.solve; per-edge numeric Jacobians in Python) + H2D "
                   "of the poses and points; numpy, NOT g2o: the reference's C++ is not measured, so b_over_a is no claim against it",
           "b_decisions": [list(x) for x in res[2]],
           "b_max_pose_distance_from_a": float(np.abs(got_T - res[0]).max()), "b_max_point_distance_from_a_m": float(np.abs(got_w - res[1]).max()),
           "clocks": "a: HIP events on the matcher's stream around the synchronising call, and the wall clock; a2, b: wall clock",
           "b_over_a": bb[0] / med(a)}
    widths = {}
    for spec in args.panel_lib:
        w, path = spec.split("=", 1)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-only", "--lib", path, "--reps", str(args.reps), "--warmup",
                            str(args.warmup)], capture_output=True, text=True, timeout=600)
        widths[w] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"failed": r.stderr[-400:]}
    if widths:
        doc["panel_widths"] = {"4": dev, **{w: v.get("device", v) for w, v in widths.items()},
                               "not_measured": "any width but these; 16 poses do not fit the 64 KB of static LDS of the trailing update"}
    if args.kernel_stats:
        doc["kernel_split"] = kernel_split(args.kernel_stats)
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["c_headline"] = {"how": "bench.py --gpus 1, one call on one box, interleaved parent / new for as many rounds as the log holds; the "
                                    "parent is the parent commit's whole tree with its own library; the headline does not run this path",
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
