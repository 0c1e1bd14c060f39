#!/usr/bin/env python3
"""Cost of KeyFrame::UpdateConnections on the device and of the host round trip it replaces, same process, same tables.

  (a) UpdateConnectionsDevice for one new key frame (U = 1) of LocalMapping::ProcessNewKeyFrame: 60 key-frame rows extracted at
      1241x376 @1000, a map of 9000 points, each observed by 2 .. 8 rows of a window of 16 consecutive rows.  The graph of the
      other 59 rows was built (on the device) from the observation lists without the new row; the measured call sees the
      lists with it, so every qualifying row gets a new connection and is re-sorted, as after a real insertion.  Warm,
      HIP-event time on the matcher's stream, median over --reps.
  (b) what a caller had to do without the entry, with the graph kept on the host: D2H of the row's slots and of the
      observation table and point flags (whole: the lists the row touches are scattered over it), the same logic in numpy
      (counter, threshold or maximum, AddConnection with its re-sort per qualifying row, the own row; checked entry for
      entry against the device result before anything is timed), H2D of the covis rows that changed and of the parent.
      Wall clock, median over --reps.
  (c) optionally the log of a headline A/B made the way tools/ab_lib.sh does in headline mode (lines "[label] value ...",
      parent and new interleaved in one call on one box): the numbers are copied into the JSON.  The parent has to run from
      its own tree: its binding declares fewer symbols than this library exports.

  python tools/bench_covis.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR] [--out profiles/covis_stage.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, ROWS, NPTS, WINDOW, NEW_ROW, TH = 1241, 376, 1000, 60, 9000, 16, 30, 15
i32, u8 = np.int32, np.uint8
PRESENT = 1
STATE = ("conn_w", "ord_kf", "ord_w", "n_ord", "covis", "first_conn", "parent")


def ordered(weights):
    """Rows with a weight, descending weight, then descending row."""
    rows = np.nonzero(weights > 0)[0]
    key = (weights[rows].astype(np.int64) << 12) | rows
    rows = rows[np.argsort(-key, kind="stable")]
    return rows.astype(i32), weights[rows].astype(i32)


def host_update_connections(r, slots, start, okf, flags, G, id0_row):
    """UpdateConnections of row r on host arrays G (the keys of STATE), in numpy.  Returns the rows whose covis changed."""
    pts = slots[slots >= 0]
    pts = pts[(flags[pts] & PRESENT) != 0]
    lens = start[pts + 1] - start[pts]
    idx = np.repeat(start[pts], lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
    seen = okf[idx]
    counter = np.bincount(seen[seen != r], minlength=len(G["n_ord"])).astype(i32)
    if not counter.any():
        return []
    qual = np.nonzero(counter >= TH)[0]
    if len(qual) == 0:
        qual = np.array([int(np.argmax(counter))])
    changed = []
    for c in qual:
        w = counter[c]
        if G["conn_w"][c, r] == w:
            continue
        G["conn_w"][c, r] = w
        rows, ws = ordered(G["conn_w"][c])
        k = len(rows)
        G["ord_kf"][c, :k], G["ord_w"][c, :k], G["n_ord"][c] = rows, ws, k
        G["covis"][c] = -1
        G["covis"][c, :min(k, 10)] = rows[:10]
        changed.append(int(c))
    G["conn_w"][r] = counter
    own = np.zeros_like(counter)
    own[qual] = counter[qual]
    rows, ws = ordered(own)
    k = len(rows)
    G["ord_kf"][r, :k], G["ord_w"][r, :k], G["n_ord"][r] = rows, ws, k
    G["covis"][r] = -1
    G["covis"][r, :min(k, 10)] = rows[:10]
    if G["first_conn"][r] and r != id0_row:
        G["parent"][r], G["first_conn"][r] = rows[0], 0
    return changed + [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-log", default="")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import ORBextractor, ORBmatcher
    from orb_slam2_comment_amd.synth import synth_frame
    stream = torch.cuda.Stream()      # explicit: the handle value 0 of torch's default stream means "the handle's own"
    ext = ORBextractor(NF, 1.2, 8, 20, 7)
    ext.set_stream(stream.cuda_stream)
    m = ORBmatcher(0.8, True)
    m.set_stream(stream.cuda_stream)
    cap = ext.capacity(H, W)
    # the key-point counts of the bank come from real extractions (10 distinct frames, repeated)
    uniq = np.stack([synth_frame(1 + i, W, H) for i in range(10)])
    d_img = torch.from_numpy(uniq).cuda()
    d_k = torch.zeros((10, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((10, cap, 32), dtype=torch.uint8, device="cuda")
    d_n10 = torch.zeros(10, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), 10, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n10.data_ptr())
    ext.sync()
    n = np.array([d_n10.cpu().numpy()[r % 10] for r in range(ROWS)], i32)
    rng = np.random.default_rng(1)
    # the map: point p lives around row centre[p] and is observed by 2 .. 8 rows of the window behind it
    centre = rng.integers(0, ROWS, NPTS)
    point_rows = [np.sort((centre[p] + rng.choice(WINDOW, rng.integers(2, 9), replace=False)) % ROWS) for p in range(NPTS)]
    slot_point = np.full((ROWS, cap), -1, i32)
    fill = np.zeros(ROWS, i32)
    keep = []
    for p, rs in enumerate(point_rows):
        rs = [r for r in rs if fill[r] < n[r]]
        for r in rs:
            slot_point[r, fill[r]] = p
            fill[r] += 1
        keep.append(np.array(rs, i32))
    for r in range(ROWS):
        slot_point[r, :n[r]] = rng.permutation(slot_point[r, :n[r]])
    flags = np.where(rng.random(NPTS) < 0.05, 0, PRESENT).astype(u8)

    def csr(lists):
        return (np.concatenate([[0], np.cumsum([len(k) for k in lists])]).astype(i32),
                np.concatenate(lists + [np.zeros(1, i32)]).astype(i32))
    start, okf = csr(keep)
    start0, okf0 = csr([k[k != NEW_ROW] for k in keep])              # before the new key frame was inserted
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tab = dict(slot_point=up(slot_point), n=up(n), obs_start=up(start), obs_kf=up(okf), flags=up(flags))
    tab0 = dict(tab, obs_start=up(start0), obs_kf=up(okf0))
    state = dict(conn_w=torch.zeros((ROWS, ROWS), dtype=torch.int32, device="cuda"),
                 ord_kf=torch.full((ROWS, ROWS), -1, dtype=torch.int32, device="cuda"),
                 ord_w=torch.zeros((ROWS, ROWS), dtype=torch.int32, device="cuda"), n_ord=torch.zeros(ROWS, dtype=torch.int32, device="cuda"),
                 covis=torch.full((ROWS, 10), -1, dtype=torch.int32, device="cuda"),
                 first_conn=torch.ones(ROWS, dtype=torch.uint8, device="cuda"), parent=torch.full((ROWS,), -1, dtype=torch.int32, device="cuda"))
    others = np.array([r for r in range(ROWS) if r != NEW_ROW], i32)
    d_others, d_new = up(others), up(np.array([NEW_ROW], i32))
    d_rep = torch.zeros((ROWS, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.UpdateConnectionsDevice(ROWS, cap, NPTS, NPTS, tab0, state, 0, len(others), d_others.data_ptr(), d_rep.data_ptr())
    m.sync()
    state0 = {k: a.clone() for k, a in state.items()}
    host0 = {k: a.cpu().numpy() for k, a in state0.items()}
    torch.cuda.synchronize()

    def reset():
        for k in STATE:
            state[k].copy_(state0[k])

    def run_device():
        m.UpdateConnectionsDevice(ROWS, cap, NPTS, NPTS, tab, state, 0, 1, d_new.data_ptr(), d_rep.data_ptr())

    # (b): page-locked buffers made once, like a caller's would be; the graph itself lives on the host there
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory()  # noqa: E731
    h_slot, h_start, h_okf, h_flags = pin(slot_point[NEW_ROW]), pin(start), pin(okf), pin(flags)
    h_covis, h_parent = pin(host0["covis"]), pin(host0["parent"])
    d_covis2, d_parent2 = state0["covis"].clone(), state0["parent"].clone()
    G = {}

    def run_host():
        with torch.cuda.stream(stream):
            h_slot.copy_(tab["slot_point"][NEW_ROW], non_blocking=True)
            for h, d in ((h_start, tab["obs_start"]), (h_okf, tab["obs_kf"]), (h_flags, tab["flags"])):
                h.copy_(d, non_blocking=True)
        stream.synchronize()
        changed = host_update_connections(NEW_ROW, h_slot.numpy()[:n[NEW_ROW]], h_start.numpy(), h_okf.numpy(), h_flags.numpy(), G, 0)
        with torch.cuda.stream(stream):
            for c in changed:
                h_covis.numpy()[c] = G["covis"][c]
                d_covis2[c].copy_(h_covis[c], non_blocking=True)
            h_parent.numpy()[NEW_ROW] = G["parent"][NEW_ROW]
            d_parent2[NEW_ROW:NEW_ROW + 1].copy_(h_parent[NEW_ROW:NEW_ROW + 1], non_blocking=True)
        stream.synchronize()
        return changed

    def reset_host():
        G.update({k: a.copy() for k, a in host0.items()})

    reset(); run_device(); m.sync()
    rep = d_rep.cpu().numpy()[0]
    reset_host()
    changed = run_host()
    dev = {k: a.cpu().numpy() for k, a in state.items()}
    assert rep[0] == 0 and rep[6] == len(changed) - 1 and rep[2] == G["n_ord"][NEW_ROW], (rep.tolist(), len(changed))
    for k in ("conn_w", "n_ord", "covis", "first_conn", "parent"):
        assert np.array_equal(dev[k], G[k]), "host route disagrees on " + k
    for r in range(ROWS):
        for k in ("ord_kf", "ord_w"):
            assert np.array_equal(dev[k][r, :dev["n_ord"][r]], G[k][r, :G["n_ord"][r]]), "host route disagrees on %s of row %d" % (k, r)
    assert np.array_equal(d_covis2.cpu().numpy(), dev["covis"]) and np.array_equal(d_parent2.cpu().numpy(), dev["parent"])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        reset(); reset_host(); run_device(); run_host()
    torch.cuda.synchronize()
    td, thost = [], []
    for _ in range(args.reps):          # interleaved, so that drift hits both alike
        reset(); reset_host()
        torch.cuda.synchronize()
        td.append(timed(run_device))
        t0 = time.perf_counter(); run_host(); thost.append((time.perf_counter() - t0) * 1e6)
    a, b = float(np.median(td)), float(np.median(thost))
    doc = {"what": "UpdateConnectionsDevice for one new key frame over %d key-frame rows at %dx%d @%d and a map of %d points vs the "
                   "host round trip it replaces" % (ROWS, W, H, NF, NPTS),
           "status": "measured", "rows": ROWS, "cap": int(cap), "map_points": NPTS, "reps": args.reps, "row_slots": int(n[NEW_ROW]),
           "row_points": int((slot_point[NEW_ROW] >= 0).sum()), "rows_voted": int(rep[1]), "rows_ordered": int(rep[2]),
           "max_weight": int(rep[4]), "rows_resorted": int(rep[6]), "covis_rows_uploaded_by_host_route": len(changed),
           "launches_per_call": "1 memset + 3 kernels (U = 1)",
           "a_device_call_us_median": round(a, 1), "a_device_call_us_min": round(float(np.min(td)), 1),
           "a_device_call_us_max": round(float(np.max(td)), 1),
           "b_host_round_trip_us_median": round(b, 1), "b_host_round_trip_us_min": round(float(np.min(thost)), 1),
           "b_over_a": round(b / a, 1), "a_not_slower_than_b": bool(a <= b)}
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["c_headline"] = {"how": "the procedure of tools/ab_lib.sh in headline mode (bench.py --full --no-cpu-baseline --no-secondary), one "
                                    "call on one box, interleaved parent / new for as many rounds as the log holds; the parent is the parent commit's "
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
