#!/usr/bin/env python3
"""Cost of LocalMapping::KeyFrameCulling and MapPointCulling on the device and of the host round trip they replace, same
process, same tables.

  (a) CullKeyFramesDevice for the covisibles of the current key frame and CullMapPointsDevice for the recent points: 60
      key-frame rows extracted at 1241x376 @1000, a map of 9000 points, each observed by 2 .. 8 rows of a window of 16
      consecutive rows.  Every seventh row sees its points two octaves coarser than the others do and only points that five
      rows and more observe, so the rows of that kind among the candidates are redundant and get culled, one after the other,
      each against what the one before left.  Warm, HIP-event time on the matcher's stream, median over --reps.
  (b) what a caller has to do without the entries: D2H of what the loops read (slot tables, the observation table, the point
      flags, the covisibility state), the loops in numpy (the candidates in order, each with its SetBadFlag; the observation
      table built again; checked array for array against the device result before anything is timed), H2D of what they
      changed.  Wall clock, median over --reps.
  (c) optionally the log of a headline A/B made the way tools/ab_lib.sh does in headline mode (lines "[label] value ...",
      parent and new interleaved in one call on one box): the numbers are copied into the JSON.

  python tools/bench_cull.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR] [--out profiles/cull_stage.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, ROWS, NPTS, WINDOW, CUR_ROW, NN = 1241, 376, 1000, 60, 9000, 16, 30, 20
i32, u8 = np.int32, np.uint8
PRESENT, OBSERVED = 1, 2
STATE = ("conn_w", "ord_kf", "ord_w", "n_ord", "covis", "first_conn", "parent")
IO = ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child")


def ordered(weights):
    """Rows with a weight, descending weight, then descending row."""
    rows = np.nonzero(weights > 0)[0]
    key = (weights[rows].astype(np.int64) << 12) | rows
    rows = rows[np.argsort(-key, kind="stable")]
    return rows.astype(i32), weights[rows].astype(i32)


def resort(G, c):
    rows, ws = ordered(G["conn_w"][c])
    k = len(rows)
    G["ord_kf"][c, :k], G["ord_w"][c, :k], G["n_ord"][c] = rows, ws, k
    G["covis"][c] = -1
    G["covis"][c, :min(k, 10)] = rows[:10]


class HostMap:
    """The tables on the host, with the alive marks and counts a host loop would keep per observation."""

    def __init__(self, A, octave):
        self.A, self.octave = A, octave
        self.start, self.okf, self.oidx = A["obs_start"], A["obs_kf"], A["obs_idx"]
        self.point_of = np.repeat(np.arange(len(self.start) - 1), np.diff(self.start))
        present = (A["flags"][self.point_of] & PRESENT) != 0
        self.alive = present.copy()
        self.nobs = np.bincount(self.point_of[present], minlength=len(self.start) - 1).astype(i32)     # monocular: 1 each
        in_list = (A["ref_obs"] >= 0) & (A["ref_obs"] < np.diff(self.start)) & ((A["flags"][:len(self.start) - 1] & PRESENT) != 0)
        self.ref = np.where(in_list, A["ref_obs"], -1).astype(i32)

    def set_bad(self, p):
        A = self.A
        A["flags"][p] &= ~np.uint8(PRESENT)
        o = np.arange(self.start[p], self.start[p + 1])
        o = o[self.alive[o]]
        self.alive[o] = False
        A["slot_point"][self.okf[o], self.oidx[o]] = -1

    def table(self):
        keep = self.alive[:int(self.start[-1])]
        cnt = np.bincount(self.point_of[keep], minlength=len(self.start) - 1)
        start = np.concatenate([[0], np.cumsum(cnt)]).astype(i32)
        rank = np.cumsum(keep) - 1                                 # new position of every alive entry
        ref = np.full(len(cnt), -1, i32)
        has = self.ref >= 0
        o = self.start[:-1][has] + self.ref[has]
        ref[has] = np.where(keep[o], rank[o] - start[:-1][has], -1)
        return start, self.okf[:len(keep)][keep], self.oidx[:len(keep)][keep], ref


def host_cull_key_frames(M, G, n, cand, id0_row):
    """KeyFrameCulling over cand on host arrays, monocular.  Returns the rows culled."""
    A, rows = M.A, len(n)
    culled = []
    for r in cand:
        if r < 0 or r == id0_row:
            continue
        slots = A["slot_point"][r, :n[r]]
        idx = np.nonzero(slots >= 0)[0]
        pts = slots[idx]
        ok = (A["flags"][pts] & PRESENT) != 0
        idx, pts = idx[ok], pts[ok]
        n_mps = len(pts)
        many = M.nobs[pts] > 3
        lens = (M.start[pts + 1] - M.start[pts])[many]
        o = np.repeat(M.start[pts[many]], lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
        level = np.repeat(M.octave[r, idx[many]], lens)
        hit = M.alive[o] & (M.okf[o] != r) & (M.octave[M.okf[o], M.oidx[o]] <= level + 1)
        per = np.bincount(np.repeat(np.arange(len(lens)), lens)[hit], minlength=len(lens))
        n_red = int((per >= 3).sum())
        if not 10 * n_red > 9 * n_mps:
            continue
        culled.append(r)
        for c in np.nonzero(G["conn_w"][r])[0]:                     # EraseConnection
            if G["conn_w"][c, r]:
                G["conn_w"][c, r] = 0
                resort(G, c)
        allp = np.unique(slots[slots >= 0])                         # EraseObservation
        lens = M.start[allp + 1] - M.start[allp]
        o = np.repeat(M.start[allp], lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
        mine = o[(M.okf[o] == r) & M.alive[o]]
        M.alive[mine] = False
        pp = M.point_of[mine]
        M.nobs[pp] -= 1
        A["flags"][pp] = (A["flags"][pp] & ~np.uint8(OBSERVED)) | np.where(M.nobs[pp] > 0, OBSERVED, 0).astype(u8)
        for p, e in zip(pp, mine):
            if M.ref[p] == e - M.start[p]:
                left = np.nonzero(M.alive[M.start[p]:M.start[p + 1]])[0]
                M.ref[p] = left[0] if len(left) else -1
        for p in pp[M.nobs[pp] <= 2]:
            M.set_bad(p)
        G["conn_w"][r] = 0
        G["n_ord"][r] = 0
        G["covis"][r] = -1
        parent = int(G["parent"][r])                                # the spanning tree
        cands = {parent} if parent >= 0 else set()
        children = [int(c) for c in np.nonzero((G["parent"] == r) & (A["kf_bad"] == 0))[0]]
        while children:
            best = (-1, None, None)
            for c in children:
                for k in G["ord_kf"][c, :G["n_ord"][c]]:
                    if int(k) in cands and G["conn_w"][c, k] > best[0]:
                        best = (int(G["conn_w"][c, k]), c, int(k))
            if best[1] is None:
                break
            G["parent"][best[1]] = best[2]
            cands.add(best[1])
            children.remove(best[1])
        for c in children:
            G["parent"][c] = parent
        A["kf_bad"][r] = 1
    return culled


def host_cull_map_points(M, recent, found, visible, first_kf_id, cur_kf_id, th_obs):
    """MapPointCulling on host arrays; a point comes once in `recent`.  Returns (kept, status)."""
    A = M.A
    age = cur_kf_id - first_kf_id[recent]
    bad = (A["flags"][recent] & PRESENT) == 0
    ratio = ~bad & (4 * found[recent].astype(np.int64) < visible[recent])
    few = ~bad & ~ratio & (age >= 2) & (M.nobs[recent] <= th_obs)
    old = ~bad & ~ratio & ~few & (age >= 3)
    status = np.select([bad, ratio, few, old], [1, 2, 3, 4], 0).astype(u8)
    for p in recent[ratio | few]:
        M.set_bad(p)
    return recent[status == 0], status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-log", default="")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import KP_DTYPE, ORBextractor, ORBmatcher
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
    coarse = np.arange(ROWS) % 7 == 3
    centre = rng.integers(0, ROWS, NPTS)
    slot_point = np.full((ROWS, cap), -1, i32)
    fill = np.zeros(ROWS, i32)
    lists = []
    for p in range(NPTS):
        rs = np.sort((centre[p] + rng.choice(WINDOW, rng.integers(2, 9), replace=False)) % ROWS)
        rs = [int(r) for r in rs if fill[r] < n[r] and not (coarse[r] and len(rs) < 5)]
        entry = []
        for r in rs:
            slot_point[r, fill[r]] = p
            entry.append((r, int(fill[r])))
            fill[r] += 1
        lists.append(entry)
    flags = (np.where(rng.random(NPTS) < 0.05, 0, PRESENT) | OBSERVED).astype(u8)
    start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(i32)
    okf = np.array([k for x in lists for k, _ in x], i32)
    oidx = np.array([i for x in lists for _, i in x], i32)
    total = len(okf)
    ref = np.array([int(rng.integers(0, len(x))) if x else -1 for x in lists], i32)
    octave = np.where(coarse[:, None], 4, rng.integers(0, 3, (ROWS, cap))).astype(i32)
    kps = np.zeros((ROWS, cap), KP_DTYPE)
    kps["octave"] = octave
    found = rng.integers(0, 40, NPTS).astype(i32)
    visible = (found * rng.choice([1, 2, 5], NPTS, p=[0.6, 0.3, 0.1])).astype(i32)
    first_kf_id = rng.integers(96, 101, NPTS).astype(i32)
    recent = rng.choice(NPTS, 600, replace=False).astype(i32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(a.shape + (a.dtype.itemsize,)) if a.dtype.fields  # noqa: E731
                                    else np.ascontiguousarray(a)).cuda()
    tab = dict(kps=up(kps), n=up(n), obs_start=up(start), obs_kf=up(okf), obs_idx=up(oidx), ref_obs=up(ref))
    io = dict(slot_point=up(slot_point), flags=up(flags), kf_bad=up(np.zeros(ROWS, u8)), to_be_erased=up(np.zeros(ROWS, u8)),
              child_start=up(np.zeros(ROWS + 1, i32)), child=up(np.zeros(ROWS, i32)), obs_start_out=up(np.zeros(NPTS + 1, i32)),
              obs_kf_out=up(np.zeros(total, i32)), obs_idx_out=up(np.zeros(total, i32)), ref_obs_out=up(np.zeros(NPTS, i32)))
    state = dict(conn_w=torch.zeros((ROWS, ROWS), dtype=torch.int32, device="cuda"),
                 ord_kf=torch.full((ROWS, ROWS), -1, dtype=torch.int32, device="cuda"),
                 ord_w=torch.zeros((ROWS, ROWS), dtype=torch.int32, device="cuda"), n_ord=torch.zeros(ROWS, dtype=torch.int32, device="cuda"),
                 covis=torch.full((ROWS, 10), -1, dtype=torch.int32, device="cuda"),
                 first_conn=torch.ones(ROWS, dtype=torch.uint8, device="cuda"), parent=torch.full((ROWS,), -1, dtype=torch.int32, device="cuda"))
    # the graph, on the device: UpdateConnections of every row in order, then the children
    d_all = up(np.arange(ROWS, dtype=i32))
    d_rep = torch.zeros((ROWS, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctab = dict(slot_point=io["slot_point"], n=tab["n"], obs_start=tab["obs_start"], obs_kf=tab["obs_kf"], flags=io["flags"])
    m.UpdateConnectionsDevice(ROWS, cap, NPTS, NPTS, ctab, state, 0, ROWS, d_all.data_ptr(), d_rep.data_ptr())
    m.ChildrenFromParentsDevice(ROWS, state["parent"].data_ptr(), io["kf_bad"].data_ptr(), io["child_start"].data_ptr(),
                                io["child"].data_ptr())
    d_cur, d_cand, d_cnt = up(np.array([CUR_ROW], i32)), torch.zeros(NN, dtype=torch.int32, device="cuda"), up(np.zeros(1, i32))
    m.CovisibleTargetsDevice(ROWS, state["ord_kf"].data_ptr(), state["n_ord"].data_ptr(), 0, 1, d_cur.data_ptr(), NN, 0,
                             d_cand.data_ptr(), d_cnt.data_ptr())
    m.sync()
    cand = d_cand.cpu().numpy()
    keep0 = {k: a.clone() for d in (io, state) for k, a in d.items()}
    host0 = {k: a.cpu().numpy() for k, a in keep0.items()}
    d_kfrep = torch.zeros((NN, 8), dtype=torch.int32, device="cuda")
    d_recent, d_found, d_visible, d_first = up(recent), up(found), up(visible), up(first_kf_id)
    d_rout, d_nout, d_status = torch.zeros(len(recent), dtype=torch.int32, device="cuda"), up(np.zeros(1, i32)), up(np.zeros(len(recent), u8))
    # the table out of the first call is the table in of the second
    tab2 = dict(tab, obs_start=io["obs_start_out"], obs_kf=io["obs_kf_out"], obs_idx=io["obs_idx_out"], ref_obs=io["ref_obs_out"])
    io2 = dict(io, obs_start_out=up(np.zeros(NPTS + 1, i32)), obs_kf_out=up(np.zeros(total, i32)), obs_idx_out=up(np.zeros(total, i32)),
               ref_obs_out=up(np.zeros(NPTS, i32)))
    torch.cuda.synchronize()

    def reset():
        for d in (io, state):
            for k, a in d.items():
                a.copy_(keep0[k])

    def run_kf():
        m.CullKeyFramesDevice(ROWS, cap, NPTS, NPTS, total, tab, io, state, 0, NN, d_cand.data_ptr(), True, 0.0, d_kfrep.data_ptr())

    def run_mp():
        m.CullMapPointsDevice(ROWS, cap, NPTS, NPTS, total, tab2, io2, len(recent), d_recent.data_ptr(), d_found.data_ptr(),
                              d_visible.data_ptr(), d_first.data_ptr(), 100, 2, d_rout.data_ptr(), d_nout.data_ptr(), d_status.data_ptr())

    # (b): page-locked buffers made once, like a caller's would be
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory()  # noqa: E731
    down = dict(slot_point=io["slot_point"], flags=io["flags"], kf_bad=io["kf_bad"], obs_start=tab["obs_start"], obs_kf=tab["obs_kf"],
                obs_idx=tab["obs_idx"], ref_obs=tab["ref_obs"], conn_w=state["conn_w"], ord_kf=state["ord_kf"], ord_w=state["ord_w"],
                n_ord=state["n_ord"], covis=state["covis"], parent=state["parent"])
    h = {k: pin(a.cpu().numpy()) for k, a in down.items()}
    up_keys = ("slot_point", "flags", "kf_bad", "conn_w", "ord_kf", "ord_w", "n_ord", "covis", "parent")
    d_back = {k: down[k].clone() for k in up_keys}
    d_tab_back = [torch.zeros_like(tab["obs_start"]), torch.zeros_like(tab["obs_kf"]), torch.zeros_like(tab["obs_idx"]),
                  torch.zeros_like(tab["ref_obs"])]
    h_tab = [pin(np.zeros(NPTS + 1, i32)), pin(np.zeros(total, i32)), pin(np.zeros(total, i32)), pin(np.zeros(NPTS, i32))]
    res = {}

    def run_host():
        with torch.cuda.stream(stream):
            for k, a in down.items():
                h[k].copy_(a, non_blocking=True)
        stream.synchronize()
        A = {k: h[k].numpy() for k in ("slot_point", "flags", "kf_bad", "obs_start", "obs_kf", "obs_idx", "ref_obs")}
        G = {k: h[k].numpy() for k in ("conn_w", "ord_kf", "ord_w", "n_ord", "covis", "parent")}
        M = HostMap(A, octave)
        res["culled"] = host_cull_key_frames(M, G, n, cand, 0)
        res["kept"], res["status"] = host_cull_map_points(M, recent, found, visible, first_kf_id, 100, 2)
        t = M.table()
        for hb, a in zip(h_tab, t):
            hb.numpy()[:len(a)] = a
        res["table"], res["A"], res["G"] = t, A, G
        with torch.cuda.stream(stream):
            for k in up_keys:
                d_back[k].copy_(h[k], non_blocking=True)
            for db, hb in zip(d_tab_back, h_tab):
                db.copy_(hb, non_blocking=True)
        stream.synchronize()

    reset(); run_kf(); run_mp(); m.sync()
    rep = d_kfrep.cpu().numpy()
    dev = {k: a.cpu().numpy() for d in (io2, state) for k, a in d.items()}
    dev_status, dev_kept = d_status.cpu().numpy(), d_rout.cpu().numpy()[:int(d_nout.cpu().numpy()[0])]
    reset()
    torch.cuda.synchronize()
    run_host()
    assert sorted(res["culled"]) == sorted(int(cand[u]) for u in range(NN) if rep[u, 0] == 1), (res["culled"], rep[:, 0].tolist())
    assert len(res["culled"]) >= 2, "the scene is meant to cull a few candidates"
    for k in ("slot_point", "flags", "kf_bad"):
        assert np.array_equal(dev[k], res["A"][k]), "host route disagrees on " + k
    for k in ("conn_w", "n_ord", "covis", "parent"):
        assert np.array_equal(dev[k], res["G"][k]), "host route disagrees on " + k
    n_left = int(dev["obs_start_out"][-1])
    assert np.array_equal(dev["obs_start_out"], res["table"][0]) and np.array_equal(dev["obs_kf_out"][:n_left], res["table"][1])
    assert np.array_equal(dev["obs_idx_out"][:n_left], res["table"][2]) and np.array_equal(dev["ref_obs_out"], res["table"][3])
    assert np.array_equal(dev_status, res["status"]) and np.array_equal(dev_kept, res["kept"])
    for k in ("slot_point", "flags", "kf_bad", "conn_w", "n_ord", "covis", "parent"):      # ... and so is what it sent back
        assert np.array_equal(d_back[k].cpu().numpy(), dev[k]), k

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        reset(); run_kf(); run_mp(); m.sync(); reset(); run_host()
    torch.cuda.synchronize()
    tk, tm, thost = [], [], []
    for _ in range(args.reps):          # interleaved, so that drift hits both alike
        reset()
        torch.cuda.synchronize()
        tk.append(timed(run_kf))
        tm.append(timed(run_mp))
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); run_host(); thost.append((time.perf_counter() - t0) * 1e6)
    a1, a2, b = float(np.median(tk)), float(np.median(tm)), float(np.median(thost))
    doc = {"what": "CullKeyFramesDevice over the %d best covisibles of one key frame and CullMapPointsDevice over %d recent points, "
                   "%d key-frame rows at %dx%d @%d and a map of %d points, vs the host round trip they replace"
                   % (NN, len(recent), ROWS, W, H, NF, NPTS),
           "status": "measured", "rows": ROWS, "cap": int(cap), "map_points": NPTS, "observations": total, "reps": args.reps,
           "candidates": int((cand >= 0).sum()), "culled": len(res["culled"]), "observations_left": n_left,
           "points_turned_bad_by_key_frames": int(rep[:, 4].sum()), "recent": len(recent), "recent_kept": len(res["kept"]),
           "launches_per_call": "key frames 2 U + 6 (U = %d), map points 7" % NN,
           "a_key_frames_us_median": round(a1, 1), "a_key_frames_us_min": round(float(np.min(tk)), 1),
           "a_key_frames_us_max": round(float(np.max(tk)), 1), "a_map_points_us_median": round(a2, 1),
           "a_map_points_us_min": round(float(np.min(tm)), 1), "a_map_points_us_max": round(float(np.max(tm)), 1),
           "b_host_round_trip_us_median": round(b, 1), "b_host_round_trip_us_min": round(float(np.min(thost)), 1),
           "b_over_a": round(b / (a1 + a2), 1), "a_not_slower_than_b": bool(a1 + a2 <= b)}
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        lo, hi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["c_headline"] = {"how": "the procedure of tools/ab_lib.sh in headline mode, one call on one box, interleaved parent / new for as "
                                    "many rounds as the log holds; the parent is the parent commit's whole tree with its own library",
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
