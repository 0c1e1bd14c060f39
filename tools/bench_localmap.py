#!/usr/bin/env python3
"""Cost of building the local map on the device and of the host round trip it replaces, same process, same tables.

  (a) UpdateLocalMapDevice for one current frame of Tracking::TrackLocalMap: 60 key-frame rows extracted at 1241x376 @1000,
      about 40 of them voted for by the frame's points, the rest reached (or not) through covisibles, children and parents; a
      map of 9000 points, each observed by 2 .. 8 rows of a window of 16 consecutive rows, so that the local map has several
      thousand points.  Warm, HIP-event time on the matcher's stream, median over --reps.
  (b) what a caller had to do without the entry: D2H of the frame's point assignment, the observation lists, key-frame flags
      and graph tables it touches and the slot tables of the bank; votes, the key-frame list and the local point list on the
      host (the walk as a loop, the rest in numpy; checked entry for entry against the device result before anything is
      timed); the gather of the five per-point arrays and the flags; H2D of the six arrays.  Wall clock, median over --reps.
  (c) optionally the log of a headline A/B made the way tools/ab_lib.sh does in headline mode (lines "[label] value ...",
      parent and new interleaved in one call on one box, the parent at least twice): the numbers are copied into the JSON.  The
      parent has to run from its own tree: its binding declares fewer symbols than this library exports.

  python tools/bench_localmap.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR] [--out profiles/localmap_stage.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, ROWS, NPTS, VOTED, WINDOW = 1241, 376, 1000, 60, 9000, 40, 16
f32, i32, u8 = np.float32, np.int32, np.uint8
PRESENT, OBSERVED = 1, 2


def host_local_map(fp, nf, start, okf, flags, kf_bad, covis, child_start, child, parent, slot_point, n, rows):
    """UpdateLocalKeyFrames + UpdateLocalPoints + the search bookkeeping on the host: numpy where the work is data parallel,
    a loop for the walk.  Returns (frame_point, list, local points, flags_l, taken)."""
    fp = fp[:nf].copy()
    held = fp >= 0
    bad = held & ((flags[np.maximum(fp, 0)] & PRESENT) == 0)
    fp[bad] = -1
    pts = fp[fp >= 0]
    lens = start[pts + 1] - start[pts]
    idx = np.repeat(start[pts], lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
    votes = np.bincount(okf[idx], minlength=rows)
    first = np.nonzero((votes > 0) & (kf_bad == 0))[0]
    out = first.tolist()
    stamped = np.zeros(rows, bool)
    stamped[first] = True
    for v in range(len(first)):
        if len(out) > 80:
            break
        r = out[v]
        for c in covis[r]:
            if c >= 0 and not kf_bad[c] and not stamped[c]:
                out.append(int(c)); stamped[c] = True
                break
        for c in child[child_start[r]:child_start[r + 1]]:
            if not kf_bad[c] and not stamped[c]:
                out.append(int(c)); stamped[c] = True
                break
        pr = parent[r]
        if pr >= 0 and not stamped[pr]:
            out.append(int(pr)); stamped[pr] = True
            break
    cand = np.concatenate([slot_point[r, :n[r]] for r in out]) if out else np.zeros(0, i32)
    cand = cand[cand >= 0]
    cand = cand[(flags[cand] & PRESENT) != 0]
    _, where = np.unique(cand, return_index=True)
    local = cand[np.sort(where)]
    is_held = np.zeros(len(flags), bool)
    is_held[pts] = True
    fl = np.where(is_held[local], 0, PRESENT | (flags[local] & OBSERVED)).astype(u8)
    taken = ((fp >= 0) & ((flags[np.maximum(fp, 0)] & OBSERVED) != 0)).astype(u8)
    return fp, np.array(out, i32), local.astype(i32), fl, taken


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
    start = np.concatenate([[0], np.cumsum([len(k) for k in keep])]).astype(i32)
    okf = np.concatenate(keep + [np.zeros(1, i32)]).astype(i32)
    flags = np.where(rng.random(NPTS) < 0.05, OBSERVED, PRESENT | OBSERVED).astype(u8)
    kf_bad = np.zeros(ROWS, u8)
    kf_bad[[7, 33]] = 1
    covis = np.stack([rng.permutation(np.delete(np.arange(ROWS), r))[:10] for r in range(ROWS)]).astype(i32)
    parent = np.array([-1] + [max(0, r - 1 - int(rng.integers(0, 3))) for r in range(1, ROWS)], i32)
    ch = [[] for _ in range(ROWS)]
    for r in range(1, ROWS):
        ch[parent[r]].append(r)
    child_start = np.concatenate([[0], np.cumsum([len(c) for c in ch])]).astype(i32)
    child = np.array([x for c in ch for x in c] + [0], i32)
    world, normal = rng.normal(0, 10, (NPTS, 3)).astype(f32), rng.normal(0, 1, (NPTS, 3)).astype(f32)
    max_dist, min_dist = rng.uniform(5, 50, NPTS).astype(f32), rng.uniform(1, 5, NPTS).astype(f32)
    point_desc = rng.integers(0, 256, (NPTS, 32), dtype=u8)
    # the current frame holds points of the rows 10 .. 10 + VOTED - WINDOW: with the window behind them about VOTED rows vote
    nf = int(n[0])
    near = np.nonzero((centre >= 10) & (centre < 10 + VOTED - WINDOW))[0]
    frame_point = np.full((1, cap), -1, i32)
    frame_point[0, :nf] = np.where(rng.random(nf) < 0.4, rng.choice(near, nf), -1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    host_tab = dict(slot_point=slot_point, n=n, kf_bad=kf_bad, covis=covis, child_start=child_start, child=child, parent=parent,
                    obs_start=start, obs_kf=okf, flags=flags, world=world, normal=normal, max_dist=max_dist, min_dist=min_dist,
                    point_desc=point_desc)
    tab = {k: up(a) for k, a in host_tab.items()}
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    io = dict(frame_point=up(frame_point), frame_n=up(np.array([nf], i32)), local_kf=z((1, ROWS), torch.int32),
              n_local_kf=z(1, torch.int32), votes=z((1, ROWS), torch.int32), local_point=z((1, NPTS), torch.int32),
              world_l=z((1, NPTS, 3), torch.float32), normal_l=z((1, NPTS, 3), torch.float32), max_dist_l=z((1, NPTS), torch.float32),
              min_dist_l=z((1, NPTS), torch.float32), desc_l=z((1, NPTS, 32), torch.uint8), flags_l=z((1, NPTS), torch.uint8),
              np_l=z(1, torch.int32), taken=z((1, cap), torch.uint8), report=z((1, 8), torch.int32))
    d_fp0 = up(frame_point)
    torch.cuda.synchronize()

    def run_device():
        m.UpdateLocalMapDevice(1, ROWS, cap, NPTS, NPTS, tab, io)

    # (b): page-locked buffers made once, like a caller's would be
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory()  # noqa: E731
    h_fp, h_slot, h_n, h_start, h_okf, h_flags, h_bad = (pin(a) for a in (frame_point, slot_point, n, start, okf, flags, kf_bad))
    h_covis, h_cs, h_child, h_parent = (pin(a) for a in (covis, child_start, child, parent))
    h_out = [torch.zeros(s, dtype=dt).pin_memory() for s, dt in (((NPTS, 3), torch.float32), ((NPTS, 3), torch.float32),
             ((NPTS,), torch.float32), ((NPTS,), torch.float32), ((NPTS, 32), torch.uint8), ((NPTS,), torch.uint8))]
    d_out2 = [torch.zeros_like(io[k][0]) for k in ("world_l", "normal_l", "max_dist_l", "min_dist_l", "desc_l", "flags_l")]

    def run_host():
        with torch.cuda.stream(stream):
            for h, d in ((h_fp, d_fp0), (h_slot, tab["slot_point"]), (h_n, tab["n"]), (h_start, tab["obs_start"]), (h_okf, tab["obs_kf"]),
                         (h_flags, tab["flags"]), (h_bad, tab["kf_bad"]), (h_covis, tab["covis"]), (h_cs, tab["child_start"]),
                         (h_child, tab["child"]), (h_parent, tab["parent"])):
                h.copy_(d, non_blocking=True)
        stream.synchronize()
        fp, kfs, local, fl, taken = host_local_map(h_fp.numpy()[0], nf, h_start.numpy(), h_okf.numpy(), h_flags.numpy(), h_bad.numpy(),
                                                   h_covis.numpy(), h_cs.numpy(), h_child.numpy(), h_parent.numpy(), h_slot.numpy(),
                                                   h_n.numpy(), ROWS)
        k = len(local)
        for h, src in zip(h_out, (world, normal, max_dist, min_dist, point_desc)):
            h.numpy()[:k] = src[local]
        h_out[5].numpy()[:k] = fl
        with torch.cuda.stream(stream):
            for d, h in zip(d_out2, h_out):
                d[:k].copy_(h[:k], non_blocking=True)
        stream.synchronize()
        return fp, kfs, local, fl, taken

    def reset():
        io["frame_point"].copy_(d_fp0)

    run_device()
    stream.synchronize()
    rep = io["report"].cpu().numpy()[0]
    fp, kfs, local, fl, taken = run_host()
    k = len(local)
    assert rep[0] == 0 and rep[2] == len(kfs) and rep[6] == k, (rep.tolist(), len(kfs), k)
    assert np.array_equal(io["local_kf"].cpu().numpy()[0, :len(kfs)], kfs), "host route disagrees on the key-frame list"
    assert np.array_equal(io["local_point"].cpu().numpy()[0, :k], local), "host route disagrees on the local points"
    assert np.array_equal(io["frame_point"].cpu().numpy()[0, :nf], fp) and np.array_equal(io["taken"].cpu().numpy()[0, :nf], taken)
    for name, d2 in zip(("world_l", "normal_l", "max_dist_l", "min_dist_l", "desc_l", "flags_l"), d_out2):
        assert np.array_equal(io[name].cpu().numpy()[0, :k].view(u8), d2.cpu().numpy()[:k].view(u8)), "host route disagrees on " + name

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        reset(); run_device(); run_host()
    torch.cuda.synchronize()
    td, thost = [], []
    for _ in range(args.reps):          # interleaved, so that drift hits both alike
        reset()
        torch.cuda.synchronize()
        td.append(timed(run_device))
        t0 = time.perf_counter(); run_host(); thost.append((time.perf_counter() - t0) * 1e6)
    a, b = float(np.median(td)), float(np.median(thost))
    doc = {"what": "UpdateLocalMapDevice for one frame over %d key-frame rows at %dx%d @%d and a map of %d points vs the host round "
                   "trip it replaces" % (ROWS, W, H, NF, NPTS),
           "status": "measured", "rows": ROWS, "cap": int(cap), "map_points": NPTS, "reps": args.reps, "frame_keypoints": nf,
           "frame_points_held": int((fp >= 0).sum()), "rows_voted": int(rep[1]), "local_keyframes": int(rep[2]),
           "walk_end": int(rep[5]), "local_points": int(rep[6]), "mean_keypoints": round(float(n.mean()), 1),
           "launches_per_call": "2 memsets + 6 kernels",
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
