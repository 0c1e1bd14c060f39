#!/usr/bin/env python3
"""Cost of refreshing map points on the device and of the host round trip it replaces, same process, same table.

  (a) UpdateMapPointsDevice (descriptor + normal / depth) for the workload of LocalMapping::SearchInNeighbors: 30 key-frame
      rows extracted at 1241x376 @1000, 1000 map points with 2 .. 30 observations each (distinct rows, random key points);
      warm, HIP-event time on the matcher's stream, median over --reps.
  (b) what a caller had to do without the entry: gather and D2H of the observed descriptors, octaves and the poses into
      page-locked memory, orbhip_distinctive_descriptors on packed lists plus UpdateNormalAndDepth in numpy (vectorised over
      the points, the sum in table order; checked bit for bit against the device result before anything is timed), the
      winning descriptors copied by hand, H2D of the four arrays.  Wall clock, median over --reps.
  (c) optionally the log of a headline A/B made the way tools/ab_lib.sh does in headline mode (lines "[label] value ...",
      parent and new interleaved in one call on one box, the parent twice): the numbers are copied into the JSON.  The
      parent has to run from its own tree: its binding declares fewer symbols than this library exports.

  python tools/bench_mappoints.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR] [--out profiles/mappoint_stage.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, ROWS, NPTS = 1241, 376, 1000, 30, 1000
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
f32, f64 = np.float32, np.float64


def host_normal_depth(T, world, start, okf, ref_obs, ref_octave, sf):
    """UpdateNormalAndDepth for every point in numpy (src/MapPoint.cc:330-371), the operation order of DESIGN.md section 3:
    observation j of every point at once, j in table order."""
    n = len(start) - 1
    counts = np.diff(start)
    Ow = np.stack([-((T[:, 0, c] * T[:, 0, 3] + T[:, 1, c] * T[:, 1, 3]) + T[:, 2, c] * T[:, 2, 3]) for c in range(3)], 1)
    normal = np.zeros((n, 3), f32)
    pc = np.zeros((n, 3), f32)
    for j in range(int(counts.max())):
        sel = np.nonzero(counts > j)[0]
        d = world[sel] - Ow[okf[start[sel] + j]]
        d64 = d.astype(f64)
        inv = 1.0 / np.sqrt((d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2])
        normal[sel] = normal[sel] + (inv[:, None] * d64).astype(f32)
        is_ref = ref_obs[sel] == j
        pc[sel[is_ref]] = d[is_ref]
    p64 = pc.astype(f64)
    dist = np.sqrt((p64[:, 0] * p64[:, 0] + p64[:, 1] * p64[:, 1]) + p64[:, 2] * p64[:, 2]).astype(f32)
    mx = dist * sf[ref_octave]
    mn = mx / sf[len(sf) - 1]
    return ((1.0 / counts.astype(f64))[:, None] * normal.astype(f64)).astype(f32), mx, mn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-log", default="")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import ORBextractor, ORBmatcher, capi
    from orb_slam2_comment_amd.matcher import make_camera
    from orb_slam2_comment_amd.synth import synth_frame
    uniq = [synth_frame(1 + i, W, H) for i in range(10)]
    frames = np.stack([uniq[r % 10] for r in range(ROWS)])
    stream = torch.cuda.Stream()      # explicit: the handle value 0 of torch's default stream means "the handle's own"
    ext = ORBextractor(NF, 1.2, 8, 20, 7)
    ext.set_stream(stream.cuda_stream)
    m = ORBmatcher(0.9, True)
    m.set_stream(stream.cuda_stream)
    cap = ext.capacity(H, W)
    sf = np.asarray(ext.GetScaleFactors(), f32)
    cam = make_camera(FX, FY, CX, CY, (0.0, 0.0, float(W), float(H)), sf, mbf=BF, mb=BF / FX)
    rng = np.random.default_rng(1)
    T = np.zeros((ROWS, 3, 4), f32)
    for r in range(ROWS):
        a = rng.normal(0, 0.3, 3)
        th = np.linalg.norm(a)
        k = a / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[r, :, :3] = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).astype(f32)
        T[r, :, 3] = rng.normal(0, 2, 3).astype(f32)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.zeros((ROWS, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((ROWS, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), ROWS, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    ext.sync()
    n = d_n.cpu().numpy()
    # the table: 2 .. 30 observations per point, distinct rows, in random order; mpRefKF anywhere in the list
    counts = rng.integers(2, ROWS + 1, NPTS)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    okf = np.concatenate([rng.permutation(ROWS)[:c] for c in counts]).astype(np.int32)
    oidx = (rng.integers(0, 1 << 30, len(okf)) % n[okf]).astype(np.int32)
    ref_obs = (rng.integers(0, 1 << 30, NPTS) % counts).astype(np.int32)
    world = rng.normal(0, 10, (NPTS, 3)).astype(f32)
    flags = np.ones(NPTS, np.uint8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_T, d_start, d_okf, d_oidx, d_ref, d_world, d_flags = (up(a) for a in (T.reshape(ROWS, 12), start, okf, oidx, ref_obs, world, flags))
    d_pd = torch.zeros((NPTS, 32), dtype=torch.uint8, device="cuda")
    d_nrm = torch.zeros((NPTS, 3), dtype=torch.float32, device="cuda")
    d_mx, d_mn = torch.zeros(NPTS, dtype=torch.float32, device="cuda"), torch.zeros(NPTS, dtype=torch.float32, device="cuda")
    d_best = torch.zeros(NPTS, dtype=torch.int32, device="cuda")
    d_status = torch.zeros(NPTS, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def run_device():
        m.UpdateMapPointsDevice(cam, capi.UPDATE_DESCRIPTOR | capi.UPDATE_NORMAL_DEPTH, d_T.data_ptr(), d_k.data_ptr(), d_d.data_ptr(),
                                d_n.data_ptr(), cap, NPTS, NPTS, d_start.data_ptr(), d_okf.data_ptr(), d_oidx.data_ptr(),
                                d_ref.data_ptr(), d_world.data_ptr(), d_flags.data_ptr(), d_pd.data_ptr(), d_nrm.data_ptr(),
                                d_mx.data_ptr(), d_mn.data_ptr(), d_status.data_ptr(), d_best_obs=d_best.data_ptr())

    # (b): the caller's gather index and page-locked buffers, made once like a caller's would be
    nobs = len(okf)
    d_flat = up(okf.astype(np.int64) * cap + oidx)
    ref_flat = up((okf[start[:-1] + ref_obs].astype(np.int64) * cap + oidx[start[:-1] + ref_obs]))
    h_desc = torch.zeros((nobs, 32), dtype=torch.uint8).pin_memory()
    h_oct = torch.zeros(NPTS, dtype=torch.int32).pin_memory()
    h_T = torch.zeros((ROWS, 12), dtype=torch.float32).pin_memory()
    h_pd = torch.zeros((NPTS, 32), dtype=torch.uint8).pin_memory()
    h_nrm = torch.zeros((NPTS, 3), dtype=torch.float32).pin_memory()
    h_mx, h_mn = torch.zeros(NPTS, dtype=torch.float32).pin_memory(), torch.zeros(NPTS, dtype=torch.float32).pin_memory()
    d_pd2, d_nrm2, d_mx2, d_mn2 = (torch.zeros_like(a) for a in (d_pd, d_nrm, d_mx, d_mn))
    d_desc_flat, d_oct_flat = d_d.view(ROWS * cap, 32), d_k.view(ROWS * cap, 7)[:, 5]
    lib, hm = capi.lib(), m._h

    def run_host():
        with torch.cuda.stream(stream):
            h_desc.copy_(d_desc_flat.index_select(0, d_flat), non_blocking=True)
            h_oct.copy_(d_oct_flat.index_select(0, ref_flat), non_blocking=True)
            h_T.copy_(d_T, non_blocking=True)
        stream.synchronize()
        desc = h_desc.numpy()
        best = np.zeros(NPTS, np.int32)
        capi.check(lib.orbhip_distinctive_descriptors(hm, capi.ptr(desc), capi.ptr(start), NPTS, capi.ptr(best)),
                   "orbhip_distinctive_descriptors")
        h_pd.numpy()[:] = desc[start[:-1] + best]
        nrm, mx, mn = host_normal_depth(h_T.numpy().reshape(ROWS, 3, 4), world, start, okf, ref_obs, h_oct.numpy(), sf)
        h_nrm.numpy()[:], h_mx.numpy()[:], h_mn.numpy()[:] = nrm, mx, mn
        with torch.cuda.stream(stream):
            d_pd2.copy_(h_pd, non_blocking=True)
            d_nrm2.copy_(h_nrm, non_blocking=True)
            d_mx2.copy_(h_mx, non_blocking=True)
            d_mn2.copy_(h_mn, non_blocking=True)
        stream.synchronize()
        return best

    run_device()
    stream.synchronize()
    best = run_host()
    assert (d_status.cpu().numpy() == capi.MAPPOINT_UPDATED).all(), "the device call left points out"
    assert np.array_equal(d_best.cpu().numpy(), best), "host route disagrees on the chosen observation"
    for name, x, y in (("descriptor", d_pd, d_pd2), ("normal", d_nrm, d_nrm2), ("max_dist", d_mx, d_mx2), ("min_dist", d_mn, d_mn2)):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), "host route disagrees on " + name

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        run_device(); run_host()
    torch.cuda.synchronize()
    td, thost = [], []
    for _ in range(args.reps):          # interleaved, so that drift hits both alike
        td.append(timed(run_device))
        t0 = time.perf_counter(); run_host(); thost.append((time.perf_counter() - t0) * 1e6)
    a, b = float(np.median(td)), float(np.median(thost))
    doc = {"what": "UpdateMapPointsDevice (descriptor + normal/depth) for %d points over %d key-frame rows at %dx%d @%d vs the host "
                   "round trip it replaces" % (NPTS, ROWS, W, H, NF),
           "status": "measured", "points": NPTS, "rows": ROWS, "cap": int(cap), "reps": args.reps, "observations": int(nobs),
           "points_with_more_than_16_observations": int((counts > 16).sum()), "mean_keypoints": round(float(n.mean()), 1),
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
                                    "call on one box, interleaved parent / new / parent / new; the parent is the parent commit's "
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
