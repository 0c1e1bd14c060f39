#!/usr/bin/env python3
"""Cost of the map-point seeding stage and of the host round trip it replaces, same process, same depths.

  (a) SeedStereoPointsDevice (mode CLOSEST) over 64 left frames of an interleaved 1241x376 stereo batch at 1000 features,
      depths from ComputeStereoMatchesDevice; warm, HIP-event time on the matcher's stream, median over --reps.
  (b) what a caller had to do without the entry: D2H of the depths and the left frames' keypoints into page-locked memory,
      the depth sort / stop rule / unprojection on the host (numpy, vectorised per frame; checked against the device
      result before anything is timed), H2D of world / flags.  Wall clock around the three steps, median over --reps.
  (c) optionally the log of a headline A/B made the way tools/ab_lib.sh does in headline mode (lines "[label] value ...",
      parent and new interleaved in one call on one box, the parent twice): the numbers are copied into the JSON.  The
      parent has to run from its own tree: its binding declares fewer symbols than this library exports and vice versa.

  python tools/bench_seed.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR] [--out profiles/seed_stage.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, PAIRS = 1241, 376, 1000, 64
FX, FY, CX, CY, BF, TH_DEPTH_SETTING = 718.856, 718.856, 607.1928, 185.2157, 386.1448, 35


def host_seed(T, xy, z, th, world, flags):
    """UpdateLastFrame's loop for one frame in numpy float32 (src/Tracking.cc:812-864, src/Frame.cc:666-680)."""
    f32 = np.float32
    idx = np.nonzero(z > 0)[0]
    if len(idx) == 0:
        return 0
    zs = z[idx]
    order = np.lexsort((idx, zs))
    c = int((~(zs > th)).sum())
    sel = idx[order[:min(len(idx), max(101, c + 1))]]
    sel = sel[~((flags[sel] & 1).astype(bool) & (flags[sel] & 2).astype(bool))]
    zz = z[sel]
    x = (xy[sel, 0] - f32(CX)) * zz * (f32(1) / f32(FX))
    y = (xy[sel, 1] - f32(CY)) * zz * (f32(1) / f32(FY))
    for r in range(3):
        ow = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
        world[sel, r] = ((T[0, r] * x + T[1, r] * y) + T[2, r] * zz) + ow
    flags[sel] = 1
    return len(sel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-log", default="")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import ORBextractor, ORBmatcher, KP_DTYPE, capi
    from orb_slam2_comment_amd.matcher import make_camera
    from orb_slam2_comment_amd.synth import synth_stereo
    uniq = [synth_stereo(1 + i, W, H) for i in range(8)]
    frames = np.stack([uniq[p % 8][e] for p in range(PAIRS) for e in (0, 1)])
    B = 2 * PAIRS
    stream = torch.cuda.Stream()      # explicit: the handle value 0 of torch's default stream means "the handle's own"
    ext = ORBextractor(NF, 1.2, 8, 20, 7)
    ext.set_stream(stream.cuda_stream)
    m = ORBmatcher(0.9, True)
    m.set_stream(stream.cuda_stream)
    cap = ext.capacity(H, W)
    cam = make_camera(FX, FY, CX, CY, (0.0, 0.0, float(W), float(H)), ext.GetScaleFactors(), mbf=BF, mb=BF / FX)
    th = np.float32(np.float32(np.float32(BF) * np.float32(TH_DEPTH_SETTING)) / np.float32(FX))
    rng = np.random.default_rng(1)
    T = np.zeros((PAIRS, 3, 4), np.float32)
    T[:, :, :3] = np.eye(3, dtype=np.float32)
    T[:, :, 3] = rng.normal(0, 1, (PAIRS, 3)).astype(np.float32)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_ur = torch.zeros((PAIRS, cap), dtype=torch.float32, device="cuda")
    d_z = torch.zeros((PAIRS, cap), dtype=torch.float32, device="cuda")
    d_nm = torch.zeros(PAIRS, dtype=torch.int32, device="cuda")
    d_T = torch.from_numpy(T.reshape(PAIRS, 12)).cuda()
    d_w = torch.zeros((PAIRS, cap, 3), dtype=torch.float32, device="cuda")
    d_f = torch.zeros((PAIRS, cap), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((PAIRS, 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    mbf, mb = float(np.float32(BF)), float(np.float32(BF) / np.float32(FX))
    m.ComputeStereoMatchesDevice(ext, 0, 2, ext, 1, 2, PAIRS, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), d_k.data_ptr(),
                                 d_d.data_ptr(), d_n.data_ptr(), cap, mbf, mb, d_ur.data_ptr(), d_z.data_ptr(), d_nm.data_ptr())

    def run_device():
        m.SeedStereoPointsDevice(PAIRS, cam, d_T.data_ptr(), d_k.data_ptr(), d_n.data_ptr(), cap, 0, 2, d_z.data_ptr(), th,
                                 capi.SEED_CLOSEST, capi.POINT_PRESENT, d_w.data_ptr(), d_f.data_ptr(), d_cnt.data_ptr())

    run_device()
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()[0::2]
    counts = d_cnt.cpu().numpy()
    # (b): page-locked host buffers, allocated once like a caller's would be
    h_z = torch.zeros((PAIRS, cap), dtype=torch.float32).pin_memory()
    h_k = torch.zeros((PAIRS, cap, 7), dtype=torch.int32).pin_memory()
    h_w = torch.zeros((PAIRS, cap, 3), dtype=torch.float32).pin_memory()
    h_f = torch.zeros((PAIRS, cap), dtype=torch.uint8).pin_memory()
    d_w2, d_f2 = torch.zeros_like(d_w), torch.zeros_like(d_f)
    d_kl = d_k[0::2]                  # the left frames' rows (a strided view: the copy below gathers them)

    def run_host():
        with torch.cuda.stream(stream):
            h_z.copy_(d_z, non_blocking=True)
            h_k.copy_(d_kl, non_blocking=True)
        stream.synchronize()
        z, k = h_z.numpy(), h_k.numpy().view(np.uint8).reshape(PAIRS, cap, 28).view(KP_DTYPE).reshape(PAIRS, cap)
        w, fg = h_w.numpy(), h_f.numpy()
        fg[:] = 0
        made = 0
        for p in range(PAIRS):
            xy = np.stack([k["x"][p, :n[p]], k["y"][p, :n[p]]], 1)
            made += host_seed(T[p], xy, z[p, :n[p]], th, w[p], fg[p])
        with torch.cuda.stream(stream):
            d_w2.copy_(h_w, non_blocking=True)
            d_f2.copy_(h_f, non_blocking=True)
        stream.synchronize()
        return made

    # the host restatement computes what the device computed (flags were zero on the first device run)
    d_f.zero_(); d_w.zero_(); torch.cuda.synchronize()
    run_device(); torch.cuda.synchronize()
    made = run_host()
    assert made == int(counts[:, 2].sum()) == int(d_cnt.cpu().numpy()[:, 2].sum()), "host restatement disagrees on the counts"
    assert np.array_equal(d_f.cpu().numpy(), d_f2.cpu().numpy()), "host restatement disagrees on the flags"
    assert np.array_equal(d_w.cpu().numpy().view(np.int32), d_w2.cpu().numpy().view(np.int32)), "host restatement disagrees on world"

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
    doc = {"what": "SeedStereoPointsDevice (CLOSEST) per %d frames at %dx%d @%d vs the host round trip it replaces" % (PAIRS, W, H, NF),
           "frames": PAIRS, "cap": int(cap), "reps": args.reps, "mean_keypoints": round(float(n.mean()), 1),
           "mean_valid_depths": round(float(counts[:, 0].mean()), 1), "mean_created": round(float(counts[:, 2].mean()), 1),
           "a_device_stage_us_median": round(a, 1), "a_device_stage_us_min": round(float(np.min(td)), 1),
           "a_device_stage_us_max": round(float(np.max(td)), 1),
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
