#!/usr/bin/env python3
"""Cost of the rectification stage: device-resident extract_remap_batch_device minus extract_batch_device on the
pre-rectified frames, same handle, same run, interleaved repetitions, HIP-event time on the handle's stream.  The maps are
the EuRoC LEFT maps of tests/golden/EuRoC_stereo.yaml, the frames 752x480.

  python tools/bench_rectify.py [--frames 64,192,400] [--reps 30] [--warmup 5] [--out profiles/rectify_stage.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_rectify.py --workload-only --frames 192   (k_remap beside k_pyr_base)
  rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/bench_rectify.py --workload-only --frames 192         (and WRITE_SIZE, a run each)

Per frame count the JSON holds the median / min difference, the algorithmic bytes of the remap (source + rectified pixels
per frame, + the 8-byte records once per XCD) and the rate they give.  192 frames x (source + rectified) = 132 MiB is
still BELOW the 256 MiB Infinity Cache, so a repeated pass can be served from it; 400 frames (275 MiB) are not.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 752, 480


def rectified_of(img, m1, m2):
    """The bilinear fixed-point remap on the host (numpy), to make the pre-rectified frames of the grey pass."""
    sx, sy = np.rint(m1.astype(np.float64) * 32).astype(np.int64), np.rint(m2.astype(np.float64) * 32).astype(np.int64)
    x0, y0, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31
    acc = np.full(x0.shape, 1 << 14, np.int64)
    wide = img.astype(np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            x, y = x0 + dx, y0 + dy
            ok = (x >= 0) & (x < img.shape[1]) & (y >= 0) & (y < img.shape[0])
            acc += np.where(ok, wide[np.clip(y, 0, img.shape[0] - 1), np.clip(x, 0, img.shape[1] - 1)], 0) * (wy * wx * 32)
    return np.minimum(acc >> 15, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,192,400")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload-only", action="store_true", help="a few untimed passes, for a profiler wrapped around the run")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import ORBextractor, init_undistort_rectify_map
    from orb_slam2_comment_amd.settings import stereo_rectification
    from orb_slam2_comment_amd.synth import synth_frame
    c = stereo_rectification(os.path.join(ROOT, "tests", "golden", "EuRoC_stereo.yaml"))["left"]
    m1, m2 = init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], (W, H))
    uniq = [synth_frame(1 + i, W, H) for i in range(8)]
    rect = [rectified_of(u, m1, m2) for u in uniq]
    pitch = (W + 63) & ~63            # the rectified frames in the layout the remap writes: same kernels, same strides
    results = []
    stream = torch.cuda.Stream()      # explicit: the handle value 0 of torch's default stream means "the handle's own"
    for B in (int(v) for v in args.frames.split(",")):
        raw = np.stack([uniq[i % 8] for i in range(B)])
        gray = np.zeros((B, H, pitch), np.uint8)
        for i in range(B):
            gray[i, :, :W] = rect[i % 8]
        ext = ORBextractor(1000, 1.2, 8, 20, 7)
        ext.set_stream(stream.cuda_stream)
        ext.set_lazy_level0(True)     # k_pyr_base is then the level-1 launch alone, the yardstick of the trace
        ext.set_remap(m1, m2)
        cap = ext.capacity(H, W)
        d_r, d_g = torch.from_numpy(raw).cuda(), torch.from_numpy(gray).cuda()
        d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
        d_s = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = (d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(), d_s.data_ptr())

        def run_remap():
            ext.extract_remap_batch_device(d_r.data_ptr(), B, H, W, *out)

        def run_gray():
            ext.extract_batch_device(d_g.data_ptr(), B, H, W, *out, stride=pitch, frame_stride=H * pitch)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            return e0.elapsed_time(e1) * 1e3
        run_remap(); torch.cuda.synchronize()
        n_remap = d_n.cpu().numpy().copy()
        run_gray(); torch.cuda.synchronize()
        assert np.array_equal(n_remap, d_n.cpu().numpy()), "remap and grey paths disagree"
        for _ in range(args.warmup):
            run_remap(); run_gray()
        torch.cuda.synchronize()
        if args.workload_only:
            continue
        tr, tg = [], []
        for _ in range(args.reps):      # interleaved, so that drift hits both alike
            tr.append(timed(run_remap)); tg.append(timed(run_gray))
        diff = np.array(tr) - np.array(tg)
        alg = 2 * H * W * B + 8 * H * W * min(B, 8)
        med = float(np.median(diff))
        results.append({"width": W, "height": H, "frames": B, "reps": args.reps,
                        "remap_us_median": round(float(np.median(tr)), 1), "gray_us_median": round(float(np.median(tg)), 1),
                        "stage_us_median": round(med, 1), "stage_us_min": round(float(diff.min()), 1),
                        "stage_us_max": round(float(diff.max()), 1), "algorithmic_bytes": alg,
                        "algorithmic_TBps_at_median": round(alg / med / 1e6, 3) if med > 0 else None,
                        "working_set_MiB": round(2 * H * W * B / 2 ** 20, 1),
                        "exceeds_infinity_cache_256MiB": 2 * H * W * B > 256 * 2 ** 20})
        del ext, d_r, d_g
    if args.workload_only:
        return
    doc = {"what": "extract_remap_batch_device - extract_batch_device, HIP events, same handle and run", "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
