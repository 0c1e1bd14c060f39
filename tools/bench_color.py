#!/usr/bin/env python3
"""Cost of the colour stage: device-resident extract_color_batch_device minus extract_batch_device on the pre-converted
grey frames, same handle, same run, HIP-event time on the handle's stream.

  python tools/bench_color.py [--frames 64] [--reps 30] [--warmup 5] [--out profiles/color_stage.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_color.py --workload-only     (k_cvt_gray beside k_pyr_base)
  rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/bench_color.py --workload-only           (and WRITE_SIZE, a run each)

Per (size, channels) the JSON holds the median / min difference, the algorithmic bytes of the conversion
((channels + 1) * rows * cols per frame) and the rate they give.  The colour frames of a 64-frame batch are 90 - 120 MB
and the grey ones 30 MB: BELOW the 256 MiB Infinity Cache, so a repeated pass can be served from it -- the rate is an
upper bound on what a cold stream from HBM reaches, the same caveat VERDICT.md attaches to the pyramid numbers.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gray_of(img, rgb):
    w = (4899, 9617, 1868) if rgb else (1868, 9617, 4899)
    c = img[..., :3].astype(np.int64)
    return np.minimum((c[..., 0] * w[0] + c[..., 1] * w[1] + c[..., 2] * w[2] + 8192) >> 14, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload-only", action="store_true", help="a few untimed passes, for a profiler wrapped around the run")
    ap.add_argument("--config", default="", help="W,H,channels: only this case (default: 1241x376 and 640x480, 3 and 4 channels)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import ORBextractor
    from orb_slam2_comment_amd.synth import synth_color_frame
    B = args.frames
    results = []
    cases = [(W, H, ch) for W, H in ((1241, 376), (640, 480)) for ch in (3, 4)]
    if args.config:
        cases = [tuple(int(v) for v in args.config.split(","))]
    stream = torch.cuda.Stream()      # explicit: the handle value 0 of torch's default stream means "the handle's own"
    for W, H, ch in cases:
        uniq = [synth_color_frame(1 + i, W, H, channels=ch) for i in range(8)]
        color = np.stack([uniq[i % 8] for i in range(B)])
        pitch = (W + 63) & ~63        # the grey frames in the layout the colour path converts into: same kernels, same strides
        gray = np.zeros((B, H, pitch), np.uint8)
        for i in range(B):
            gray[i, :, :W] = gray_of(uniq[i % 8], True)
        ext = ORBextractor(1000, 1.2, 8, 20, 7)
        ext.set_stream(stream.cuda_stream)
        ext.set_lazy_level0(True)     # monocular / RGB-D configuration: k_pyr_base is then the level-1 launch alone
        cap = ext.capacity(H, W)
        d_c, d_g = torch.from_numpy(color).cuda(), torch.from_numpy(gray).cuda()
        d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
        d_s = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = (d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(), d_s.data_ptr())

        def run_color():
            ext.extract_color_batch_device(d_c.data_ptr(), B, H, W, ch, True, *out)

        def run_gray():
            ext.extract_batch_device(d_g.data_ptr(), B, H, W, *out, stride=pitch, frame_stride=H * pitch)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            return e0.elapsed_time(e1) * 1e3
        run_color(); torch.cuda.synchronize()
        n_color = d_n.cpu().numpy().copy()
        run_gray(); torch.cuda.synchronize()
        assert np.array_equal(n_color, d_n.cpu().numpy()), "colour and grey paths disagree"
        for _ in range(args.warmup):
            run_color(); run_gray()
        torch.cuda.synchronize()
        if args.workload_only:
            continue
        tc, tg = [], []
        for _ in range(args.reps):      # interleaved, so that drift hits both alike
            tc.append(timed(run_color)); tg.append(timed(run_gray))
        diff = np.array(tc) - np.array(tg)
        alg = (ch + 1) * H * W * B
        med = float(np.median(diff))
        results.append({"width": W, "height": H, "channels": ch, "frames": B, "reps": args.reps,
                        "color_us_median": round(float(np.median(tc)), 1), "gray_us_median": round(float(np.median(tg)), 1),
                        "stage_us_median": round(med, 1), "stage_us_min": round(float(diff.min()), 1),
                        "stage_us_max": round(float(diff.max()), 1), "algorithmic_bytes": alg,
                        "algorithmic_TBps_at_median": round(alg / med / 1e6, 3) if med > 0 else None,
                        "working_set_MiB": round((alg + 0.0) / 2 ** 20, 1), "exceeds_infinity_cache_256MiB": alg > 256 * 2 ** 20})
    if args.workload_only:
        return
    doc = {"what": "extract_color_batch_device - extract_batch_device, HIP events, same handle and run", "results": results}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
