#!/usr/bin/env python3
"""Development tool: where k_octree spends its time, and the register path against the workspace path.

One 64-frame pipeline of the benchmark's frames (16 distinct images), through the -DORBHIP_DEVTOOLS build
(tools/_dev/liborbhip_dev.so, orbhip_dev_set_octree_variant / orbhip_dev_octree_stamps; the product library has neither):

  * the candidates K per (level, frame) of the distinct frames, i.e. which (level, frame)s fit the register capacity;
  * HIP-event time of the octree stage, keys in registers against every workgroup forced through the workspace path
    (the parent's code), interleaved rounds in ONE process, outputs compared;
  * the s_memtime split of a level-0 workgroup for both paths (stamped build: shares, not lengths, are meaningful).

  python tools/octree_ab.py [--rounds 8] [--frames 64] [--calls 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = ["cell_offsets", "gather", "initial_table", "first_sweep_or_label_shift", "count", "careful_order", "table_wavefront",
          "relabel_or_fused_sweep", "best_key"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", default="1241x376")
    ap.add_argument("--nfeatures", type=int, default=1000)
    args = ap.parse_args()
    from fast_ab import use_dev_build
    use_dev_build()
    import torch
    from orb_slam2_comment_amd import ORBextractor
    from orb_slam2_comment_amd.capi import lib
    from orb_slam2_comment_amd.synth import synth_frame
    W, H = (int(v) for v in args.size.split("x"))
    dev = torch.device("cuda", 0)
    B = args.frames
    uniq = np.stack([synth_frame(1 + (i // 2) % 8, W, H, shift_xy=(3 * (i % 2), 0)) for i in range(min(B, 16))])
    frames = np.stack([uniq[i % len(uniq)] for i in range(B)])
    d_img = torch.from_numpy(frames).to(dev)
    ext = ORBextractor(args.nfeatures, 1.2, 8, 20, 7, device=0)
    ext.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    cap = ext.capacity(H, W)
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    d_s = torch.zeros(B, dtype=torch.int32, device=dev)
    L = lib()

    def run():
        ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(), d_s.data_ptr())

    variants = {"registers": 0, "workspace": 1}
    sig = {}
    for name, v in variants.items():
        L.orbhip_dev_set_octree_variant(ext._h, v)
        run()
        torch.cuda.synchronize()
        sig[name] = (d_n.cpu().numpy().copy(), d_d.cpu().numpy().copy(), d_k.cpu().numpy().copy())
    n = sig["registers"][0]
    same = np.array_equal(n, sig["workspace"][0]) and all(
        np.array_equal(sig["registers"][i][b, :n[b]], sig["workspace"][i][b, :n[b]]) for b in range(B) for i in (1, 2))
    kdist = [[len(ext.level_candidates(l, frame=f)[0]) for l in range(8)] for f in range(len(uniq))]
    res = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, v in variants.items():
            L.orbhip_dev_set_octree_variant(ext._h, v)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            ext.set_profiling(True)
            for _ in range(args.calls):
                run()
            torch.cuda.synchronize()
            res[name].append(ext.stage_times_us()["octree"])
            ext.set_profiling(False)
    stamps = {}
    z = (C.c_ulonglong * 16)()
    for name, v in variants.items():
        L.orbhip_dev_set_octree_variant(ext._h, v | 2)
        run()
        torch.cuda.synchronize()
        L.orbhip_dev_octree_stamps(z)          # clear what the first call of the stamped kernel left
        run()
        torch.cuda.synchronize()
        L.orbhip_dev_octree_stamps(z)
        wgs = max(1, z[10])
        tot = float(sum(z[i] for i in range(9)))
        stamps[name] = {"ticks_per_workgroup": {PHASES[i]: round(z[i] / wgs, 1) for i in range(9)},
                        "shares": {PHASES[i]: round(z[i] / tot, 3) for i in range(9)},
                        "passes_per_workgroup": round(z[9] / wgs, 2), "keys_per_workgroup": round(z[11] / wgs, 1),
                        "level0_workgroups": int(z[10])}
    L.orbhip_dev_set_octree_variant(ext._h, 0)
    k = np.array(kdist)
    print(json.dumps({
        "frames": B, "size": args.size, "outputs_identical": bool(same),
        "octree_stage_us": {name: {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2)} for name, v in res.items()},
        "stamps_level0": stamps,
        "candidates_per_level": {"max": k.max(0).tolist(), "median": np.median(k, 0).tolist(), "min": k.min(0).tolist()}}))


if __name__ == "__main__":
    main()
