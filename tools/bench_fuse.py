#!/usr/bin/env python3
"""Cost of fusing one key frame's map points into its K neighbours (LocalMapping::SearchInNeighbors), same process, same data.

  K = 30 targets of about 1000 key points at 1241x376 (one scene under 30 small shifts, extracted in one batch), the map
  points of the first key frame (one per key point) plus as many again that project into no target, th = 3.

  (a) FuseDevice with the grids precomputed by AssignFeaturesToGridDevice: one launch.  HIP-event time on the matcher's
      stream, warm, median over --reps.
  (b) FuseDevice building the grids inside the call: two launches.  Same clock.
  (c) the only route without the entry: K x orbhip_fuse on host buffers (each call stages the points and the key frame,
      reads the queries back, stages them again and reads the result back).  Wall clock, median over --reps.
  (d) FuseBatch, the host entry: one staged copy, (b), one read-back.  Wall clock.
  (e) with --mappings (development build, orbhip_dev_fuse_lanes): (a) with one wavefront per query against the 8 lanes per
      query the library ships.

  All results are compared with (c) before anything is timed.
  python tools/bench_fuse.py [--reps 30] [--warmup 5] [--mappings] [--out profiles/fuse_stage.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, K = 1241, 376, 1000, 30
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mappings", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from orb_slam2_comment_amd import capi
    if args.mappings:
        dev_lib = os.path.join(ROOT, "tools", "_dev", "liborbhip_dev.so")
        if not os.path.exists(dev_lib):
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), "dev"], check=True)
        capi.use_library(dev_lib)
    import torch
    from orb_slam2_comment_amd import FrameView, KP_DTYPE, ORBextractor, ORBmatcher
    from orb_slam2_comment_amd.matcher import make_camera
    from orb_slam2_comment_amd.synth import synth_frame
    rng = np.random.default_rng(3)
    frames = np.stack([synth_frame(5, W, H, shift_xy=(k % 6, k // 6)) for k in range(K)])
    stream = torch.cuda.Stream()
    ext = ORBextractor(NF, 1.2, 8, 20, 7)
    ext.set_stream(stream.cuda_stream)
    m = ORBmatcher(0.6, True)
    m.set_stream(stream.cuda_stream)
    cap = ext.capacity(H, W)
    sf = ext.GetScaleFactors()
    bounds = (0.0, 0.0, float(W), float(H))
    cam = make_camera(FX, FY, CX, CY, bounds, sf, mbf=BF, mb=BF / FX)
    inv_sigma2 = (1.0 / (sf * sf)).astype(np.float32)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.zeros((K, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((K, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(K, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), K, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    ext.sync()
    n = d_n.cpu().numpy()
    hk = d_k.cpu().numpy().view(np.uint8).reshape(K, cap, 28).view(KP_DTYPE).reshape(K, cap)
    hd = d_d.cpu().numpy()
    # poses: target k looks at the scene shifted by (k % 6, k // 6) px, i.e. the camera moved sideways at depth 20
    T = np.zeros((K, 3, 4), np.float32)
    T[:, :, :3] = np.eye(3, dtype=np.float32)
    T[:, 0, 3] = [(k % 6) * 20.0 / FX for k in range(K)]
    T[:, 1, 3] = [(k // 6) * 20.0 / FY for k in range(K)]
    k0 = hk[0, :n[0]]
    n0 = len(k0)
    z = np.full(n0, 20.0, np.float32)
    X = np.stack([(k0["x"] - np.float32(CX)) * z / np.float32(FX), (k0["y"] - np.float32(CY)) * z / np.float32(FY), z], 1).astype(np.float32)
    dist = np.linalg.norm(X, axis=1)
    nrm = (X / dist[:, None]).astype(np.float32)
    max_d = (dist * np.float32(1.2) ** (k0["octave"].astype(np.float32) - np.float32(0.3))).astype(np.float32)
    nowhere = X.copy()
    nowhere[: n0 // 2, 2] = -nowhere[: n0 // 2, 2]                    # behind every camera
    nowhere[n0 // 2:, 0] += np.float32(200.0)                         # far outside every image
    X = np.ascontiguousarray(np.concatenate([X, nowhere]))
    nrm = np.ascontiguousarray(np.concatenate([nrm, nrm]))
    max_d = np.ascontiguousarray(np.concatenate([max_d, max_d]))
    min_d = (max_d / np.float32(1.2 ** 7)).astype(np.float32)
    pdesc = np.ascontiguousarray(np.concatenate([hd[0, :n0], hd[0, :n0]]))
    npts = len(X)
    flags = (rng.random((K, npts)) < 0.9).astype(np.uint8)
    d_idx = torch.arange(K, dtype=torch.int32, device="cuda")
    d_T = torch.from_numpy(T.reshape(K, 12)).cuda()
    dX, dNr, dMx, dMn, dP, dF = (torch.from_numpy(a).cuda() for a in (X, nrm, max_d, min_d, pdesc, flags))
    d_bi = torch.zeros((K, npts), dtype=torch.int32, device="cuda")
    d_bd = torch.zeros((K, npts), dtype=torch.int32, device="cuda")
    d_cell = torch.zeros((K, cap), dtype=torch.int32, device="cuda")
    d_items = torch.zeros((K, cap), dtype=torch.int32, device="cuda")
    d_start = torch.zeros((K, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.AssignFeaturesToGridDevice(K, d_k.data_ptr(), d_n.data_ptr(), cap, bounds, d_cell.data_ptr(), d_start.data_ptr(),
                                 d_items.data_ptr())

    def run_device(csr):
        m.FuseDevice(K, d_idx.data_ptr(), cam, d_T.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, npts, npts,
                     dX.data_ptr(), dNr.data_ptr(), dMx.data_ptr(), dMn.data_ptr(), dP.data_ptr(), dF.data_ptr(), 3.0, inv_sigma2,
                     d_bi.data_ptr(), d_bd.data_ptr(), d_cell_start=d_start.data_ptr() if csr else 0,
                     d_cell_items=d_items.data_ptr() if csr else 0)

    # (c): raw C calls on prepared arguments, so that no Python conversion is timed
    L, p = capi.lib(), capi.ptr
    views = [FrameView(hk[k, :n[k]].copy(), hd[k, :n[k]].copy(), sf, bounds) for k in range(K)]
    cviews = [v.c_view() for v in views]
    Tk = [np.ascontiguousarray(T[k]) for k in range(K)]
    h_bi, h_bd = np.zeros((K, npts), np.int32), np.zeros((K, npts), np.int32)

    def run_single():
        for k in range(K):
            capi.check(L.orbhip_fuse(m._h, C.byref(cviews[k]), C.byref(cam), p(Tk[k]), 0, npts, p(X), p(nrm), p(max_d), p(min_d),
                                     p(flags[k]), p(pdesc), 3.0, p(inv_sigma2), p(h_bi[k]), p(h_bd[k])), "orbhip_fuse")

    arr = (C.POINTER(capi.FrameView) * K)(*[C.pointer(v) for v in cviews])
    Tall = np.ascontiguousarray(T.reshape(K, 12))
    b_bi, b_bd = np.zeros((K, npts), np.int32), np.zeros((K, npts), np.int32)

    def run_batch():
        capi.check(L.orbhip_fuse_batch(m._h, K, arr, C.byref(cam), p(Tall), 0, npts, p(X), p(nrm), p(max_d), p(min_d), p(flags),
                                       p(pdesc), 3.0, p(inv_sigma2), p(b_bi), p(b_bd)), "orbhip_fuse_batch")

    run_single()
    run_batch()
    assert np.array_equal(b_bi, h_bi) and np.array_equal(b_bd, h_bd), "FuseBatch disagrees with K x Fuse"
    lanes = [8, 64] if args.mappings else [8]
    for ln in lanes:
        if args.mappings:
            capi.check(L.orbhip_dev_fuse_lanes(ln), "orbhip_dev_fuse_lanes")
        for csr in (True, False):
            d_bi.zero_(); d_bd.zero_(); torch.cuda.synchronize()
            run_device(csr); m.sync()
            assert np.array_equal(d_bi.cpu().numpy(), h_bi) and np.array_equal(d_bd.cpu().numpy(), h_bd), "FuseDevice disagrees"
    fused = int((h_bd <= 50).sum())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    res = {}
    for ln in lanes:
        if args.mappings:
            L.orbhip_dev_fuse_lanes(ln)
        for _ in range(args.warmup):
            run_device(True); run_device(False)
        m.sync()
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(lambda: run_device(True)))
            tb.append(timed(lambda: run_device(False)))
        res[ln] = (ta, tb)
    if args.mappings:
        L.orbhip_dev_fuse_lanes(8)
    for _ in range(args.warmup):
        run_single(); run_batch()
    tc, td = [], []
    for _ in range(args.reps):          # interleaved, so that drift hits both alike
        tc.append(wall(run_single))
        td.append(wall(run_batch))
    med = lambda v: round(float(np.median(v)), 1)   # noqa: E731
    a, b, c, d = med(res[8][0]), med(res[8][1]), med(tc), med(td)
    doc = {"what": "Fuse of %d map points into K = %d key frames of about %d key points at %dx%d, th 3" % (npts, K, int(n.mean()), W, H),
           "K": K, "points": npts, "cap": int(cap), "reps": args.reps, "mean_keypoints": round(float(n.mean()), 1),
           "results_within_TH_LOW": fused,
           "a_fuse_device_csr_given_us_median": a, "a_min": round(float(np.min(res[8][0])), 1), "a_max": round(float(np.max(res[8][0])), 1),
           "b_fuse_device_csr_inside_us_median": b, "b_min": round(float(np.min(res[8][1])), 1), "b_max": round(float(np.max(res[8][1])), 1),
           "c_K_times_orbhip_fuse_us_median": c, "c_min": round(float(np.min(tc)), 1), "c_max": round(float(np.max(tc)), 1),
           "d_fuse_batch_host_us_median": d, "d_min": round(float(np.min(td)), 1), "d_max": round(float(np.max(td)), 1),
           "clocks": "a, b: HIP events on the matcher's stream (device time of the call); c, d: wall clock of synchronous host calls",
           "c_over_b": round(c / b, 1), "c_over_d": round(c / d, 1), "batched_not_slower": bool(b <= c and d <= c)}
    if args.mappings:
        doc["mappings"] = {"kept_8_lanes_per_query_us_median": {"csr_given": a, "csr_inside": b},
                           "dropped_one_wavefront_per_query_us_median": {"csr_given": med(res[64][0]), "csr_inside": med(res[64][1])}}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
