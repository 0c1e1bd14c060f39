#!/usr/bin/env python3
"""Cost of creating one key frame's new map points against its K neighbours (LocalMapping::CreateNewMapPoints), same
process, same data.

  K = 20 neighbours of about 1000 key points at 1241x376 (one scene under 20 sideways shifts of 20 ... 58 px, extracted in
  one batch with the current key frame): a plane at 20 m seen from cameras 0.56 ... 1.6 m to the side, KITTI intrinsics,
  half of the key points stereo, 30 % of the slots already holding a map point, check_ori = 0 (what LocalMapping uses).
  Node ids are a stand-in for the FeatureVector level: descriptor byte 0 mod 100, about 10 key points per node and frame,
  as levelsup 2 of a k = 10, L = 4 tree gives.

  (a) CreateNewMapPointsDevice: three launches.  HIP-event time on the matcher's stream, warm, median over --reps.
  (b) CreateNewMapPoints, the host entry: one staged copy, (a), one read-back.  Wall clock.
  (c) the only route without the entry, for a caller whose frames live in device memory: download of the K + 1 frame rows
      into page-locked memory, K x orbhip_search_for_triangulation on them (raw C calls on prepared arguments; F12 and the
      epipole are handed in precomputed, which favours this route), the loop body of :286-431 in numpy (vectorised per
      neighbour, float64, batched np.linalg.svd), upload of matches, points and status codes.  Wall clock.
  (d) optionally the log of a headline A/B (lines "[label] value ...", parent and new interleaved in one call on one box,
      the parent twice, each from its own tree): the numbers are copied into the JSON.

  The match rows of (a), (b) and (c) are compared exactly, the status codes of (c) against (a) by share (float64 against
  the library's fp32 order of operations: at least 98 % of the matched pairs agree), before anything is timed.
  python tools/bench_triangulate.py [--reps 30] [--warmup 5] [--ab-log FILE --parent-label SUBSTR]
                                    [--out profiles/triangulate_stage.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, NF, K = 1241, 376, 1000, 20
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
Z = 20.0
(CREATED, NO_MATCH, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE) = range(10)


def host_triangulate(T1, T2, k1, ur1, z1, k2, ur2, z2, sf, mb):
    """The loop body of LocalMapping::CreateNewMapPoints (:286-431) for the matched pairs of one neighbour, float64."""
    M = len(k1)
    st = np.full(M, CREATED, np.uint8)
    X = np.zeros((M, 3))
    if M == 0:
        return st, X.astype(np.float32)
    T1, T2 = T1.astype(np.float64), T2.astype(np.float64)
    s1, s2 = ur1 >= 0, ur2 >= 0
    xn1 = np.stack([(k1["x"] - CX) / FX, (k1["y"] - CY) / FY, np.ones(M)], 1)
    xn2 = np.stack([(k2["x"] - CX) / FX, (k2["y"] - CY) / FY, np.ones(M)], 1)
    r1, r2 = xn1 @ T1[:, :3], xn2 @ T2[:, :3]                       # Rwc * xn
    cos_rays = (r1 * r2).sum(1) / (np.linalg.norm(r1, axis=1) * np.linalg.norm(r2, axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        c1 = np.where(s1, np.cos(2 * np.arctan2(mb / 2, z1.astype(np.float64))), cos_rays + 1)
        c2 = np.where(~s1 & s2, np.cos(2 * np.arctan2(mb / 2, z2.astype(np.float64))), cos_rays + 1)
    linear = (cos_rays < np.minimum(c1, c2)) & (cos_rays > 0) & (s1 | s2 | (cos_rays < 0.9998))
    from1 = ~linear & s1 & (c1 < c2)
    from2 = ~linear & ~from1 & s2 & (c2 < c1)
    st[~(linear | from1 | from2)] = LOW_PARALLAX
    A = np.stack([xn1[:, :1] * T1[2] - T1[0], xn1[:, 1:2] * T1[2] - T1[1],
                  xn2[:, :1] * T2[2] - T2[0], xn2[:, 1:2] * T2[2] - T2[1]], 1)
    x = np.linalg.svd(A)[2][:, 3]
    w0 = linear & (x[:, 3] == 0)
    st[w0] = W_ZERO
    with np.errstate(divide="ignore", invalid="ignore"):
        X[linear] = (x[:, :3] / x[:, 3:])[linear]
    O1, O2 = -T1[:, :3].T @ T1[:, 3], -T2[:, :3].T @ T2[:, 3]
    X[from1] = (xn1 * z1[:, None])[from1] @ T1[:, :3] + O1
    X[from2] = (xn2 * z2[:, None])[from2] @ T2[:, :3] + O2
    X[w0 | (st == LOW_PARALLAX)] = 0
    live = st == CREATED

    def gate(code, fails):
        nonlocal live
        st[live & fails] = code
        live = live & ~fails

    P1, P2 = X @ T1[:, :3].T + T1[:, 3], X @ T2[:, :3].T + T2[:, 3]
    gate(BEHIND_1, P1[:, 2] <= 0)
    gate(BEHIND_2, P2[:, 2] <= 0)
    for code, P, k, s, ur in ((REPROJ_1, P1, k1, s1, ur1), (REPROJ_2, P2, k2, s2, ur2)):
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = FX * P[:, 0] / P[:, 2] + CX, FY * P[:, 1] / P[:, 2] + CY
            e2 = (u - k["x"]) ** 2 + (v - k["y"]) ** 2
            e2s = e2 + (u - BF / P[:, 2] - ur) ** 2
        sig2 = (sf[k["octave"]] ** 2).astype(np.float64)
        gate(code, np.where(s, e2s > 7.8 * sig2, e2 > 5.991 * sig2))
    d1, d2 = np.linalg.norm(X - O1, axis=1), np.linalg.norm(X - O2, axis=1)
    gate(ZERO_DIST, (d1 == 0) | (d2 == 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        rd, ro, rf = d2 / d1, sf[k1["octave"]].astype(np.float64) / sf[k2["octave"]], 1.5 * float(sf[1])
    gate(SCALE, (rd * rf < ro) | (rd > ro * rf))
    return st, X.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab-log", default="")
    ap.add_argument("--parent-label", default="parent")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from orb_slam2_comment_amd import FrameView, KP_DTYPE, ORBextractor, ORBmatcher, capi
    from orb_slam2_comment_amd.matcher import make_camera
    from orb_slam2_comment_amd.synth import synth_frame
    rng = np.random.default_rng(3)
    B = K + 1
    shifts = [(0, 0)] + [(20 + 2 * k, k % 3) for k in range(K)]
    frames = np.stack([synth_frame(5, W, H, shift_xy=s) for s in shifts])
    stream = torch.cuda.Stream()
    ext = ORBextractor(NF, 1.2, 8, 20, 7)
    ext.set_stream(stream.cuda_stream)
    m = ORBmatcher(0.6, False)
    m.set_stream(stream.cuda_stream)
    cap = ext.capacity(H, W)
    sf = ext.GetScaleFactors()
    sigma2 = (sf * sf).astype(np.float32)
    bounds = (0.0, 0.0, float(W), float(H))
    mb = BF / FX
    cam = make_camera(FX, FY, CX, CY, bounds, sf, mbf=BF, mb=mb)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    ext.sync()
    n = d_n.cpu().numpy()
    hk = d_k.cpu().numpy().view(np.uint8).reshape(B, cap, 28).view(KP_DTYPE).reshape(B, cap)
    # frame f sees the scene shifted by (sx, sy) px: its camera stands sx*Z/fx, sy*Z/fy to the side of a plane at depth Z
    T = np.zeros((B, 3, 4), np.float32)
    T[:, :, :3] = np.eye(3, dtype=np.float32)
    T[:, 0, 3] = [s[0] * Z / FX for s in shifts]
    T[:, 1, 3] = [s[1] * Z / FY for s in shifts]
    stereo = rng.random((B, cap)) < 0.5
    ur = np.where(stereo, hk["x"] - np.float32(BF / Z), -1).astype(np.float32)
    dz = np.where(stereo, Z, -1).astype(np.float32)
    hp = (rng.random((B, cap)) < 0.3).astype(np.uint8)
    d_ur, d_z, d_hp = (torch.from_numpy(a).cuda() for a in (ur, dz, hp))
    d_node = (d_d[:, :, 0].to(torch.int32) % 100).contiguous()
    d_T = torch.from_numpy(T.reshape(B, 12)).cuda()
    d_idx = torch.arange(1, B, dtype=torch.int32, device="cuda")
    o_m = torch.zeros((K, cap), dtype=torch.int32, device="cuda")
    o_nm = torch.zeros(K, dtype=torch.int32, device="cuda")
    o_x = torch.zeros((K, cap, 3), dtype=torch.float32, device="cuda")
    o_st = torch.zeros((K, cap), dtype=torch.uint8, device="cuda")
    o_sk = torch.zeros(K, dtype=torch.uint8, device="cuda")
    o_f = torch.zeros((K, 9), dtype=torch.float32, device="cuda")
    o_e = torch.zeros((K, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def run_device():
        m.CreateNewMapPointsDevice(0, K, d_idx, cam, d_T, d_k, d_d, d_n, cap, d_node, sigma2, o_m, o_nm, o_x, o_st, o_sk,
                                   d_u_right=d_ur, d_depth=d_z, d_has_point=d_hp, d_f12=o_f, d_epipole=o_e)

    run_device()
    m.sync()
    n0 = int(n[0])
    a_m, a_nm, a_st, a_x = o_m.cpu().numpy()[:, :n0], o_nm.cpu().numpy(), o_st.cpu().numpy()[:, :n0], o_x.cpu().numpy()[:, :n0]
    assert not o_sk.cpu().numpy().any(), "a neighbour was skipped by the baseline gate"
    f12, ep = o_f.cpu().numpy(), o_e.cpu().numpy()

    # (c): page-locked host rows, allocated once like a caller's would be; the views point into them
    L, p = capi.lib(), capi.ptr
    pin = {name: torch.zeros(t.shape, dtype=t.dtype).pin_memory() for name, t in
           (("k", d_k), ("d", d_d), ("ur", d_ur), ("z", d_z), ("node", d_node), ("hp", d_hp))}
    hv = {name: t.numpy() for name, t in pin.items()}
    hkv = hv["k"].view(np.uint8).reshape(B, cap, 28).view(KP_DTYPE).reshape(B, cap)
    hnode = hv["node"].view(np.uint32)
    keep = [FrameView(hkv[f, :n[f]], hv["d"][f, :n[f]], sf, bounds, hv["ur"][f, :n[f]]) for f in range(B)]
    for f, v in enumerate(keep):       # the views alias the page-locked rows, no copy was made
        assert v.keys.ctypes.data == hkv[f].ctypes.data and v.desc.ctypes.data == hv["d"][f].ctypes.data
        assert v.u_right.ctypes.data == hv["ur"][f].ctypes.data
    cviews = [v.c_view() for v in keep]
    c_m = np.full((K, cap), -1, np.int32)
    c_x = np.zeros((K, cap, 3), np.float32)
    c_st = np.full((K, cap), NO_MATCH, np.uint8)
    h_m, h_x, h_st = (torch.from_numpy(a).pin_memory() for a in (c_m, c_x, c_st))
    c_m, c_x, c_st = h_m.numpy(), h_x.numpy(), h_st.numpy()
    u_m, u_x, u_st = torch.zeros_like(o_m), torch.zeros_like(o_x), torch.zeros_like(o_st)
    nm = C.c_int(0)
    f12k = [np.ascontiguousarray(f12[k]) for k in range(K)]

    def run_single():
        with torch.cuda.stream(stream):
            for name, t in (("k", d_k), ("d", d_d), ("ur", d_ur), ("z", d_z), ("node", d_node), ("hp", d_hp)):
                pin[name].copy_(t, non_blocking=True)
        stream.synchronize()
        valid = 1 - hv["hp"]
        c_st[:] = NO_MATCH
        for k in range(K):
            f = k + 1
            capi.check(L.orbhip_search_for_triangulation(m._h, C.byref(cviews[0]), p(hnode[0]), p(valid[0]), C.byref(cviews[f]),
                                                         p(hnode[f]), p(valid[f]), p(f12k[k]), float(ep[k, 0]), float(ep[k, 1]),
                                                         p(sigma2), 0, 0, p(c_m[k]), C.byref(nm)),
                       "orbhip_search_for_triangulation")
            i = np.nonzero(c_m[k, :n0] >= 0)[0]
            j = c_m[k, i]
            st, X = host_triangulate(T[0], T[f], hkv[0, i], hv["ur"][0, i], hv["z"][0, i], hkv[f, j], hv["ur"][f, j],
                                     hv["z"][f, j], sf, mb)
            c_st[k, i], c_x[k, i] = st, X
        with torch.cuda.stream(stream):
            u_m.copy_(h_m, non_blocking=True); u_x.copy_(h_x, non_blocking=True); u_st.copy_(h_st, non_blocking=True)
        stream.synchronize()

    # (b): raw C call on prepared arguments
    views = [FrameView(hk[f, :n[f]].copy(), d_d[f, :n[f]].cpu().numpy(), sf, bounds, ur[f, :n[f]].copy()) for f in range(B)]
    bviews = [v.c_view() for v in views]
    arr = (C.POINTER(capi.FrameView) * K)(*[C.pointer(bviews[f]) for f in range(1, B)])
    nodes_h = d_node.cpu().numpy().view(np.uint32)
    rows = {name: [np.ascontiguousarray(a[f, :n[f]]) for f in range(B)] for name, a in (("node", nodes_h), ("hp", hp), ("z", dz))}
    tabs = {name: (C.c_void_p * K)(*[r.ctypes.data for r in rows[name][1:]]) for name in rows}
    T0, Tn = np.ascontiguousarray(T[0].reshape(12)), np.ascontiguousarray(T[1:].reshape(K, 12))
    b_m, b_nm = np.full((K, n0), -1, np.int32), np.zeros(K, np.int32)
    b_x, b_st, b_sk = np.zeros((K, n0, 3), np.float32), np.zeros((K, n0), np.uint8), np.zeros(K, np.uint8)

    def run_batch():
        capi.check(L.orbhip_create_new_map_points(m._h, C.byref(bviews[0]), p(rows["node"][0]), p(rows["hp"][0]), p(rows["z"][0]),
                                                  p(T0), K, arr, tabs["node"], tabs["hp"], tabs["z"], p(Tn), None, C.byref(cam),
                                                  0, 0, p(sigma2), p(b_m), p(b_nm), p(b_x), p(b_st), p(b_sk), None, None),
                   "orbhip_create_new_map_points")

    run_single()
    run_batch()
    assert np.array_equal(b_m, a_m) and np.array_equal(b_nm, a_nm) and np.array_equal(b_st, a_st), "host entry disagrees"
    assert np.array_equal(b_x.view(np.uint32), a_x.view(np.uint32)), "host entry disagrees on x3d"
    assert np.array_equal(c_m[:, :n0], a_m), "K x orbhip_search_for_triangulation disagrees with the batched search"
    matched = a_m >= 0
    agree = float((c_st[:, :n0][matched] == a_st[matched]).mean())
    both = matched & (a_st == CREATED) & (c_st[:, :n0] == CREATED)
    x_err = float(np.abs(c_x[:, :n0][both] - a_x[both]).max()) if both.any() else 0.0
    assert agree >= 0.98, "numpy triangulation agrees with the library on %.4f of the matched pairs only" % agree

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def wall(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e6

    for _ in range(args.warmup):
        run_device(); run_single(); run_batch()
    m.sync()
    ta, tb, tc = [], [], []
    for _ in range(args.reps):          # interleaved, so that drift hits all alike
        ta.append(timed(run_device))
        tb.append(wall(run_batch))
        tc.append(wall(run_single))
    med = lambda v: round(float(np.median(v)), 1)   # noqa: E731
    lo = lambda v: round(float(np.min(v)), 1)       # noqa: E731
    hi = lambda v: round(float(np.max(v)), 1)       # noqa: E731
    a, b, c = med(ta), med(tb), med(tc)
    doc = {"what": "CreateNewMapPoints of a key frame of %d key points against K = %d neighbours of about %d at %dx%d, stereo, "
                   "check_ori 0" % (n0, K, int(n[1:].mean()), W, H),
           "K": K, "cap": int(cap), "reps": args.reps, "mean_keypoints": round(float(n.mean()), 1),
           "matched_pairs": int(matched.sum()), "created": int((a_st == CREATED).sum()),
           "status_histogram": np.bincount(a_st[matched], minlength=10).tolist(),
           "c_status_agreement_with_a": round(agree, 4), "c_x3d_max_abs_difference_m": round(x_err, 6),
           "a_device_call_us_median": a, "a_min": lo(ta), "a_max": hi(ta),
           "b_host_entry_us_median": b, "b_min": lo(tb), "b_max": hi(tb),
           "c_K_searches_numpy_triangulation_us_median": c, "c_min": lo(tc), "c_max": hi(tc),
           "clocks": "a: HIP events on the matcher's stream (device time of the call); b, c: wall clock of synchronous host work",
           "c_over_a": round(c / a, 1), "c_over_b": round(c / b, 1), "batched_not_slower": bool(a <= c and b <= c)}
    if args.ab_log:
        runs = {"parent": [], "new": []}
        for ln in open(args.ab_log):
            if ln.startswith("["):
                label, rest = ln[1:].split("]", 1)
                runs["parent" if args.parent_label in label else "new"].append(float(rest.split()[0]))
        plo, phi = (min(runs["parent"]), max(runs["parent"])) if runs["parent"] else (None, None)
        doc["d_headline"] = {"how": "bench.py --full --no-cpu-baseline --no-secondary, one call on one box, interleaved parent / new / "
                                    "parent / new; the parent is the parent commit's whole tree with its own library, because its "
                                    "binding declares fewer symbols",
                             "unit": "frames/s, higher is better",
                             "parent_runs": runs["parent"], "new_runs": runs["new"], "parent_spread": [plo, phi],
                             "new_within_parent_spread": [bool(plo <= v <= phi) for v in runs["new"]] if runs["parent"] else None,
                             "new_below_parent_min": [bool(v < plo) for v in runs["new"]] if runs["parent"] else None}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
