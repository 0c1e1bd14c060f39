"""Seeding stereo / RGB-D map points on the device (orbhip_seed_stereo_points*, orbhip_count_close_points*) against the
sequential restatement tests/seqref/seed.py: world, flags, order, created and the counts bit for bit, host and device
entries, both modes, and the composition extract -> ComputeStereoMatches -> seed -> TrackLastFrame on one stream."""
import ctypes as C

import numpy as np
import pytest

from helpers import synth_stereo
from seqref import seed as SS

pytestmark = pytest.mark.gpu

FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
KK = (FX, FY, CX, CY)
P, O = SS.POINT_PRESENT, SS.POINT_OBSERVED
SIZES = (0, 1, 63, 64, 65, 100, 101, 102, 1000, 2047, 4096)
SENT = np.float32(-12345.5)


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd import matcher as M
    sf = np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2))])).astype(np.float32)
    cam = M.make_camera(FX, FY, CX, CY, (0.0, 0.0, 1241.0, 376.0), sf, mbf=BF, mb=BF / FX)
    return pkg, M, cam


def _pose(rng):
    """A random rigid pose, float32 3x4."""
    a = rng.normal(0, 0.7, 3)
    th = np.linalg.norm(a)
    k = a / max(th, 1e-12)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = R.astype(np.float32)
    T[:, 3] = rng.normal(0, 3.0, 3).astype(np.float32)
    return T


def _keys(pkg, rng, n):
    k = np.zeros(n, pkg.KP_DTYPE)
    k["x"] = rng.uniform(0, 1241, n).astype(np.float32)
    k["y"] = rng.uniform(0, 376, n).astype(np.float32)
    return k


def _depths(rng, n, valid_frac=0.8):
    """Random depths with planted exact ties, +inf, NaN, -1 and 0."""
    z = rng.uniform(0.5, 80.0, n).astype(np.float32)
    if n >= 8:
        ties = rng.integers(0, n, n // 4)
        z[ties] = z[rng.integers(0, n, n // 4)]                  # exact ties
        z[rng.integers(0, n, max(1, n // 50))] = np.inf
        z[rng.integers(0, n, max(1, n // 50))] = np.nan
    bad = rng.random(n) >= valid_frac
    z[bad] = rng.choice(np.array([-1.0, 0.0, -0.0], np.float32), bad.sum())
    return z


def _th(rng, z, want_close):
    """A threshold with about want_close valid depths at or below it (one of them exactly equal to it)."""
    v = np.sort(z[z > 0])
    if len(v) == 0:
        return np.float32(10.0)
    return v[min(len(v) - 1, want_close)]


def _ref(Tcw, keys, depth, th, mode, cf, world, flags):
    return SS.seed_stereo_points(KK, Tcw, np.stack([keys["x"], keys["y"]], 1), depth, th, mode, cf, world, flags)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("n", SIZES)
def test_host_entry_equals_seqref(env, n):
    pkg, M, cam = env
    m = pkg.ORBmatcher(0.9, True)
    rng = np.random.default_rng(1000 + n)
    seen_c = set()
    for mode in (SS.SEED_CLOSEST, SS.SEED_ALL):
        for cf in (P, P | O):
            for want_close in (30, 100, 101, 400):
                keys, z, Tcw = _keys(pkg, rng, n), _depths(rng, n), _pose(rng)
                th = _th(rng, z, want_close)
                world = np.full((n, 3), SENT, np.float32)
                flags = rng.integers(0, 256, n).astype(np.uint8)
                rw, rf, ro, rc, rcounts = _ref(Tcw, keys, z, th, mode, cf, world, flags)
                w, fg, order, created, counts = m.SeedStereoPoints(cam, Tcw, keys, z, th, mode, cf, world, flags)
                what = (n, mode, cf, want_close)
                assert counts == rcounts, what
                assert np.array_equal(order, ro), what
                assert np.array_equal(created, rc), what
                assert np.array_equal(fg, rf), what
                assert _same_bits(w, rw), what
                keep = created == 0                                 # entries that were not created are untouched
                assert np.all(w[keep] == SENT) and np.array_equal(fg[keep], flags[keep])
                assert np.all(world == SENT)                        # the caller's arrays are not written through
                seen_c.add(int(((z > 0) & ~(z > th)).sum()) > 100)
                tr, nt = m.CountClosePoints(z, flags, th)
                assert (tr, nt) == SS.count_close_points(z, flags, th), what
    if n >= 1000:
        assert seen_c == {False, True}                              # both c < 100 and c > 100 occurred


def test_no_positive_depth_and_capacity_and_arguments(env):
    pkg, M, cam = env
    from orb_slam2_comment_amd import capi
    m = pkg.ORBmatcher(0.9, True)
    rng = np.random.default_rng(3)
    keys, Tcw = _keys(pkg, rng, 50), _pose(rng)
    z = np.array([-1.0, 0.0, np.nan, -0.0, -np.inf] * 10, np.float32)
    world, flags = np.full((50, 3), SENT, np.float32), np.full(50, 3, np.uint8)
    for mode in (0, 1):
        w, fg, order, created, counts = m.SeedStereoPoints(cam, Tcw, keys, z, 10.0, mode, P, world, flags)
        assert counts == (0, 0, 0) and len(order) == 0 and not created.any() and np.all(w == SENT) and np.all(fg == 3)
    L, p = capi.lib(), capi.ptr
    big = 4097
    kb, zb = _keys(pkg, rng, big), np.ones(big, np.float32)
    wb, fb, ob, cnt = np.zeros((big, 3), np.float32), np.zeros(big, np.uint8), np.zeros(big, np.int32), np.full(3, -7, np.int32)
    T = np.ascontiguousarray(Tcw)
    assert L.orbhip_seed_stereo_points(m._h, C.byref(cam), p(T), p(kb), p(zb), big, 10.0, 1, 1, p(wb), p(fb), p(ob), p(fb),
                                       p(cnt)) == capi.E_CAPACITY
    assert L.orbhip_seed_stereo_points_device(m._h, 1, C.byref(cam), 256, 256, 256, big, 0, 1, 256, 10.0, 1, 1, 256, 256, 0, 0,
                                              256) == capi.E_CAPACITY      # refused before any pointer is used
    for bad in (dict(mode=2), dict(mode=-1), dict(cf=256), dict(cf=-1), dict(n=-1), dict(counts=None), dict(T=None)):
        a = dict(mode=1, cf=1, n=50, counts=p(cnt), T=p(T))
        a.update(bad)
        assert L.orbhip_seed_stereo_points(m._h, C.byref(cam), a["T"], p(keys), p(z), a["n"], 10.0, a["mode"], a["cf"], p(world),
                                           p(flags), None, None, a["counts"]) == capi.E_ARG, bad
    assert L.orbhip_seed_stereo_points(m._h, None, p(T), p(keys), p(z), 50, 10.0, 1, 1, p(world), p(flags), None, None,
                                       p(cnt)) == capi.E_ARG
    assert L.orbhip_seed_stereo_points_device(m._h, 1, C.byref(cam), 256, 256, 256, 64, -1, 1, 256, 10.0, 1, 1, 256, 256, 0, 0,
                                              256) == capi.E_ARG
    assert L.orbhip_count_close_points(m._h, p(z), p(flags), 50, 10.0, None, None) == capi.E_ARG
    assert cnt.tolist() == [-7] * 3 and np.all(world == SENT)
    # nullable order / created
    z2 = _depths(rng, 50)
    assert L.orbhip_seed_stereo_points(m._h, C.byref(cam), p(T), p(keys), p(z2), 50, 10.0, 1, 1, p(world), p(flags), None, None,
                                       p(cnt)) == capi.OK
    assert tuple(cnt) == _ref(Tcw, keys, z2, 10.0, 1, 1, np.full((50, 3), SENT, np.float32), np.full(50, 3, np.uint8))[4]


def _upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1) if a.dtype.fields else np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("mode,cf,kp_step", [(SS.SEED_CLOSEST, P, 1), (SS.SEED_CLOSEST, P | O, 2), (SS.SEED_ALL, P | O, 1),
                                             (SS.SEED_ALL, P, 2)])
def test_device_entry_batch_equals_seqref(env, mode, cf, kp_step):
    """72 frames in one launch, every size of the list among them; kp_step = 2 addresses the left frames of an interleaved
    stereo batch (the right frames' keypoints and counts are decoys)."""
    import torch
    pkg, M, cam = env
    rng = np.random.default_rng(77 + 10 * mode + cf + 100 * kp_step)
    F, cap = 72, 4096
    ns = list(SIZES) + [int(v) for v in rng.integers(0, cap + 1, F - len(SIZES))]
    rng.shuffle(ns)
    keys = np.zeros((F * kp_step, cap), pkg.KP_DTYPE)
    n_all = rng.integers(0, cap + 1, F * kp_step).astype(np.int32)
    depth = np.full((F, cap), np.float32(3.0))                  # beyond n: positive decoys that must not be read
    world = np.full((F, cap, 3), SENT, np.float32)
    flags = rng.integers(0, 256, (F, cap)).astype(np.uint8)
    Tcw = np.stack([_pose(rng) for _ in range(F)])
    ths = np.zeros(F, np.float32)
    for f in range(F):
        n = ns[f]
        n_all[f * kp_step] = n
        keys[f * kp_step, :n] = _keys(pkg, rng, n)
        for d in range(1, kp_step):
            keys[f * kp_step + d] = _keys(pkg, rng, cap)
        depth[f, :n] = _depths(rng, n, valid_frac=rng.choice([0.2, 0.8, 1.0]))
    th = _th(rng, depth[ns.index(1000), :1000], 150)            # one threshold per call: c < 100 and c > 100 both occur
    m = pkg.ORBmatcher(0.9, True)
    d_T, d_k, d_n, d_z = _upload(torch, Tcw.reshape(F, 12)), _upload(torch, keys), _upload(torch, n_all), _upload(torch, depth)
    d_w, d_f = _upload(torch, world), _upload(torch, flags)
    d_o = torch.full((F, cap), -9, dtype=torch.int32, device="cuda")
    d_c = torch.full((F, cap), 9, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((F, 3), -9, dtype=torch.int32, device="cuda")
    d_close = torch.full((F, 2), -9, dtype=torch.int32, device="cuda")
    d_nf = _upload(torch, np.array(ns, np.int32))
    torch.cuda.synchronize()
    m.CountClosePointsDevice(F, d_z.data_ptr(), d_f.data_ptr(), d_nf.data_ptr(), cap, th, d_close.data_ptr())
    m.SeedStereoPointsDevice(F, cam, d_T.data_ptr(), d_k.data_ptr(), d_n.data_ptr(), cap, 0, kp_step, d_z.data_ptr(), th, mode, cf,
                             d_w.data_ptr(), d_f.data_ptr(), d_cnt.data_ptr(), d_order=d_o.data_ptr(), d_created=d_c.data_ptr())
    m.sync()
    w, fg, od, cr, cnt, close = (t.cpu().numpy() for t in (d_w, d_f, d_o, d_c, d_cnt, d_close))
    cs = set()
    for f in range(F):
        n = ns[f]
        rw, rf, ro, rc, rcounts = _ref(Tcw[f], keys[f * kp_step, :n], depth[f, :n], th, mode, cf, world[f, :n], flags[f, :n])
        assert tuple(cnt[f]) == rcounts, (f, n)
        assert np.array_equal(od[f, :rcounts[1]], ro) and np.all(od[f, rcounts[1]:] == -9), (f, n)
        assert np.array_equal(cr[f, :n], rc) and np.all(cr[f, n:] == 9), (f, n)
        assert np.array_equal(fg[f, :n], rf) and np.array_equal(fg[f, n:], flags[f, n:]), (f, n)
        assert _same_bits(w[f, :n], rw) and np.all(w[f, n:] == SENT), (f, n)
        assert np.all(w[f, :n][rc == 0] == SENT)
        assert tuple(close[f]) == SS.count_close_points(depth[f, :n], flags[f, :n], th), (f, n)
        if rcounts[0] > 0:
            cs.add(int(((depth[f, :n] > 0) & ~(depth[f, :n] > th)).sum()) > 100)
    assert cs == {False, True}


def _extract_interleaved(torch, pkg, frames, nfeatures=1000, before_launch=None):
    B, H, W = frames.shape
    ext = pkg.ORBextractor(nfeatures, 1.2, 8, 20, 7)
    cap = ext.capacity(H, W)
    stream = torch.cuda.Stream()            # one explicit stream for the extractor and the matcher
    st = stream.cuda_stream
    ext.set_stream(st)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    if before_launch is not None:
        before_launch(cap)
    torch.cuda.synchronize()                # the buffers were filled on torch's stream
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    return ext, cap, st, (d_img, d_k, d_d, d_n, stream)


def _kps(pkg, d_k):
    B, cap = d_k.shape[:2]
    return d_k.cpu().numpy().view(np.uint8).reshape(B, cap, 28).copy().view(pkg.KP_DTYPE).reshape(B, cap)


def test_depths_of_the_real_chains(env):
    """mvDepth as the library produces it: ComputeStereoMatchesDevice on synthetic stereo pairs (sub-pixel disparities) and
    ComputeStereoFromRGBDRawDevice on the 16-bit synthetic depth image (many exact ties), seeded in both modes."""
    import torch
    pkg, M, cam = env
    from orb_slam2_comment_amd import capi
    from orb_slam2_comment_amd.synth import synth_depth, synth_frame
    rng = np.random.default_rng(9)
    # stereo, interleaved batch
    Pn, H, W = 3, 376, 1241
    frames = np.stack([im for p in range(Pn) for im in synth_stereo(40 + p, W, H)])
    ext, cap, st, (d_img, d_k, d_d, d_n, _s) = _extract_interleaved(torch, pkg, frames)
    assert cap <= 4096
    m = pkg.ORBmatcher(0.9, True)
    m.set_stream(st)
    mbf, mb = float(np.float32(BF)), float(np.float32(BF) / np.float32(FX))
    d_ur = torch.full((Pn, cap), -7.0, dtype=torch.float32, device="cuda")
    d_dp = torch.full((Pn, cap), -7.0, dtype=torch.float32, device="cuda")
    d_nm = torch.zeros(Pn, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.ComputeStereoMatchesDevice(ext, 0, 2, ext, 1, 2, Pn, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), d_k.data_ptr(),
                                 d_d.data_ptr(), d_n.data_ptr(), cap, mbf, mb, d_ur.data_ptr(), d_dp.data_ptr(), d_nm.data_ptr())
    Tcw = np.stack([_pose(rng) for _ in range(Pn)])
    d_T = _upload(torch, Tcw.reshape(Pn, 12))
    torch.cuda.synchronize()
    kps, n, dp = _kps(pkg, d_k), d_n.cpu().numpy(), d_dp.cpu().numpy()
    for mode, cf, th in ((SS.SEED_CLOSEST, P, np.float32(6.0)), (SS.SEED_CLOSEST, P | O, np.float32(40.0)), (SS.SEED_ALL, P | O, np.float32(0))):
        world = np.full((Pn, cap, 3), SENT, np.float32)
        flags = rng.integers(0, 4, (Pn, cap)).astype(np.uint8)
        d_w, d_f = _upload(torch, world), _upload(torch, flags)
        d_o = torch.full((Pn, cap), -9, dtype=torch.int32, device="cuda")
        d_c = torch.full((Pn, cap), 9, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((Pn, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.SeedStereoPointsDevice(Pn, cam, d_T.data_ptr(), d_k.data_ptr(), d_n.data_ptr(), cap, 0, 2, d_dp.data_ptr(), th, mode, cf,
                                 d_w.data_ptr(), d_f.data_ptr(), d_cnt.data_ptr(), d_order=d_o.data_ptr(), d_created=d_c.data_ptr())
        m.sync()
        w, fg, od, cr, cnt = (t.cpu().numpy() for t in (d_w, d_f, d_o, d_c, d_cnt))
        for p in range(Pn):
            nl = int(n[2 * p])
            rw, rf, ro, rc, rcounts = _ref(Tcw[p], kps[2 * p, :nl], dp[p, :nl], th, mode, cf, world[p, :nl], flags[p, :nl])
            assert tuple(cnt[p]) == rcounts and rcounts[0] > 100, (mode, p, rcounts)
            assert np.array_equal(od[p, :rcounts[1]], ro) and np.array_equal(cr[p, :nl], rc) and np.array_equal(fg[p, :nl], rf)
            assert _same_bits(w[p, :nl], rw) and np.all(w[p, nl:] == SENT)
    # RGB-D: raw 16-bit depth sampled at the keypoints
    Wd, Hd = 640, 480
    img = synth_frame(71, Wd, Hd)
    raw = synth_depth(71, Wd, Hd)
    ext2, cap2, st2, (d_img2, d_k2, d_d2, d_n2, _s2) = _extract_interleaved(torch, pkg, img[None], 1500)
    m.set_stream(st2)
    d_raw = torch.from_numpy(raw.view(np.int16)).cuda()
    d_ur2 = torch.zeros((1, cap2), dtype=torch.float32, device="cuda")
    d_dp2 = torch.zeros((1, cap2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m.compute_stereo_from_rgbd_raw_device(1, d_k2.data_ptr(), 0, d_n2.data_ptr(), cap2, d_raw.data_ptr(), capi.DEPTH_U16, Hd, Wd,
                                          np.float32(1.0) / np.float32(5000.0), 40.0, d_ur2.data_ptr(), d_dp2.data_ptr())
    torch.cuda.synchronize()
    k2, n2, z2 = _kps(pkg, d_k2)[0], int(d_n2.cpu().numpy()[0]), d_dp2.cpu().numpy()[0]
    zv = z2[:n2][z2[:n2] > 0]
    assert len(zv) > 500 and len(np.unique(zv)) < len(zv)            # exact ties are there
    T2 = _pose(rng)
    d_T2 = _upload(torch, T2.reshape(1, 12))
    for th in (np.float32(0.7), np.float32(3.09)):
        world = np.full((1, cap2, 3), SENT, np.float32)
        flags = rng.integers(0, 4, (1, cap2)).astype(np.uint8)
        d_w, d_f = _upload(torch, world), _upload(torch, flags)
        d_o = torch.full((1, cap2), -9, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.SeedStereoPointsDevice(1, cam, d_T2.data_ptr(), d_k2.data_ptr(), d_n2.data_ptr(), cap2, 0, 1, d_dp2.data_ptr(), th,
                                 SS.SEED_CLOSEST, P, d_w.data_ptr(), d_f.data_ptr(), d_cnt.data_ptr(), d_order=d_o.data_ptr())
        m.sync()
        rw, rf, ro, rc, rcounts = _ref(T2, k2[:n2], z2[:n2], th, SS.SEED_CLOSEST, P, world[0, :n2], flags[0, :n2])
        assert tuple(d_cnt.cpu().numpy()[0]) == rcounts
        assert np.array_equal(d_o.cpu().numpy()[0, :rcounts[1]], ro) and np.array_equal(d_f.cpu().numpy()[0, :n2], rf)
        assert _same_bits(d_w.cpu().numpy()[0, :n2], rw)


def test_composition_with_the_tracking_step(env):
    """extract (interleaved stereo batch: last pair, current pair) -> ComputeStereoMatchesDevice -> SeedStereoPointsDevice
    (CLOSEST, zero flags) -> TrackLastFrameDevice on one stream, nothing copied to the host in between; the same track call
    fed by seqref-made world / flags uploaded from the host gives the same d_assign / d_nmatches bit for bit."""
    import torch
    pkg, M, cam = env
    H, W, th_track = 376, 1241, 7.0
    last, cur = synth_stereo(21, W, H), synth_stereo(21, W, H, shift_xy=(3, 0))
    frames = np.stack([last[0], last[1], cur[0], cur[1]])
    B = 4
    mbf, mb = float(np.float32(BF)), float(np.float32(BF) / np.float32(FX))
    th_depth = SS.th_depth(BF, 35, FX)
    T = np.eye(4, dtype=np.float32)[:3].reshape(1, 12)
    bufs = {}

    def alloc(cap):
        # arrays indexed by the frame's place in the extractor batch, which is how TrackLastFrameDevice addresses them
        bufs["ur"] = torch.full((B, cap), -1.0, dtype=torch.float32, device="cuda")
        bufs["dp"] = torch.full((B, cap), -1.0, dtype=torch.float32, device="cuda")
        bufs["nm"] = torch.zeros(B, dtype=torch.int32, device="cuda")
        bufs["w"] = torch.zeros((B, cap, 3), dtype=torch.float32, device="cuda")
        bufs["f"] = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
        bufs["cnt"] = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
        bufs["Tl"], bufs["Tc"] = _upload(torch, T), _upload(torch, T)
        bufs["assign"] = torch.full((1, cap), -5, dtype=torch.int32, device="cuda")
        bufs["nmatch"] = torch.zeros(1, dtype=torch.int32, device="cuda")

    m = pkg.ORBmatcher(0.9, True)
    ext, cap, st, (d_img, d_k, d_d, d_n, _s) = _extract_interleaved(torch, pkg, frames, before_launch=alloc)
    m.set_stream(st)
    d_ur, d_dp, d_nm, d_w, d_f, d_cnt = (bufs[k] for k in ("ur", "dp", "nm", "w", "f", "cnt"))
    d_Tl, d_Tc, d_assign, d_nmatch = (bufs[k] for k in ("Tl", "Tc", "assign", "nmatch"))
    # from here to the synchronize below: one stream, no host copy
    for l0 in (0, 2):          # pair (l0, l0 + 1) -> row l0 of the output arrays
        m.ComputeStereoMatchesDevice(ext, l0, 2, ext, l0 + 1, 2, 1, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), d_k.data_ptr(),
                                     d_d.data_ptr(), d_n.data_ptr(), cap, mbf, mb, d_ur[l0].data_ptr(), d_dp[l0].data_ptr(),
                                     d_nm[l0:].data_ptr())
    m.SeedStereoPointsDevice(1, cam, d_Tl.data_ptr(), d_k.data_ptr(), d_n.data_ptr(), cap, 0, 1, d_dp.data_ptr(), th_depth,
                             SS.SEED_CLOSEST, P, d_w.data_ptr(), d_f.data_ptr(), d_cnt.data_ptr())
    m.TrackLastFrameDevice(1, cam, d_Tc.data_ptr(), d_Tl.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, 2, 1, 0, 1,
                           d_w.data_ptr(), d_f.data_ptr(), th_track, False, d_assign.data_ptr(), d_nmatch.data_ptr(),
                           d_u_right=d_ur.data_ptr())
    torch.cuda.synchronize()
    assign, nmatch = d_assign.cpu().numpy().copy(), d_nmatch.cpu().numpy().copy()
    # the host's version of the seeding step, from the downloaded depths
    kps, n, dp = _kps(pkg, d_k), d_n.cpu().numpy(), d_dp.cpu().numpy()
    n0 = int(n[0])
    rw, rf, ro, rc, rcounts = _ref(T.reshape(3, 4), kps[0, :n0], dp[0, :n0], th_depth, SS.SEED_CLOSEST, P,
                                   np.zeros((n0, 3), np.float32), np.zeros(n0, np.uint8))
    assert tuple(d_cnt.cpu().numpy()[0]) == rcounts and rcounts[2] == rcounts[1] > 100
    assert _same_bits(d_w.cpu().numpy()[0, :n0], rw) and np.array_equal(d_f.cpu().numpy()[0, :n0], rf)
    world = np.zeros((B, cap, 3), np.float32)
    flags = np.zeros((B, cap), np.uint8)
    world[0, :n0], flags[0, :n0] = rw, rf
    d_w2, d_f2 = _upload(torch, world), _upload(torch, flags)
    d_assign2 = torch.full((1, cap), -5, dtype=torch.int32, device="cuda")
    d_nmatch2 = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.TrackLastFrameDevice(1, cam, d_Tc.data_ptr(), d_Tl.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, 2, 1, 0, 1,
                           d_w2.data_ptr(), d_f2.data_ptr(), th_track, False, d_assign2.data_ptr(), d_nmatch2.data_ptr(),
                           d_u_right=d_ur.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(assign, d_assign2.cpu().numpy()) and np.array_equal(nmatch, d_nmatch2.cpu().numpy())
    # the seeded points carry POINT_PRESENT alone (nobody observes them yet), so an accepted query does not block its slot
    # (src/ORBmatcher.cc:1403-1405): a later query may take the slot over, nmatches counts both, assign keeps the last
    held = int((assign[0, :int(n[2])] >= 0).sum())
    assert 30 < held <= int(nmatch[0])
