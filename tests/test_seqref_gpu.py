"""The HIP kernels against the sequential reference (tests/seqref), through the public entry points: keypoints,
descriptors, assignment arrays, match counts and stereo outputs must be identical."""
import numpy as np
import pytest

from helpers import assert_kps_equal, frame_bounds, synth_frame, synth_stereo
from seqref import extractor as SX
from seqref import matcher as SM

pytestmark = pytest.mark.gpu

f32 = np.float32
KITTI_FX, KITTI_CX, KITTI_CY, KITTI_BF = 718.856, 607.1928, 185.2157, 386.1448


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd import matcher as M
    return pkg, M


@pytest.fixture(scope="module")
def kitti_pair(env):
    pkg, M = env
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    k1, d1 = ext(synth_frame(4))
    k2, d2 = ext(synth_frame(4, shift_xy=(3, 0)))
    return k1, d1, k2, d2, ext.GetScaleFactors()


@pytest.mark.parametrize("W,H,nf,seed", [(1241, 376, 1000, 1), (1241, 376, 1000, 2), (1241, 376, 1000, 3),
                                         (752, 480, 2000, 1)])
def test_extractor_equals_seqref(env, W, H, nf, seed):
    """The bench's synth_frame(1|2|3) at 1241x376 @1000 and configs[4]'s 752x480 @2000."""
    pkg, M = env
    img = synth_frame(seed, W, H)
    k, d = pkg.ORBextractor(nf, 1.2, 8, 20, 7)(img)
    sk, sd = SX.extract(img, nf, 1.2, 8, 20, 7)
    assert_kps_equal(k, sk, "seed %d %dx%d" % (seed, W, H))
    assert np.array_equal(d, sd)


def _last_frame_queries(M, k_last, sf, th, rng, bf):
    fx, cx, cy = KITTI_FX, KITTI_CX, KITTI_CY
    z = rng.uniform(4, 40, len(k_last)).astype(f32)
    X = np.stack([(k_last["x"] - cx) * z / fx, (k_last["y"] - cy) * z / fx, z], 1).astype(f32)
    T = np.eye(4, dtype=f32)
    T[0, 3] = 3 * 15.0 / fx
    return M.project_last_frame(T, (fx, fx, cx, cy), (0, 0, 1241, 376), X, k_last["octave"], k_last["angle"],
                                rng.random(len(k_last)) < 0.85, rng.random(len(k_last)) < 0.7, sf, th, mbf=bf)


@pytest.mark.parametrize("th,stereo", [(15, False), (7, True)])
def test_search_by_projection_frame_equals_seqref(env, kitti_pair, th, stereo):
    """SearchByProjection(CurrentFrame, LastFrame): th 15 mono, th 7 stereo with the ur gate (src/Tracking.cc:880-892)."""
    pkg, M = env
    k1, d1, k2, d2, sf = kitti_pair
    rng = np.random.default_rng(th)
    ur = np.where(rng.random(len(k2)) < 0.6, k2["x"] - rng.uniform(2, 60, len(k2)), -1).astype(f32) if stereo else None
    b = (0.0, 0.0, 1241.0, 376.0)
    q = _last_frame_queries(M, k1, sf, th, rng, KITTI_BF if stereo else 0.0)
    taken = (rng.random(len(k2)) < 0.05).astype(np.uint8)
    for ori in (True, False):
        n, a = pkg.ORBmatcher(0.9, ori).SearchByProjectionFrame(pkg.FrameView(k2, d2, sf, b, ur), q, d1, taken)
        sn, sa = SM.search_by_projection_frame(SM.Frame(k2, d2, ur, b, sf), q, d1, taken, ori)
        assert n == sn and np.array_equal(a, sa) and n > 100


def test_fused_track_last_frame_equals_seqref(env):
    """orbhip_track_last_frame_device (the headline's fused prologue + search) against seqref's search on the
    queries of the device prologue, for every pair of a small batch, mono th 15 and stereo th 7."""
    torch = pytest.importorskip("torch")
    pkg, M = env
    rng = np.random.default_rng(5)
    dev = torch.device("cuda", 0)
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    frames = np.stack([synth_frame(1 + (i // 2) % 3, shift_xy=(3 * (i % 2), 0)) for i in range(6)])
    B, H, W = frames.shape
    cap = ext.capacity(H, W)
    d_img = torch.from_numpy(frames).to(dev)
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ext.set_stream(st)
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    torch.cuda.synchronize()
    kps = d_k.cpu().numpy().view(np.uint8).reshape(B, cap, 28).copy().view(pkg.KP_DTYPE).reshape(B, cap)
    desc, n = d_d.cpu().numpy(), d_n.cpu().numpy()
    sf = ext.GetScaleFactors()
    bounds = frame_bounds(frames[0])
    cam = M.make_camera(KITTI_FX, KITTI_FX, KITTI_CX, KITTI_CY, bounds, sf, mbf=KITTI_BF, mb=KITTI_BF / KITTI_FX)
    pairs = B // 2
    zc = f32(12.0)
    Tlw = np.stack([np.eye(4, dtype=f32) for _ in range(pairs)])
    Tcw = Tlw.copy()
    Tcw[:, 0, 3] = f32(3.0) * zc / f32(KITTI_FX)
    world = np.zeros((B, cap, 3), f32)
    flags = np.zeros((B, cap), np.uint8)
    for p in range(pairs):
        kl = kps[2 * p, :n[2 * p]]
        world[2 * p, :n[2 * p], 0] = (kl["x"] - f32(KITTI_CX)) * zc / f32(KITTI_FX)
        world[2 * p, :n[2 * p], 1] = (kl["y"] - f32(KITTI_CY)) * zc / f32(KITTI_FX)
        world[2 * p, :n[2 * p], 2] = zc
        flags[2 * p, :n[2 * p]] = (rng.random(n[2 * p]) < 0.9) * pkg.capi.POINT_PRESENT + \
            (rng.random(n[2 * p]) < 0.7) * pkg.capi.POINT_OBSERVED
    taken = (rng.random((pairs, cap)) < 0.05).astype(np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_Tcw, d_Tlw = t(Tcw[:, :3, :].reshape(pairs, 12)), t(Tlw[:, :3, :].reshape(pairs, 12))
    d_world, d_flags, d_taken = t(world), t(flags), t(taken)
    d_q = torch.zeros((pairs, cap, 10), dtype=torch.int32, device=dev)
    d_nq = torch.zeros(pairs, dtype=torch.int32, device=dev)
    d_assign = torch.zeros((pairs, cap), dtype=torch.int32, device=dev)
    d_nm = torch.zeros(pairs, dtype=torch.int32, device=dev)
    for mono, th in ((True, 15.0), (False, 7.0)):
        m = pkg.ORBmatcher(0.9, True)
        m.set_stream(st)
        m.ProjectLastFrameDevice(pairs, cam, d_Tcw.data_ptr(), d_Tlw.data_ptr(), d_k.data_ptr(), d_n.data_ptr(), cap, 0, 2,
                                 d_world.data_ptr(), d_flags.data_ptr(), th, mono, d_q.data_ptr(), d_nq.data_ptr())
        m.TrackLastFrameDevice(pairs, cam, d_Tcw.data_ptr(), d_Tlw.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(),
                               cap, 1, 2, 0, 2, d_world.data_ptr(), d_flags.data_ptr(), th, mono, d_assign.data_ptr(),
                               d_nm.data_ptr(), d_taken=d_taken.data_ptr())
        torch.cuda.synchronize()
        qd = d_q.cpu().numpy().view(np.uint8).reshape(pairs, cap, 40).copy().view(pkg.QUERY_DTYPE).reshape(pairs, cap)
        assign, nm = d_assign.cpu().numpy(), d_nm.cpu().numpy()
        for p in range(pairs):
            fl, fc = 2 * p, 2 * p + 1
            S = SM.Frame(kps[fc, :n[fc]], desc[fc, :n[fc]], None, bounds, sf)
            sn, sa = SM.search_by_projection_frame(S, qd[p, :n[fl]], desc[fl, :n[fl]], taken[p, :n[fc]], True)
            assert nm[p] == sn and np.array_equal(assign[p, :n[fc]], sa), (mono, p)
            assert sn > 300


@pytest.mark.parametrize("th", [1, 3, 5])
def test_search_by_projection_points_equals_seqref(env, kitti_pair, th):
    """SearchByProjection(F, vpMapPoints, th) as SearchLocalPoints calls it (nnratio 0.8, th 1/3/5)."""
    pkg, M = env
    k1, d1, k2, d2, sf = kitti_pair
    rng = np.random.default_rng(30 + th)
    b = (0.0, 0.0, 1241.0, 376.0)
    ur = np.where(rng.random(len(k2)) < 0.5, k2["x"] - rng.uniform(2, 60, len(k2)), -1).astype(f32)
    nq = len(k1)
    q = np.zeros(nq, pkg.QUERY_DTYPE)
    q["valid"] = rng.random(nq) < 0.9
    q["u"] = k1["x"] + 3 + rng.normal(0, 1.0, nq).astype(f32)
    q["v"] = k1["y"] + rng.normal(0, 1.0, nq).astype(f32)
    pred = np.clip(k1["octave"] + rng.integers(-1, 2, nq), 0, 7)
    r = np.array([M.RadiusByViewingCos(c) for c in rng.uniform(0.99, 1.0, nq)], f32)
    if th != 1:
        r = r * f32(th)
    q["radius"] = r * sf[pred]
    q["min_level"], q["max_level"], q["level_aux"] = pred - 1, pred, pred
    q["ur"] = q["u"] - rng.uniform(2, 60, nq).astype(f32)
    q["observed"] = rng.random(nq) < 0.8
    taken = (rng.random(len(k2)) < 0.1).astype(np.uint8)
    n, a = pkg.ORBmatcher(0.8, True).SearchByProjectionPoints(pkg.FrameView(k2, d2, sf, b, ur), q, d1, taken)
    sn, sa = SM.search_by_projection_points(SM.Frame(k2, d2, ur, b, sf), q, d1, taken, 0.8)
    assert n == sn and np.array_equal(a, sa) and n > 50


def test_search_for_initialization_equals_seqref(env):
    """configs[4]: 752x480 @2000, windowSize 100, nnratio 0.9, two rounds from the updated vbPrevMatched."""
    pkg, M = env
    W, H = 752, 480
    ext = pkg.ORBextractor(2000, 1.2, 8, 20, 7)
    k1, d1 = ext(synth_frame(1, W, H))
    k2, d2 = ext(synth_frame(1, W, H, shift_xy=(5, 0)))
    sf = ext.GetScaleFactors()
    b = (0.0, 0.0, float(W), float(H))
    g1, g2 = pkg.FrameView(k1, d1, sf, b), pkg.FrameView(k2, d2, sf, b)
    s1, s2 = SM.Frame(k1, d1, None, b, sf), SM.Frame(k2, d2, None, b, sf)
    prev = sprev = np.stack([k1["x"], k1["y"]], 1).astype(f32)
    m = pkg.ORBmatcher(0.9, True)
    for _ in range(2):
        n, m12, prev = m.SearchForInitialization(g1, g2, prev, 100)
        sn, sm12, sprev = SM.search_for_initialization(s1, s2, sprev, 100, 0.9, True)
        assert n == sn and np.array_equal(m12, sm12) and np.array_equal(prev, sprev) and n > 50


def test_compute_stereo_matches_equals_seqref(env):
    """Frame::ComputeStereoMatches on a KITTI-shape pair; seqref works on its own pyramid of the two images."""
    pkg, M = env
    left, right = synth_stereo(1)
    eL, eR = pkg.ORBextractor(1000, 1.2, 8, 20, 7), pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    kl, dl = eL(left)
    kr, dr = eR(right)
    mbf = float(f32(KITTI_BF))
    mb = float(f32(KITTI_BF) / f32(KITTI_FX))
    n, ur, dp = pkg.ORBmatcher().ComputeStereoMatches(eL, eR, kl, dl, kr, dr, mbf, mb)
    t = SX.tables(1000, 1.2, 8)
    lv_l, _ = SX.compute_pyramid(left, t["inv_scale"])
    lv_r, _ = SX.compute_pyramid(right, t["inv_scale"])
    sn, sur, sdp = SM.compute_stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], mbf, mb)
    assert n == sn and n > 100
    assert np.array_equal(ur, sur) and np.array_equal(dp, sdp)


def _desc(nbits):
    bits = np.zeros(256, np.uint8)
    bits[:nbits] = 1
    return np.packbits(bits)


def _keys(pkg, xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), pkg.KP_DTYPE)
    k["x"], k["y"] = np.asarray(xy, f32).reshape(-1, 2).T
    k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = octave, angle, 31.0, 20.0, -1
    return k


def _queries(pkg, uv, radius, angle=0.0, observed=1, ur=-1.0, lmin=-1, lmax=-1):
    q = np.zeros(len(uv), pkg.QUERY_DTYPE)
    q["valid"] = 1
    q["u"], q["v"] = np.asarray(uv, f32).reshape(-1, 2).T
    q["radius"], q["min_level"], q["max_level"], q["ur"], q["angle"], q["observed"] = radius, lmin, lmax, ur, angle, observed
    return q


def test_constructed_edge_cases_equal_seqref(env):
    """The constructed inputs of test_seqref_cpu.py that the entry points can express: window edges and visiting
    order, level windows, TH_HIGH / TH_LOW, the level-conditional ratio test, exact-half rotation bins and the
    cull, two unobserved queries on one slot, the ur gate at er == radius."""
    pkg, M = env
    B = (0.0, 0.0, 640.0, 480.0)
    sf = SX.tables(1000, 1.2, 8)["scale"]

    def frame(k, d, ur=None):
        return pkg.FrameView(k, d, sf, B, ur), SM.Frame(k, d, ur, B, sf)

    def same_frame(k, d, q, qd, ori, ur=None, taken=None):
        g, s = frame(k, d, ur)
        got = pkg.ORBmatcher(0.9, ori).SearchByProjectionFrame(g, q, qd, taken)
        want = SM.search_by_projection_frame(s, q, qd, taken, ori)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (got, want)
        return want

    def same_points(k, d, q, qd, nnratio, ur=None):
        g, s = frame(k, d, ur)
        got = pkg.ORBmatcher(nnratio, True).SearchByProjectionPoints(g, q, qd)
        want = SM.search_by_projection_points(s, q, qd, None, nnratio)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (got, want)
        return want

    z1 = np.zeros((1, 32), np.uint8)
    # |dx| == r and the cell of x = 25 (2.5 -> 3): visiting order decides equal distances
    k = _keys(pkg, [(28, 100), (25, 100), (34.9, 100), (24.9, 100), (40, 100)])
    n, a = same_frame(k, np.zeros((5, 32), np.uint8), _queries(pkg, [(30, 100), (30, 100)], 10.0),
                      np.zeros((2, 32), np.uint8), False)
    assert a.tolist() == [1, -1, -1, 0, -1]
    # level windows (-1,-1), (0,-1), (1,-1), (2,2)
    k = _keys(pkg, [(100 + 2 * i, 100) for i in range(4)], octave=np.array([0, 1, 2, 3]))
    d = np.stack([_desc(i) for i in (0, 1, 2, 3)])
    for lo, hi, want in ((-1, -1, 0), (0, -1, 0), (1, -1, 1), (2, 2, 2), (4, -1, -1)):
        n, a = same_frame(k, d, _queries(pkg, [(103, 100)], 10.0, lmin=lo, lmax=hi), z1, False)
        assert (a.tolist().index(0) if 0 in a else -1) == want, (lo, hi)
    # TH_HIGH 100 / 101
    k = _keys(pkg, [(100, 100), (200, 100)])
    d = np.stack([_desc(100), _desc(101)])
    q = _queries(pkg, [(100, 100), (200, 100)], 5.0)
    assert same_frame(k, d, q, np.zeros((2, 32), np.uint8), False)[1].tolist() == [0, -1]
    assert same_points(k, d, q, np.zeros((2, 32), np.uint8), 0.8)[1].tolist() == [0, -1]
    # ratio test: equality passes, a second best on another level is no test at all
    for db, d2, lb, l2, r, want in ((30, 40, 1, 1, 0.75, 1), (31, 40, 1, 1, 0.75, 0), (40, 50, 2, 2, 0.8, 1),
                                    (39, 40, 1, 2, 0.75, 1), (39, 40, 2, 2, 0.75, 0)):
        k = _keys(pkg, [(100, 100), (102, 100)], octave=np.array([lb, l2]))
        assert same_points(k, np.stack([_desc(db), _desc(d2)]), _queries(pkg, [(101, 100)], 5.0), z1, r)[0] == want
    # TH_LOW 50 / 51 and the float ratio of SearchForInitialization
    for d_best, d_second, nnratio, want in ((50, 256, 0.9, 1), (51, 256, 0.9, 0), (30, 40, 0.75, 0), (29, 40, 0.75, 1)):
        k2 = _keys(pkg, [(100, 100), (102, 100)])
        d2 = np.stack([_desc(d_best), _desc(d_second)])
        k1 = _keys(pkg, [(101, 100)])
        prev = np.array([[101, 100]], f32)
        got = pkg.ORBmatcher(nnratio, False).SearchForInitialization(pkg.FrameView(k1, z1, sf, B), pkg.FrameView(k2, d2, sf, B),
                                                                     prev, 10)
        want_ = SM.search_for_initialization(SM.Frame(k1, z1, None, B, sf), SM.Frame(k2, d2, None, B, sf), prev, 10,
                                             nnratio, False)
        assert got[0] == want_[0] == want and np.array_equal(got[1], want_[1])
    # exact-half rotation bins and the cull
    rots = np.array([0.0] * 10 + [150.0] * 10 + [270.0] * 10 + [135.0, 255.0, float(np.nextafter(f32(135), f32(0))),
                                                                 float(np.nextafter(f32(360), f32(0))), 15.0], f32)
    xy = [(30 + 15 * (i % 38), 30 + 40 * (i // 38)) for i in range(len(rots))]
    q = _queries(pkg, xy, 3.0)
    q["angle"] = np.array([f32(f32(20.0) + r) for r in rots], f32) % f32(360)
    n, a = same_frame(_keys(pkg, xy, angle=f32(20.0)), np.zeros((len(rots), 32), np.uint8), q,
                      np.zeros((len(rots), 32), np.uint8), True)
    assert n == 32 and [i for i in range(len(rots)) if a[i] == i] == list(range(32))
    # two unobserved queries on one slot; the cull of the first one's bin empties the slot
    xy = [(100, 100)] + [(200 + 10 * i, 200) for i in range(12)]
    q = _queries(pkg, [(100, 100), (100, 100)] + [(200 + 10 * i, 200) for i in range(12)], 3.0, observed=0)
    q["angle"][0] = 300.0
    n, a = same_frame(_keys(pkg, xy), np.zeros((13, 32), np.uint8), q, np.zeros((14, 32), np.uint8), True)
    assert a[0] == -1 and n == 13
    # the ur gate at er == radius (passes) and just above it
    k = _keys(pkg, [(100, 100), (101, 100), (102, 100), (103, 100)])
    d = np.stack([_desc(10), _desc(0), _desc(20), _desc(30)])
    q = _queries(pkg, [(101, 100)], 5.0, ur=100.0)
    for ur0, want in ((105.0, [0, -1, -1, -1]), (105.00001, [-1, -1, 0, -1])):
        ur = np.array([ur0, 105.5, -1.0, 0.0], f32)
        assert same_frame(k, d, q, z1, False, ur)[1].tolist() == want
        assert same_points(k, d, q, z1, 0.9, ur)[1].tolist() == want
