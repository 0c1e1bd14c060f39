"""orbhip_create_new_map_points_device / orbhip_create_new_map_points (LocalMapping::CreateNewMapPoints for the current
key frame and K neighbours in one call) against tests/seqref/triangulate.py with a search_for_triangulation run pair by
pair, the oracle's or, in the *_with_the_sequential_search tests, that of tests/seqref/bow.py: F12, epipole, gate,
matches, status codes and 3-D points bit-identical, row by row.

The scene: one extraction batch of 7 frames at 376x240, 500 features.  A uniform image shift s is a fronto-parallel plane at
depth Z seen from a camera translated sideways by s*Z/f, so with identity rotations the matched pairs really triangulate
onto the plane.  Rows: 0 the current key frame, 1-4 shifted views (row 4 by 3 px only: monocular pairs have too little
parallax), 5 an unshifted copy (zero baseline: the gate skips it), 6 blank (n == 0).  Rows 7 and 8 are written by hand,
one key point each, because cameras that differ by a sideways translation only cannot produce two of the codes:
row 7 copies a key point of the current frame 6.5 px to the side although its camera sits straight below the current
one, which gives the 4x4 system an exact null vector with w == 0 (ORBHIP_NEWPOINT_W_ZERO); row 8 copies a stereo key
point of the current frame into a camera 15 m ahead, beyond the plane, so the point unprojected from the current key
frame lies in front of camera 1 and behind camera 2 (ORBHIP_NEWPOINT_BEHIND_2; with equal tz, z1 == z2 always).
Row 9, also by hand, is a camera 30 px to the side holding four copies of current key points that fail one gate each by
a wide margin, so that no code depends on which false matches the extraction happens to produce: moved the wrong way
(BEHIND_1), five pyramid levels up (SCALE), with a right coordinate for depth 2 instead of 10 on either side (REPROJ_2,
REPROJ_1: 9 px).

ORBHIP_NEWPOINT_ZERO_DIST cannot be reached through the search: dist == 0 needs x3D equal to a camera centre, whose depth
in that camera is R*Ow + t = 0 up to rounding, which the z <= 0 tests or, failing those, the reprojection tests (1/z)
catch first; and a key point whose ray passes through the other camera centre has no epipolar line (den ~ 0).  It is
produced by a hand-built pair on the sequential reference in tests/test_triangulate_cpu.py; here the other nine codes are
asserted to occur."""
import numpy as np
import pytest

from helpers import make_vocabulary, synth_frame, write_vocabulary
from seqref import bow as SB
from seqref import triangulate as R

pytestmark = pytest.mark.gpu

W, H, NF = 376, 240, 500
FX = FY = 250.0
CX, CY = 188.0, 120.0
Z, MB = 10.0, 0.09
MBF = MB * FX
SHIFTS = [(0, 0), (12, 0), (-15, 0), (9, 6), (3, 0), (0, 0), None]   # None: blank
CUR, COPY, BLANK, HAND, HAND2, HAND3 = 0, 5, 6, 7, 8, 9
KF_INDEX = [3, 1, HAND, 1, 4, BLANK, CUR, HAND3, COPY, HAND2, 2]   # a repeat, a gap, the blank row and cur itself
HAND_ROWS = (HAND, HAND2, HAND3)
SIDE = 30                                                # px, the sideways camera of row 9
T_CUR = (0.0, 0.5, 0.0)
SENT = -77


def _T(t):
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = np.eye(3, dtype=np.float32)
    T[:, 3] = t
    return T.reshape(12)


def build_scene(pkg, kd, node, sf, seed=11):
    rng = np.random.default_rng(seed)
    B = len(SHIFTS) + len(HAND_ROWS)
    S = dict(sf=np.asarray(sf, np.float32), B=B)
    S["sigma2"] = (S["sf"] * S["sf"]).astype(np.float32)
    S["cam"] = pkg.matcher.make_camera(FX, FY, CX, CY, (0.0, 0.0, float(W), float(H)), sf, mbf=MBF, mb=MB)
    S["rcam"] = R.make_cam(FX, FY, CX, CY, MBF, MB)
    T = []
    for s in SHIFTS:
        sx, sy = s if s is not None else (40, 0)
        T.append(_T((T_CUR[0] + sx * Z / FX, T_CUR[1] + sy * Z / FY, T_CUR[2])))
    T.append(_T((0.0, -T_CUR[1], 0.0)))
    T.append(_T((T_CUR[0], T_CUR[1], -15.0)))
    T.append(_T((T_CUR[0] + SIDE * Z / FX, T_CUR[1], T_CUR[2])))
    S["T"] = np.stack(T).astype(np.float32)
    keys, desc, nodes, ur, depth, hp = [], [], [], [], [], []
    for f in range(len(SHIFTS)):
        k, d = kd[f]
        n = len(k)
        stereo = rng.random(n) < 0.5
        u = np.where(stereo, k["x"] - np.float32(MBF / Z), -1).astype(np.float32)
        z = np.where(stereo, Z, -1).astype(np.float32)
        bad = stereo & (rng.random(n) < 0.12)        # inconsistent depth: reprojection and scale failures
        zb = rng.choice([2.0, 4.0, 25.0, 60.0], n).astype(np.float32)
        z = np.where(bad, zb, z)
        u = np.where(bad, k["x"] - np.float32(MBF) / zb, u).astype(np.float32)
        keys.append(k); desc.append(d); nodes.append(node[f]); ur.append(u); depth.append(z)
        hp.append((rng.random(n) < 0.3).astype(np.uint8))
    # the hand-written row: one stereo key point at octave 7, 6.5 px to the side of a free monocular key point of cur
    k0 = keys[CUR]
    free = np.nonzero((hp[CUR] == 0) & (ur[CUR] < 0) & (nodes[CUR] != pkg.capi.NO_NODE))[0]
    i0 = int(free[np.argmin((k0["x"][free] - CX) ** 2 + (k0["y"][free] - CY) ** 2)])
    kh = k0[i0:i0 + 1].copy()
    kh["x"] += np.float32(6.5)
    kh["octave"] = 7
    keys.append(kh); desc.append(desc[CUR][i0:i0 + 1].copy()); nodes.append(nodes[CUR][i0:i0 + 1].copy())
    ur.append((kh["x"] - np.float32(MBF / Z)).astype(np.float32)); depth.append(np.full(1, Z, np.float32))
    hp.append(np.zeros(1, np.uint8))
    # the second one: a free stereo key point of cur with the plane's depth, seen unchanged from 15 m ahead (monocular there)
    free = np.nonzero((hp[CUR] == 0) & (depth[CUR] == np.float32(Z)) & (nodes[CUR] != pkg.capi.NO_NODE))[0]
    i1 = int(free[0])
    keys.append(k0[i1:i1 + 1].copy()); desc.append(desc[CUR][i1:i1 + 1].copy()); nodes.append(nodes[CUR][i1:i1 + 1].copy())
    ur.append(np.full(1, -1, np.float32)); depth.append(np.full(1, -1, np.float32)); hp.append(np.zeros(1, np.uint8))
    # the third one: four copies, each failing one gate
    used = {i0, i1}

    def pick(mask):
        free = [int(i) for i in np.nonzero((hp[CUR] == 0) & (nodes[CUR] != pkg.capi.NO_NODE) & mask)[0] if int(i) not in used]
        used.add(free[0])
        return free[0]
    low = k0["octave"] <= 2
    inside = (k0["x"] > SIDE + 20) & (k0["x"] < W - SIDE - 20)
    i2 = pick((ur[CUR] < 0) & inside)                                # BEHIND_1
    i3 = pick((ur[CUR] < 0) & low & inside)                          # SCALE
    i4 = pick((depth[CUR] == np.float32(Z)) & low & inside)          # REPROJ_2
    i5 = pick((ur[CUR] >= 0) & low & inside)                         # REPROJ_1: its own depth is made inconsistent
    depth[CUR][i5] = 2.0
    ur[CUR][i5] = k0["x"][i5] - np.float32(MBF) / np.float32(2.0)
    kh = k0[[i2, i3, i4, i5]].copy()
    kh["x"] += np.array([-SIDE, SIDE, SIDE, SIDE], np.float32)
    kh["octave"][1] += 5
    keys.append(kh); desc.append(desc[CUR][[i2, i3, i4, i5]].copy()); nodes.append(nodes[CUR][[i2, i3, i4, i5]].copy())
    ur.append(np.array([-1, -1, kh["x"][2] - np.float32(MBF) / np.float32(2.0), -1], np.float32))
    depth.append(np.array([-1, -1, 2.0, -1], np.float32)); hp.append(np.zeros(4, np.uint8))
    S["hand3"] = {i2: R.BEHIND_1, i3: R.SCALE, i4: R.REPROJ_2, i5: R.REPROJ_1}
    S.update(keys=keys, desc=desc, node=nodes, ur=ur, depth=depth, hp=hp, i0=i0, i1=i1, n=[len(k) for k in keys])
    return S


class Run:
    def __init__(self, env):
        self.env = env
        self.pair_cache = {}

    def frames(self, mono, n_cur=None):
        S = self.env["S"]
        fr = []
        for f in range(S["B"]):
            n = S["n"][f] if (f != CUR or n_cur is None) else n_cur
            fr.append(dict(keys=S["keys"][f][:n], n=n, T=S["T"][f], u_right=None if mono else S["ur"][f][:n],
                           depth=None if mono else S["depth"][f][:n]))
        return fr

    def expected(self, kf_index, mono, only_stereo, check_ori, median=None, n_cur=None, search_from="oracle"):
        """seqref rows; the search is the unchanged oracle's, or (search_from="seqref") tests/seqref/bow.py's, called per
        pair with the seqref's F12 and epipole"""
        S, O = self.env["S"], self.env["O"]
        fr = self.frames(mono, n_cur)
        n1 = fr[CUR]["n"]
        bounds = (0.0, 0.0, float(W), float(H))

        def view(f, n, keep):
            return O.make_frame(S["keys"][f][:n], S["desc"][f][:n], None if mono else S["ur"][f][:n], bounds, S["sf"], keep)

        def search(k, f, F12, ex, ey):
            n2 = fr[f]["n"]
            if n1 == 0 or n2 == 0:
                return np.full(n1, -1, np.int32)
            keep = []
            o1, o2 = view(CUR, n1, keep), view(f, n2, keep)
            nm, m12 = O.search_for_triangulation(o1, S["node"][CUR][:n1], 1 - S["hp"][CUR][:n1], o2, S["node"][f][:n2],
                                                 1 - S["hp"][f][:n2], F12, float(ex), float(ey), S["sigma2"], only_stereo,
                                                 check_ori)
            return m12

        def search_seqref(k, f, F12, ex, ey):
            n2 = fr[f]["n"]
            if n1 == 0 or n2 == 0:
                return np.full(n1, -1, np.int32)
            nm, m12 = SB.search_for_triangulation(
                S["keys"][CUR][:n1], S["desc"][CUR][:n1], S["node"][CUR][:n1], 1 - S["hp"][CUR][:n1],
                None if mono else S["ur"][CUR][:n1], S["keys"][f][:n2], S["desc"][f][:n2], S["node"][f][:n2], 1 - S["hp"][f][:n2],
                None if mono else S["ur"][f][:n2], F12, ex, ey, S["sigma2"], S["sf"], only_stereo, check_ori)
            return m12
        key = (tuple(kf_index), mono, only_stereo, check_ori, n_cur, search_from)
        if key not in self.pair_cache:
            self.pair_cache[key] = R.create_new_map_points(fr, CUR, kf_index, S["rcam"], S["sigma2"], S["sf"],
                                                           search if search_from == "oracle" else search_seqref, median)
        return self.pair_cache[key]

    def device(self, kf_index, mono, only_stereo, check_ori, median=None, n_cur=None, cap=None, cur=CUR, f12=True):
        env = self.env
        t, D, S = env["torch"], env["D"], env["S"]
        K = len(kf_index)
        cap = D["cap"] if cap is None else cap
        d_n = D["n"]
        if n_cur is not None:
            d_n = D["n"].clone()
            d_n[CUR] = n_cur
        d_idx = t.tensor(kf_index if K else [0], dtype=t.int32, device=D["dev"])
        d_med = t.tensor(median, dtype=t.float32, device=D["dev"]) if median is not None else 0
        out = dict(m12=t.full((max(K, 1), cap), SENT, dtype=t.int32, device=D["dev"]),
                   nm=t.full((max(K, 1),), SENT, dtype=t.int32, device=D["dev"]),
                   x3d=t.full((max(K, 1), cap, 3), float(SENT), dtype=t.float32, device=D["dev"]),
                   st=t.full((max(K, 1), cap), 200, dtype=t.uint8, device=D["dev"]),
                   sk=t.full((max(K, 1),), 200, dtype=t.uint8, device=D["dev"]),
                   f12=t.full((max(K, 1), 9), float(SENT), dtype=t.float32, device=D["dev"]),
                   ep=t.full((max(K, 1), 2), float(SENT), dtype=t.float32, device=D["dev"]))
        t.cuda.synchronize()
        m = env["m1"] if check_ori else env["m0"]
        m.CreateNewMapPointsDevice(cur, K, d_idx, S["cam"], D["T"], D["k"], D["d"], d_n, cap, D["node"], S["sigma2"],
                                   out["m12"], out["nm"], out["x3d"], out["st"], out["sk"],
                                   d_u_right=0 if mono else D["ur"], d_depth=0 if mono else D["z"], d_has_point=D["hp"],
                                   d_median_depth=d_med, bOnlyStereo=only_stereo, d_f12=out["f12"] if f12 else 0,
                                   d_epipole=out["ep"] if f12 else 0)
        m.sync()
        return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(got, exp, n1, K):
    assert np.array_equal(got["sk"][:K], exp["skipped"])
    assert np.array_equal(bits(got["f12"][:K].reshape(K, 3, 3)), bits(exp["f12"]))
    assert np.array_equal(got["ep"][:K], exp["epipole"], equal_nan=True)
    assert np.array_equal(got["m12"][:K, :n1], exp["matches12"])
    assert np.array_equal(got["nm"][:K], exp["nmatches"])
    assert np.array_equal(got["st"][:K, :n1], exp["status"]), np.nonzero(got["st"][:K, :n1] != exp["status"])
    assert np.array_equal(bits(got["x3d"][:K, :n1]), bits(exp["x3d"]))
    # entries >= n[cur] are untouched
    assert (got["m12"][:, n1:] == SENT).all() and (got["st"][:, n1:] == 200).all() and (got["x3d"][:, n1:] == SENT).all()


@pytest.fixture(scope="module")
def env(oracle, tmp_path_factory):
    return make_env(tmp_path_factory.mktemp("voc"), oracle)


def make_env(voc_dir, oracle=None):
    import torch
    import orb_slam2_comment_amd as pkg
    dev = torch.device("cuda:0")
    ext = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    cap = ext.capacity(H, W)
    B0 = len(SHIFTS)
    imgs = np.stack([np.full((H, W), 127, np.uint8) if s is None else synth_frame(41, W, H, shift_xy=s) for s in SHIFTS])
    B = B0 + len(HAND_ROWS)
    d_img = torch.from_numpy(imgs).to(dev)
    d_k = torch.zeros((B, cap, 28), dtype=torch.uint8, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    d_node = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
    voc = make_vocabulary(10, 4, seed=5)
    gv = pkg.ORBVocabulary()
    assert gv.loadFromTextFile(write_vocabulary(voc_dir / "voc.txt", voc))
    gv.set_stream(ext.stream())
    ext.extract_batch_device(d_img.data_ptr(), B0, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    scratch = [torch.zeros((B0, cap), dtype=dt, device=dev) for dt in (torch.int32, torch.float64, torch.int32, torch.float64)]
    d_nb = torch.zeros(B0, dtype=torch.int32, device=dev)
    gv.transform_device(B0, d_d.data_ptr(), d_n.data_ptr(), cap, 2, scratch[0].data_ptr(), scratch[1].data_ptr(),
                        d_node.data_ptr(), scratch[2].data_ptr(), scratch[3].data_ptr(), d_nb.data_ptr())
    gv.sync()
    gv.set_stream(0)
    n = d_n.cpu().numpy()
    hk = d_k.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)
    hd = d_d.cpu().numpy()
    hn = d_node.cpu().numpy().view(np.uint32)
    assert n[BLANK] == 0 and all(n[f] > 300 for f in range(B0) if f != BLANK) and cap > n.max()
    kd = [(hk[f, :n[f]].copy(), hd[f, :n[f]].copy()) for f in range(B0)]
    S = build_scene(pkg, kd, [hn[f, :n[f]].copy() for f in range(B0)], ext.GetScaleFactors())

    def rows(parts, dt, fill, tail=()):
        a = np.full((B, cap) + tail, fill, dt)
        for f, p in enumerate(parts):
            a[f, :len(p)] = p
        return torch.from_numpy(a).to(dev)
    # the extracted rows stay as the extractor wrote them; the hand-written rows are added behind them
    for r in HAND_ROWS:
        nr = S["n"][r]
        d_k[r, :nr] = torch.from_numpy(S["keys"][r].view(np.uint8).reshape(nr, 28)).to(dev)
        d_d[r, :nr] = torch.from_numpy(S["desc"][r]).to(dev)
        d_n[r] = nr
        d_node[r, :nr] = torch.from_numpy(S["node"][r].view(np.int32)).to(dev)
    D = dict(k=d_k, d=d_d, n=d_n, node=d_node, cap=cap, dev=dev, T=torch.from_numpy(S["T"]).to(dev),
             ur=rows(S["ur"], np.float32, -1.0), z=rows(S["depth"], np.float32, -1.0), hp=rows(S["hp"], np.uint8, 1))
    e = dict(pkg=pkg, O=oracle, S=S, D=D, torch=torch, m0=pkg.ORBmatcher(0.6, False), m1=pkg.ORBmatcher(0.6, True))
    e["run"] = Run(e)
    return e


@pytest.mark.parametrize("only_stereo,check_ori", [(False, False), (True, False), (False, True)])
def test_stereo_rows_equal_the_sequential_reference(env, only_stereo, check_ori):
    run, S = env["run"], env["S"]
    exp = run.expected(KF_INDEX, False, only_stereo, check_ori)
    got = run.device(KF_INDEX, False, only_stereo, check_ori)
    compare(got, exp, S["n"][CUR], len(KF_INDEX))
    sk = dict(zip(KF_INDEX, exp["skipped"]))
    assert sk[COPY] == 1 and sk[CUR] == 1 and sk[1] == 0 and sk[BLANK] == 0
    assert exp["nmatches"][KF_INDEX.index(BLANK)] == 0
    assert np.array_equal(exp["matches12"][1], exp["matches12"][3])          # the repeated key frame
    if not only_stereo and not check_ori:
        assert exp["nmatches"].sum() > 150
        seen = set(np.unique(exp["status"]).tolist())
        assert seen >= set(range(10)) - {R.ZERO_DIST}, seen                  # see the module docstring for ZERO_DIST
        assert exp["status"][KF_INDEX.index(HAND), S["i0"]] == R.W_ZERO
        assert exp["status"][KF_INDEX.index(HAND2), S["i1"]] == R.BEHIND_2
        for i, code in S["hand3"].items():
            assert exp["status"][KF_INDEX.index(HAND3), i] == code, (i, code)
        created = exp["status"] == R.CREATED
        assert created.sum() > 50 and np.median(np.abs(exp["x3d"][created][:, 2] - Z)) < 0.1 * Z   # onto the plane


@pytest.mark.parametrize("only_stereo,check_ori", [(False, True), (True, False)])
def test_stereo_rows_with_the_sequential_search(env, only_stereo, check_ori):
    """The same rows with tests/seqref/bow.py's SearchForTriangulation in the oracle's place: nothing of the expected
    values comes from the oracle."""
    run, S = env["run"], env["S"]
    exp = run.expected(KF_INDEX, False, only_stereo, check_ori, search_from="seqref")
    got = run.device(KF_INDEX, False, only_stereo, check_ori)
    compare(got, exp, S["n"][CUR], len(KF_INDEX))
    assert exp["nmatches"].sum() > (150 if not only_stereo else 20)


def test_monocular_rows_with_the_sequential_search(env):
    run, S = env["run"], env["S"]
    median = [Z] * len(KF_INDEX)
    exp = run.expected(KF_INDEX, True, False, False, median, search_from="seqref")
    got = run.device(KF_INDEX, True, False, False, median)
    compare(got, exp, S["n"][CUR], len(KF_INDEX))
    assert (exp["status"] == R.CREATED).sum() > 30


def test_rows_equal_todays_single_pair_search(env):
    pkg, S = env["pkg"], env["S"]
    got = env["run"].device(KF_INDEX, False, False, True)
    bounds = (0.0, 0.0, float(W), float(H))
    n1 = S["n"][CUR]
    g1 = pkg.FrameView(S["keys"][CUR], S["desc"][CUR], S["sf"], bounds, S["ur"][CUR])
    for k, f in enumerate(KF_INDEX):
        if got["sk"][k] or S["n"][f] == 0:
            assert got["nm"][k] == 0 and (got["m12"][k, :n1] == -1).all()
            continue
        g2 = pkg.FrameView(S["keys"][f], S["desc"][f], S["sf"], bounds, S["ur"][f])
        nm, m12 = env["m1"].SearchForTriangulation(g1, S["node"][CUR], 1 - S["hp"][CUR], g2, S["node"][f], 1 - S["hp"][f],
                                                   got["f12"][k], got["ep"][k], S["sigma2"], False)
        assert nm == got["nm"][k] and np.array_equal(m12, got["m12"][k, :n1]), k


def test_monocular_rows(env):
    run, S = env["run"], env["S"]
    median = [Z] * len(KF_INDEX)
    median[1] = 1000.0                         # baseline / median < 0.01: skipped although the baseline is fine
    exp = run.expected(KF_INDEX, True, False, False, median)
    got = run.device(KF_INDEX, True, False, False, median)
    compare(got, exp, S["n"][CUR], len(KF_INDEX))
    assert exp["skipped"][1] == 1 and exp["skipped"][3] == 0 and exp["skipped"][KF_INDEX.index(COPY)] == 1
    assert (exp["status"] == R.LOW_PARALLAX).any() and (exp["status"] == R.CREATED).sum() > 30


@pytest.mark.parametrize("n_cur", [1, 333])
def test_odd_counts(env, n_cur):
    """n[cur] = 1, and a count that is a multiple of neither 4 nor 64"""
    run = env["run"]
    assert env["S"]["n"][CUR] > 333
    kf = [1, 3, HAND, HAND2, HAND3]
    exp = run.expected(kf, False, False, False, n_cur=n_cur)
    got = run.device(kf, False, False, False, n_cur=n_cur)
    compare(got, exp, n_cur, len(kf))


def test_host_twin_equals_the_device_call(env):
    pkg, S = env["pkg"], env["S"]
    bounds = (0.0, 0.0, float(W), float(H))
    views = [pkg.FrameView(S["keys"][f], S["desc"][f], S["sf"], bounds, S["ur"][f]) for f in range(S["B"])]
    for check_ori in (False, True):
        got = env["run"].device(KF_INDEX, False, False, check_ori)
        m = env["m1"] if check_ori else env["m0"]
        h = m.CreateNewMapPoints(views[CUR], S["node"][CUR], S["hp"][CUR], S["depth"][CUR], S["T"][CUR].reshape(3, 4),
                                 [views[f] for f in KF_INDEX], [S["node"][f] for f in KF_INDEX],
                                 [S["hp"][f] for f in KF_INDEX], [S["depth"][f] for f in KF_INDEX],
                                 np.stack([S["T"][f].reshape(3, 4) for f in KF_INDEX]), S["cam"], S["sigma2"])
        K, n1 = len(KF_INDEX), S["n"][CUR]
        assert np.array_equal(h["matches12"], got["m12"][:, :n1]) and np.array_equal(h["nmatches"], got["nm"])
        assert np.array_equal(h["status"], got["st"][:, :n1]) and np.array_equal(h["skipped"], got["sk"])
        assert np.array_equal(bits(h["x3d"]), bits(got["x3d"][:, :n1]))
        assert np.array_equal(bits(h["f12"]).reshape(K, 9), bits(got["f12"]))
        assert np.array_equal(h["epipole"], got["ep"], equal_nan=True)


def test_limits_and_empty_calls(env):
    pkg, run, S = env["pkg"], env["run"], env["S"]
    with pytest.raises(pkg.OrbHipError) as e:
        run.device(KF_INDEX, False, False, False, cap=4097)
    assert e.value.code == pkg.capi.E_CAPACITY
    for kf, cur in (([], CUR), (KF_INDEX, BLANK)):          # K == 0; an empty current key frame: nothing is written
        got = run.device(kf, False, False, False, cur=cur)
        assert (got["m12"] == SENT).all() and (got["nm"] == SENT).all() and (got["st"] == 200).all()
        assert (got["sk"] == 200).all() and (got["x3d"] == SENT).all() and (got["f12"] == SENT).all()
