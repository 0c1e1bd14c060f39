"""The sequential reference (tests/seqref: written from the reference text, independent of the C oracle) against
cases worked by hand and against the oracle, bit for bit.  CPU only.

A disagreement between seqref and the oracle means one of them misreads the reference; the kernels are checked
against seqref in test_seqref_gpu.py."""
import math

import numpy as np
import pytest

from helpers import assert_kps_equal, synth_frame, synth_stereo
from orb_slam2_comment_amd import matcher as M
from seqref import extractor as SX
from seqref import matcher as SM

f32 = np.float32
B640 = (0.0, 0.0, 640.0, 480.0)
SF = SX.tables(1000, 1.2, 8)["scale"]


def _desc(nbits):
    """A descriptor with its first `nbits` bits set: Hamming distance nbits to the zero descriptor."""
    bits = np.zeros(256, np.uint8)
    bits[:nbits] = 1
    return np.packbits(bits)


def _keys(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), SX.KP_DTYPE)
    k["x"], k["y"] = np.asarray(xy, f32).reshape(-1, 2).T
    k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = octave, angle, 31.0, 20.0, -1
    return k


def _frames(oracle, keys, desc, u_right=None, bounds=B640):
    keep = []
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    return SM.Frame(keys, desc, u_right, bounds, SF), oracle.make_frame(keys, desc, u_right, bounds, SF, keep), keep


def _queries(uv, radius, lmin=-1, lmax=-1, angle=0.0, observed=1, ur=-1.0):
    q = np.zeros(len(uv), SM.QUERY_DTYPE)
    q["valid"] = 1
    q["u"], q["v"] = np.asarray(uv, f32).reshape(-1, 2).T
    q["radius"], q["min_level"], q["max_level"], q["ur"], q["angle"], q["observed"] = radius, lmin, lmax, ur, angle, observed
    return q


def _same_frame_search(oracle, S, O, q, qd, taken=None, ori=True):
    n, a = SM.search_by_projection_frame(S, q, qd, taken, ori)
    on, oa = oracle.search_by_projection_frame(O, q, qd, taken, ori)
    assert n == on and np.array_equal(a, oa), (n, on, a, oa)
    return n, a


def _same_points_search(oracle, S, O, q, qd, nnratio, taken=None):
    n, a = SM.search_by_projection_points(S, q, qd, taken, nnratio)
    on, oa = oracle.search_by_projection_points(O, q, qd, taken, nnratio)
    assert n == on and np.array_equal(a, oa), (n, on, a, oa)
    return n, a


def _same_init(oracle, S1, O1, S2, O2, prev, window, nnratio, ori=True):
    n, m12, pm = SM.search_for_initialization(S1, S2, prev, window, nnratio, ori)
    on, om12, opm = oracle.search_for_initialization(O1, O2, prev, window, nnratio, ori)
    assert n == on and np.array_equal(m12, om12) and np.array_equal(pm, opm), (n, on, m12, om12)
    return n, m12


# ---- known answers -------------------------------------------------------------------------------------

def test_seqref_tables_and_pyramid_sizes():
    """src/ORBextractor.cc:410-470 and :1111-1112, the same known answers test_oracle_known_answers pins."""
    t = SX.tables(1000, 1.2, 8)
    assert t["feat"] == [217, 181, 151, 126, 105, 87, 73, 60]
    assert SX.tables(2000, 1.2, 8)["feat"] == [434, 362, 302, 251, 209, 175, 145, 122]
    assert t["umax"] == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert np.array_equal(t["inv_scale"], np.array([1, 0.833333313, 0.694444418, 0.578703642, 0.482253015,
                                                    0.401877522, 0.334897906, 0.279081583], f32))
    assert SX.level_sizes(1241, 376, t["inv_scale"]) == [(1241, 376), (1034, 313), (862, 261), (718, 218), (598, 181),
                                                         (499, 151), (416, 126), (346, 105)]


@pytest.mark.parametrize("seed,t", [(1, 20), (2, 7), (3, 20), (4, 7)])
def test_seqref_fast_cell_matches_bruteforce(seed, t):
    """The vectorised per-cell FAST against the exhaustive segment test of test_oracle_known_answers."""
    from test_oracle_known_answers import _fast_bruteforce
    img = np.ascontiguousarray(synth_frame(seed, 160, 120)[40:78, 60:97])
    assert SX.fast_cell(img, t) == _fast_bruteforce(img, t)


def test_seqref_fast_atan2_edges_and_accuracy(oracle):
    """OpenCV 3.x fastAtan2: within 0.3 degrees, and bit-identical to the oracle at the axes, near 0 / 360 and
    for negative moments (the quadrant flips 180 - a and 360 - a)."""
    L = oracle.lib()
    rng = np.random.default_rng(1)
    pts = [(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (-1.0, 5000.0), (1.0, 5000.0), (-1.0, -5000.0),
           (1.0, -5000.0), (-3.0, 3.0), (3.0, -3.0), (0.0, 0.0), (-0.0, 7.0), (-7.0, -0.0), (12345.0, 12344.0)]
    pts += [tuple(v) for v in (rng.normal(size=(3000, 2)) * 3000).round()]
    for y, x in pts:
        a = SX.fast_atan2(y, x)
        assert a == f32(L.oracle_fast_atan2(y, x)), (y, x)
        if (y, x) != (0.0, 0.0):
            ref = math.degrees(math.atan2(y, x)) % 360
            d = abs(float(a) - ref)
            assert min(d, 360 - d) < 0.3
    assert 359.9 < SX.fast_atan2(-1.0, 5000.0) < 360.0 and SX.fast_atan2(0.0, 1.0) == 0.0


def test_seqref_three_maxima_ties_and_cut(oracle):
    """src/ORBmatcher.cc:1601-1642: strict > keeps the FIRST of equal bins; max2 < 0.1f*max1 drops bins 2 and 3."""
    import ctypes as C
    cases = [([0, 0, 0, 50, 0, 0, 0, 20, 0, 4], (3, 7, -1)),      # 4 < 5.0: third dropped
             ([0, 0, 0, 50, 0, 0, 0, 4], (3, -1, -1)),
             ([5, 5, 5, 5], (0, 1, 2)),                            # ties: first three bins in order
             ([10, 1, 1], (0, 1, 2)),                              # 1 < 0.1f*10 = 1.0 is false: kept
             ([20, 1, 2, 1], (0, 2, -1)),                          # 2 < 2.0 false: kept; 1 < 2.0: dropped
             ([0, 0, 0], (-1, -1, -1)),
             ([7, 0, 0], (0, -1, -1))]
    L = oracle.lib()
    rng = np.random.default_rng(2)
    rand = [(list(rng.integers(0, 6, 30) * rng.integers(0, 2, 30)), None) for _ in range(200)]
    for h, want in cases + rand:
        got = SM.compute_three_maxima(h)
        if want is not None:
            assert got == want, (h, got)
        a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        hh = np.array(h + [0] * (30 - len(h)), np.int32)
        L.oracle_three_maxima(hh.ctypes.data, 30, C.byref(a), C.byref(b), C.byref(c))
        assert (a.value, b.value, c.value) == SM.compute_three_maxima(list(hh)), h


def test_seqref_rotation_bins_hand_worked():
    """:1433-1438: factor = 1.0f/30, round() half away from zero; float products that land exactly on x.5."""
    rb = SM.rotation_bin
    assert rb(0.0, 0.0) == 0 and rb(10.0, 10.0) == 0
    assert rb(np.nextafter(f32(360), f32(0)), 0.0) == 12               # just under 360 -> 11.99999... -> 12
    assert rb(10.0, 20.0) == 12                                        # -10 -> 350 -> 11.67
    assert f32(f32(135.0) * SM.FACTOR) == f32(4.5) and rb(135.0, 0.0) == 5        # exact half: away from zero
    assert f32(f32(255.0) * SM.FACTOR) == f32(8.5) and rb(255.0, 0.0) == 9
    assert rb(np.nextafter(f32(135), f32(0)), 0.0) == 4                # the float below lands under 4.5
    assert rb(15.0, 0.0) == 1 and rb(14.0, 0.0) == 0
    assert max(rb(a, 0.0) for a in np.linspace(0, 359.99, 5000, dtype=f32)) == 12


# ---- extractor against the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,nf", [(320, 240, 500), (640, 360, 1000), (752, 480, 1000)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seqref_extract_equals_oracle(oracle, W, H, nf, seed):
    img = synth_frame(seed, W, H)
    k, d = SX.extract(img, nf, 1.2, 8, 20, 7)
    ok, od = oracle.OracleExtractor(nf, 1.2, 8, 20, 7).extract(img)
    assert_kps_equal(k, ok, "seed %d %dx%d" % (seed, W, H))
    assert np.array_equal(d, od)
    assert len(k) >= 0.95 * nf


def test_seqref_extract_other_arguments_dense_flat_and_angles(oracle):
    """scale 1.5 / 5 levels; white noise (thousands of candidates, the careful octree phase everywhere); a low
    contrast frame that only the per-cell minThFAST retry finds; a flat frame (no keypoints); angles near 0 and
    360 (negative m_01 with positive m_10) occur and agree bit for bit."""
    rng = np.random.default_rng(3)
    cases = [(synth_frame(4, 640, 480), (800, 1.5, 5, 20, 7)),
             (rng.integers(0, 256, (300, 400), dtype=np.uint8), (1500, 1.2, 8, 20, 7)),
             ((128 + rng.integers(-12, 13, (240, 320))).astype(np.uint8), (500, 1.2, 8, 20, 7)),
             (np.full((240, 320), 128, np.uint8), (500, 1.2, 8, 20, 7))]
    angles = []
    for img, args in cases:
        k, d = SX.extract(img, *args)
        ok, od = oracle.OracleExtractor(*args).extract(img)
        assert_kps_equal(k, ok, str(args))
        assert np.array_equal(d, od)
        angles.append(k["angle"])
    assert len(angles[3]) == 0 and len(angles[2]) > 50
    a = np.concatenate(angles)
    assert ((a > 0) & (a < 2)).any() and ((a > 358) & (a < 360)).any()


def test_seqref_octree_equals_oracle_on_the_same_candidates(oracle):
    """DistributeOctTree alone (src/ORBextractor.cc:539-763) on each level's FAST candidates, including quotas far
    below and above the candidate count: the retained indices in list order."""
    L = oracle.lib()
    levels, _ = SX.compute_pyramid(synth_frame(2, 752, 480), SX.tables(2000, 1.2, 8)["inv_scale"])
    for lv in levels[:4]:
        X, Y, R, (x0, x1, y0, y1) = SX.level_candidates(lv, 20, 7)
        x, y, r = (np.array(a, f32) for a in (X, Y, R))
        for N in (5, 60, 434, len(x) + 10):
            out = np.zeros(N + 64 + len(x), np.int32)
            n = L.oracle_distribute_octree(x.ctypes.data, y.ctypes.data, r.ctypes.data, len(x), x0, x1, y0, y1, N,
                                           out.ctypes.data, len(out))
            assert SX.distribute_octree(X, Y, R, x0, x1, y0, y1, N) == out[:n].tolist(), (lv.shape, N)


# ---- matchers against the oracle on synthetic pairs --------------------------------------------------------

@pytest.fixture(scope="module")
def euroc_pair(oracle):
    W, H = 752, 480
    e = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    k1, d1 = e.extract(synth_frame(1, W, H))
    k2, d2 = e.extract(synth_frame(1, W, H, shift_xy=(5, 0)))
    return (W, H), k1, d1, k2, d2, e.tables()["scale"]


def test_seqref_search_for_initialization_equals_oracle(oracle, euroc_pair):
    """configs[4]: 752x480 @2000, windowSize 100, nnratio 0.9 (and 0.6 without the rotation check), two rounds."""
    (W, H), k1, d1, k2, d2, sf = euroc_pair
    b = (0.0, 0.0, float(W), float(H))
    keep = []
    S1, S2 = SM.Frame(k1, d1, None, b, sf), SM.Frame(k2, d2, None, b, sf)
    O1, O2 = oracle.make_frame(k1, d1, None, b, sf, keep), oracle.make_frame(k2, d2, None, b, sf, keep)
    prev = np.stack([k1["x"], k1["y"]], 1).astype(f32)
    for nnratio, ori in ((0.9, True), (0.6, False)):
        n, m12, pm = SM.search_for_initialization(S1, S2, prev, 100, nnratio, ori)
        on, om12, opm = oracle.search_for_initialization(O1, O2, prev, 100, nnratio, ori)
        assert n == on and np.array_equal(m12, om12) and np.array_equal(pm, opm) and n > 50
        n2, m12b, _ = SM.search_for_initialization(S1, S2, pm, 100, nnratio, ori)
        on2, om12b, _ = oracle.search_for_initialization(O1, O2, opm, 100, nnratio, ori)
        assert n2 == on2 and np.array_equal(m12b, om12b)


@pytest.mark.parametrize("th,stereo,fwd,bwd", [(15, False, False, False), (7, True, False, False),
                                               (7, True, True, False), (7, True, False, True)])
def test_seqref_search_by_projection_frame_equals_oracle(oracle, euroc_pair, th, stereo, fwd, bwd):
    """SearchByProjection(CurrentFrame, LastFrame): the host projection prologue builds the queries."""
    (W, H), k1, d1, k2, d2, sf = euroc_pair
    rng = np.random.default_rng(th + 4 * fwd + 8 * bwd)
    b = (0.0, 0.0, float(W), float(H))
    ur = np.where(rng.random(len(k2)) < 0.6, k2["x"] - rng.uniform(2, 60, len(k2)), -1).astype(f32) if stereo else None
    S, O, keep = _frames(oracle, k2, d2, ur, b)
    fx, cx, cy = 718.856, W / 2.0, H / 2.0
    z = rng.uniform(4, 40, len(k1)).astype(f32)
    X = np.stack([(k1["x"] - cx) * z / fx, (k1["y"] - cy) * z / fx, z], 1).astype(f32)
    T = np.eye(4, dtype=f32)
    T[0, 3] = 5 * 15.0 / fx
    q = M.project_last_frame(T, (fx, fx, cx, cy), b, X, k1["octave"], k1["angle"], rng.random(len(k1)) < 0.85,
                             rng.random(len(k1)) < 0.7, sf, th, mbf=386.1448 if stereo else 0.0, bForward=fwd,
                             bBackward=bwd)
    taken = (rng.random(len(k2)) < 0.05).astype(np.uint8)
    for ori in (True, False):
        n, _ = _same_frame_search(oracle, S, O, q, d1, taken, ori)
        assert n > 100
    q2 = q.copy()
    q2["observed"] = 0                          # every slot may be overwritten by later queries (:1428)
    _same_frame_search(oracle, S, O, q2, d1, None, True)


@pytest.mark.parametrize("th,nnratio", [(1, 0.8), (3, 0.8), (5, 0.8), (3, 0.6)])
def test_seqref_search_by_projection_points_equals_oracle(oracle, euroc_pair, th, nnratio):
    (W, H), k1, d1, k2, d2, sf = euroc_pair
    rng = np.random.default_rng(th * 10 + int(nnratio * 100))
    b = (0.0, 0.0, float(W), float(H))
    ur = np.where(rng.random(len(k2)) < 0.5, k2["x"] - rng.uniform(2, 60, len(k2)), -1).astype(f32)
    S, O, keep = _frames(oracle, k2, d2, ur, b)
    nq = len(k1)
    pred = np.clip(k1["octave"] + rng.integers(-1, 2, nq), 0, 7)
    r = np.array([M.RadiusByViewingCos(c) for c in rng.uniform(0.99, 1.0, nq)], f32)
    if th != 1:
        r = r * f32(th)
    q = _queries(np.stack([k1["x"] + 5 + rng.normal(0, 1, nq), k1["y"] + rng.normal(0, 1, nq)], 1), r * sf[pred],
                 pred - 1, pred, ur=0, observed=rng.random(nq) < 0.8)
    q["valid"] = rng.random(nq) < 0.9
    q["ur"] = q["u"] - rng.uniform(2, 60, nq).astype(f32)
    taken = (rng.random(len(k2)) < 0.1).astype(np.uint8)
    n, _ = _same_points_search(oracle, S, O, q, d1, nnratio, taken)
    assert n > 50


@pytest.mark.parametrize("seed,W,H", [(1, 752, 480), (2, 640, 360)])
def test_seqref_compute_stereo_matches_equals_oracle(oracle, seed, W, H):
    left, right = synth_stereo(seed, W, H)
    eL, eR = oracle.OracleExtractor(1000, 1.2, 8, 20, 7), oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    kl, dl = eL.extract(left)
    kr, dr = eR.extract(right)
    lv_l = [np.ascontiguousarray(eL.level_padded(l))[19:-19, 19:-19] for l in range(8)]
    lv_r = [np.ascontiguousarray(eR.level_padded(l))[19:-19, 19:-19] for l in range(8)]
    t = eL.tables()
    mbf = float(f32(386.1448))
    mb = float(f32(386.1448) / f32(718.856))
    n, ur, dp = SM.compute_stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], mbf, mb)
    on, our, odp = oracle.compute_stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], mbf, mb)
    assert n == on and n > 100
    assert np.array_equal(ur, our) and np.array_equal(dp, odp)


# ---- constructed edge inputs: each names the reference line it targets -----------------------------------

def test_edge_window_bounds_grid_cells_and_visiting_order(oracle):
    """src/Frame.cc:373 strict |dx| < r, |dy| < r; :384-385 round() half away from zero for the cell (x = 25 with
    inv 0.1 is exactly 2.5 -> cell 3); :350-358 visiting order (cell column, row, push_back order) decides ties."""
    xy = [(100, 100), (110, 100), (90, 100), (109.99, 100), (100, 110), (100, 90.01)]
    S, O, keep = _frames(oracle, _keys(xy), np.zeros((len(xy), 32), np.uint8))
    got = SM.features_in_area(S, 100.0, 100.0, 10.0)
    assert got.tolist() == oracle.features_in_area(O, 100.0, 100.0, 10.0).tolist()
    assert sorted(got.tolist()) == [0, 3, 5]
    # equal distances: the first candidate in visiting order wins (:1419 strict <)
    xy = [(28, 100), (25, 100), (34.9, 100), (24.9, 100)]        # cells 3, 3, 3, 2
    S, O, keep = _frames(oracle, _keys(xy), np.zeros((4, 32), np.uint8))
    assert [S.pos_in_grid(i)[0] for i in range(4)] == [3, 3, 3, 2]
    assert SM.features_in_area(S, 30.0, 100.0, 10.0).tolist() == [3, 0, 1, 2]
    q = _queries([(30.0, 100.0), (30.0, 100.0)], 10.0, observed=1)
    n, a = _same_frame_search(oracle, S, O, q, np.zeros((2, 32), np.uint8), None, False)
    assert n == 2 and a.tolist() == [1, -1, -1, 0]               # query 0 takes idx 3 (cell 2), query 1 idx 0


def test_edge_queries_on_the_image_bounds(oracle):
    """src/Frame.cc:332-346: the cell range is clamped to [0, 63] x [0, 47] for queries at mnMinX / mnMaxX exactly,
    and a window entirely outside the image returns nothing; :384-389 keys whose cell rounds to 64 (x >= 635 at
    inv 0.1) are not in the grid at all."""
    xy = [(0.5, 0.5), (3, 3), (639.5, 479.5), (634, 474), (320, 0.2), (0.0, 240.0), (640.0, 240.0)]
    S, O, keep = _frames(oracle, _keys(xy), np.zeros((len(xy), 32), np.uint8))
    for (u, v, r) in [(0.0, 0.0, 5.0), (640.0, 480.0, 5.0), (0.0, 480.0, 8.0), (640.0, 0.0, 8.0), (320.0, 0.0, 1.0),
                      (0.0, 240.0, 0.5), (640.0, 240.0, 0.5), (700.0, 240.0, 10.0), (-30.0, 240.0, 10.0)]:
        got = SM.features_in_area(S, u, v, r).tolist()
        assert got == oracle.features_in_area(O, u, v, r).tolist(), (u, v, r)
    assert sorted(SM.features_in_area(S, 0.0, 0.0, 5.0).tolist()) == [0, 1]
    assert SM.features_in_area(S, 640.0, 480.0, 8.0).tolist() == [3]
    assert SM.features_in_area(S, 640.0, 240.0, 0.5).tolist() == []
    assert SM.features_in_area(S, 0.0, 240.0, 0.5).tolist() == [5]
    assert SM.features_in_area(S, 700.0, 240.0, 10.0).tolist() == []


def test_edge_level_windows(oracle):
    """src/Frame.cc:348: bCheckLevels = minLevel > 0 || maxLevel >= 0, so (-1, -1) and (0, -1) take every level,
    (1, -1) drops level 0, (lo, hi) is inclusive."""
    xy = [(100 + 2 * i, 100) for i in range(6)]
    k = _keys(xy, octave=np.array([0, 1, 2, 3, 0, 2]))
    S, O, keep = _frames(oracle, k, np.zeros((6, 32), np.uint8))
    want = {(-1, -1): [0, 1, 2, 3, 4, 5], (0, -1): [0, 1, 2, 3, 4, 5], (1, -1): [1, 2, 3, 5], (2, 2): [2, 5],
            (-1, 1): [0, 1, 4], (0, 0): [0, 4], (3, -1): [3], (4, 7): []}
    for (lo, hi), w in want.items():
        got = SM.features_in_area(S, 105.0, 100.0, 20.0, lo, hi).tolist()
        assert got == oracle.features_in_area(O, 105.0, 100.0, 20.0, lo, hi).tolist()
        assert sorted(got) == w, (lo, hi)


def test_edge_distance_thresholds(oracle):
    """TH_HIGH (src/ORBmatcher.cc:1426, :118): 100 accepted, 101 rejected; TH_LOW (:459): 50 accepted, 51 not."""
    xy = [(100, 100), (200, 100)]
    S, O, keep = _frames(oracle, _keys(xy), np.stack([_desc(100), _desc(101)]))
    q = _queries([(100.0, 100.0), (200.0, 100.0)], 5.0)
    qd = np.zeros((2, 32), np.uint8)
    n, a = _same_frame_search(oracle, S, O, q, qd, None, False)
    assert n == 1 and a.tolist() == [0, -1]
    n, a = _same_points_search(oracle, S, O, q, qd, 0.8)
    assert n == 1 and a.tolist() == [0, -1]
    S2, O2, keep2 = _frames(oracle, _keys(xy), np.stack([_desc(50), _desc(51)]))
    S1, O1, keep1 = _frames(oracle, _keys(xy), qd)
    prev = np.array(xy, f32)
    n, m12 = _same_init(oracle, S1, O1, S2, O2, prev, 10, 0.9, False)
    assert n == 1 and m12.tolist() == [0, -1]


def test_edge_ratio_tests_and_levels(oracle):
    """:120 bestDist > mfNNratio*bestDist2 in float, only when best and second share a level: 30 vs 0.75*40 = 30
    passes, 31 does not; 40 vs 0.8f*50 (= 40.0000006 -> 40.0f) passes; a second best on another level is no
    ratio test at all.  :461 bestDist < (float)bestDist2*mfNNratio: 30 vs 30 fails, 29 passes."""
    def pts(d_best, d_second, lv_best, lv_second, nnratio):
        k = _keys([(100, 100), (102, 100)], octave=np.array([lv_best, lv_second]))
        S, O, keep = _frames(oracle, k, np.stack([_desc(d_best), _desc(d_second)]))
        return _same_points_search(oracle, S, O, _queries([(101.0, 100.0)], 5.0), np.zeros((1, 32), np.uint8),
                                   nnratio)[0]
    assert pts(30, 40, 1, 1, 0.75) == 1 and pts(31, 40, 1, 1, 0.75) == 0
    assert f32(f32(0.8) * f32(50)) == f32(40) and pts(40, 50, 2, 2, 0.8) == 1 and pts(41, 50, 2, 2, 0.8) == 0
    assert pts(39, 40, 1, 2, 0.75) == 1 and pts(39, 40, 2, 2, 0.75) == 0

    def init(d_best, d_second, nnratio):
        S2, O2, k2 = _frames(oracle, _keys([(100, 100), (102, 100)]), np.stack([_desc(d_best), _desc(d_second)]))
        S1, O1, k1 = _frames(oracle, _keys([(101, 100)]), np.zeros((1, 32), np.uint8))
        return _same_init(oracle, S1, O1, S2, O2, np.array([[101, 100]], f32), 10, nnratio, False)[0]
    assert init(30, 40, 0.75) == 0 and init(29, 40, 0.75) == 1
    assert init(40, 50, 0.8) == 0 and init(39, 50, 0.8) == 1


def test_edge_rotation_bins_and_cull(oracle):
    """:1433-1467: 10 matches each at rot 0, 150, 270 (bins 0, 5, 9) hold the three maxima; single matches at the
    exact halves 135.0f -> 4.5 and 255.0f -> 8.5 round away from zero into bins 5 and 9 and survive, the float
    just below 135 (bin 4), rot just under 360 (bin 12) and rot 15 (bin 1) are culled."""
    rots = [0.0] * 10 + [150.0] * 10 + [270.0] * 10
    tests = [135.0, 255.0, float(np.nextafter(f32(135), f32(0))), float(np.nextafter(f32(360), f32(0))), 15.0]
    rots = np.array(rots + tests, f32)
    xy = [(30 + 15 * (i % 38), 30 + 40 * (i // 38)) for i in range(len(rots))]
    k = _keys(xy, angle=f32(20.0))
    S, O, keep = _frames(oracle, k, np.zeros((len(rots), 32), np.uint8))
    q = _queries(xy, 3.0, angle=f32(20.0) + rots)
    q["angle"] = np.array([f32(f32(20.0) + r) for r in rots], f32) % f32(360)
    n, a = _same_frame_search(oracle, S, O, q, np.zeros((len(rots), 32), np.uint8), None, True)
    kept = [i for i in range(len(rots)) if a[i] == i]
    assert kept == list(range(32)) and n == 32
    # the same with the query index order reversed (histogram order is the order of acceptance)
    _same_frame_search(oracle, S, O, q[::-1].copy(), np.zeros((len(rots), 32), np.uint8), None, True)
    # SearchForInitialization's histogram of the same rotations (:475-495)
    prev = np.array(xy, f32)
    S1, O1, keep1 = _frames(oracle, _keys(xy, angle=q["angle"]), np.zeros((len(rots), 32), np.uint8))
    n, m12 = _same_init(oracle, S1, O1, S, O, prev, 3, 0.9, True)
    assert [i for i in range(len(rots)) if m12[i] == i] == list(range(32)) and n == 32


def test_edge_two_unobserved_queries_on_one_slot(oracle):
    """:1403-1406, :1428-1441, :1458-1463: a slot taken by a map point without observations stays open; a second
    query writes it again, both count and both enter the histogram, and culling the first query's bin empties the
    slot the second query holds while the count drops only by one."""
    xy = [(100, 100)] + [(200 + 10 * i, 200) for i in range(12)]
    S, O, keep = _frames(oracle, _keys(xy, angle=f32(0)), np.zeros((13, 32), np.uint8))
    uv = [(100.0, 100.0), (100.0, 100.0)] + [(200.0 + 10 * i, 200.0) for i in range(12)]
    q = _queries(uv, 3.0, angle=f32(0), observed=0)
    q["angle"][0] = 300.0                        # bin 10: a single entry, culled
    qd = np.zeros((14, 32), np.uint8)
    n, a = _same_frame_search(oracle, S, O, q, qd, None, True)
    assert a[0] == -1 and n == 13                # 14 accepted, one culled entry; slot 0 emptied although query 1 held it
    n, a = _same_frame_search(oracle, S, O, q, qd, None, False)
    assert a[0] == 1 and n == 14                 # without the rotation check the last writer holds the slot
    q["observed"][0] = 1                         # an observed first query blocks the slot for query 1
    n, a = _same_frame_search(oracle, S, O, q, qd, None, False)
    assert a[0] == 0 and n == 13


def test_edge_stereo_consistency_gate(oracle):
    """:1407-1413 and :91-96: the ur gate applies only where mvuRight > 0, and er == radius passes (er > r skips)."""
    xy = [(100, 100), (101, 100), (102, 100), (103, 100)]
    ur = np.array([105.0, 105.5, -1.0, 0.0], f32)            # er = 5 (gate passes), 5.5 (skipped), no gate, no gate
    desc = np.stack([_desc(10), _desc(0), _desc(20), _desc(30)])
    S, O, keep = _frames(oracle, _keys(xy), desc, ur)
    q = _queries([(101.0, 100.0)], 5.0, ur=100.0)
    n, a = _same_frame_search(oracle, S, O, q, np.zeros((1, 32), np.uint8), None, False)
    assert a.tolist() == [0, -1, -1, -1]
    n, a = _same_points_search(oracle, S, O, q, np.zeros((1, 32), np.uint8), 0.9)
    assert a.tolist() == [0, -1, -1, -1]
    ur[0] = 105.00001                                        # er just above the radius: key 0 skipped
    S, O, keep = _frames(oracle, _keys(xy), desc, ur)
    n, a = _same_frame_search(oracle, S, O, q, np.zeros((1, 32), np.uint8), None, False)
    assert a.tolist() == [-1, -1, 0, -1]


def test_edge_stereo_disparity_range_and_window_edges(oracle):
    """src/Frame.cc:516-538 uR in [uL - maxD, uL] inclusive; :573-576 windows that would leave the right level are
    rejected (endu >= cols); :594-595 a SAD minimum on the +-5 edge is rejected; :612-618 disparity < maxD and the
    clamp of a disparity <= 0 to 0.01."""
    rng = np.random.default_rng(8)
    H, W = 120, 200
    tex = rng.integers(0, 256, (H, W + 64)).astype(np.int32)
    tex = ((tex + np.roll(tex, 1, 1) + np.roll(tex, 1, 0)) // 3).astype(np.uint8)

    def run(shift, pairs):
        left = np.ascontiguousarray(tex[:, 32:32 + W])
        right = np.ascontiguousarray(np.clip(tex[:, 32 + shift:32 + shift + W].astype(int) + rng.integers(-2, 3, (H, W)),
                                             0, 255).astype(np.uint8))
        lv_l = [left] + [left[:60, :100]] * 7
        lv_r = [right] + [right[:60, :100]] * 7
        kl = _keys([(u, v) for (u, v, _) in pairs])
        kr = _keys([(ur_, v) for (_, v, ur_) in pairs])
        d = np.zeros((len(pairs), 32), np.uint8)
        args = (kl, d, kr, d, lv_l, lv_r, SF, (f32(1) / SF).astype(f32), 40.0, 1.0)      # maxD = 40
        n, ur, dp = SM.compute_stereo_matches(*args)
        on, our, odp = oracle.compute_stereo_matches(*args)
        assert n == on and np.array_equal(ur, our) and np.array_equal(dp, odp)
        return ur
    # true disparity 20: candidates at the range edges and just outside
    ur = run(20, [(100.0, 20.0, 80.0), (60.0, 35.0, 20.0), (140.0, 50.0, 140.5), (120.0, 65.0, 79.5),
                   (100.0, 80.0, 80.0), (150.0, 95.0, 130.0)])
    assert ur[2] == -1 and ur[3] == -1 and (ur[[0, 4, 5]] > 0).all()
    # true disparity 3, right keypoints at uR == uL (inside the range, :538 <=) and within 11 px of the right
    # edge of the level, where the window does not fit
    ur = run(3, [(W - 12.0, 20.0, W - 12.0), (W - 11.0, 40.0, W - 11.0), (100.0, 60.0, 100.0), (60.0, 80.0, 60.0)])
    assert ur[1] == -1 and ur[0] > 0 and (ur[2:] > 0).all()
    # a shift of 7 px puts the SAD minimum beyond the +-5 search: rejected at the edge
    ur = run(7, [(100.0, 30.0, 100.0), (80.0, 60.0, 80.0), (120.0, 90.0, 120.0)])
    assert (ur == -1).all()
