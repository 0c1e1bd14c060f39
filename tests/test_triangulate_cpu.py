"""tests/seqref/triangulate.py (the sequential reference of orbhip_create_new_map_points*) on hand-worked cases, the
fp32 Jacobi choice against a float64 SVD, the row-application rule of INTEGRATION.md section 3, and the argument checks
of the two C entries that need no device.  The device checks are in tests/test_triangulate_gpu.py."""
import ctypes as C
import math
import os

import numpy as np

from seqref import triangulate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
KFX, KFY, KCX, KCY, KBF = 718.856, 718.856, 607.1928, 185.2157, 386.1448      # KITTI 00-02
SF = (1.2 ** np.arange(8)).astype(np.float32)
SIGMA2 = (SF * SF).astype(np.float32)
# Largest relative error of x3D (fp32 one-sided Jacobi against np.linalg.svd in float64) over the pairs of the plane scene
# below that take the linear branch.  The pairs are synthetic (plane_pairs: the GPU scene's cameras, plane and key-point
# grid with random octaves, no descriptor search), not the GPU scene's own matches, which need a device to extract.
# Seed 1 (526 pairs) gives 2.11e-6, seed 2 (527 pairs) 2.54e-6.  The constant was set from the seed-1 figure before seed 2
# was run, so the bound is 4x the seed-1 value: 3.3x the larger of the two, tighter than 4x the maximum over both.
JACOBI_SEED1 = 2.11e-6
JACOBI_BOUND = 4 * JACOBI_SEED1


def pose(t, R3=None):
    T = np.zeros((3, 4), f32)
    T[:, :3] = np.eye(3) if R3 is None else R3
    T[:, 3] = t
    return T


def project(cam, T, X):
    Xc = T[:, :3].astype(np.float64) @ np.asarray(X, np.float64) + T[:, 3]
    return float(cam["fx"]) * Xc[0] / Xc[2] + float(cam["cx"]), float(cam["fy"]) * Xc[1] / Xc[2] + float(cam["cy"]), Xc[2]


def kitti():
    return R.make_cam(KFX, KFY, KCX, KCY, KBF, KBF / KFX)


def test_compute_f12_hand_worked():
    """Identity rotations and a sideways baseline b: t12 = t1 - t2 = (b, 0, 0), so F12 = K^-T [t12]x K^-1 is the skew form
    with only F[1,2] = -b/fy and F[2,1] = b/fy ... (cy terms cancel), and x1^T F12 x2 = 0 for two views of one point."""
    cam = kitti()
    b = 0.5
    T1, T2 = pose((b, 0, 0)), pose((0, 0, 0))
    F = R.compute_f12(T1, T2, cam["fx"], cam["fy"], cam["cx"], cam["cy"]).astype(np.float64)
    expect = np.zeros((3, 3))
    expect[1, 2], expect[2, 1] = -b / KFY, b / KFY
    assert np.allclose(F, expect, rtol=1e-5, atol=1e-9)
    for X in ((1.0, -0.5, 8.0), (-3.0, 1.0, 20.0)):
        u1, v1, _ = project(cam, T1, X)
        u2, v2, _ = project(cam, T2, X)
        assert abs(np.array([u1, v1, 1.0]) @ F @ np.array([u2, v2, 1.0])) < 1e-6
        assert abs(v1 - v2) < 1e-9
    ex, ey = R.epipole(T1, T2, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert not np.isfinite(ex)                      # sideways motion: the epipole is at infinity
    T2f = pose((0, 0, -1.0))                        # camera 2 one metre ahead: the epipole is the principal point
    ex, ey = R.epipole(pose((0, 0, 0)), T2f, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert ex == cam["cx"] and ey == cam["cy"]


def test_baseline_gate():
    T1 = pose((0, 0, 0))
    assert R.baseline_gate(T1, pose((0.3, 0, 0)), mb=0.54) and not R.baseline_gate(T1, pose((0.6, 0, 0)), mb=0.54)
    assert R.baseline_gate(T1, pose((0.3, 0, 0)), median_depth=40.0)            # 0.0075 < 0.01
    assert not R.baseline_gate(T1, pose((0.3, 0, 0)), median_depth=20.0)        # 0.015
    assert R.baseline_gate(T1, T1, mb=0.0) is False and R.baseline_gate(T1, T1, median_depth=5.0)


def _pair(cam, T1, T2, X, oct1=0, oct2=0, stereo1=False, stereo2=False, d1=(0, 0), d2=(0, 0), z1=None, z2=None):
    u1, v1, zz1 = project(cam, T1, X)
    u2, v2, zz2 = project(cam, T2, X)
    zz1 = zz1 if z1 is None else z1
    zz2 = zz2 if z2 is None else z2
    p1 = (u1 + d1[0], v1 + d1[1], oct1, u1 + d1[0] - KBF / zz1 if stereo1 else -1.0, zz1 if stereo1 else -1.0)
    p2 = (u2 + d2[0], v2 + d2[1], oct2, u2 + d2[0] - KBF / zz2 if stereo2 else -1.0, zz2 if stereo2 else -1.0)
    return p1, p2


def _status(T1, T2, p1, p2, cam=None):
    return R.triangulate_pair(T1, T2, p1, p2, cam or kitti(), SIGMA2, SF)


def test_every_status_code_from_a_hand_built_pair():
    cam = kitti()
    T1, T2 = pose((0, 0, 0)), pose((-1.0, 0, 0))
    X = (1.0, 0.5, 10.0)
    st, P = _status(T1, T2, *_pair(cam, T1, T2, X))
    assert st == R.CREATED and np.allclose(P, X, rtol=1e-3)
    # monocular, baseline 1 cm at 10 m: cosParallaxRays > 0.9998 (:349)
    Tn = pose((-0.01, 0, 0))
    assert _status(T1, Tn, *_pair(cam, T1, Tn, X))[0] == R.LOW_PARALLAX
    # disparity of the wrong sign (40 px the wrong way): the rays meet 5 m BEHIND both cameras
    p1, p2 = _pair(cam, T1, T2, X)
    p2b = (2 * p1[0] - p2[0], p2[1], 0, -1.0, -1.0)
    st, P = _status(T1, T2, p1, p2b)
    assert st == R.BEHIND_1 and P[2] < -4
    # a point in front of camera 1 and 5 m behind camera 2 (stereo depth of key frame 1 taken for x3D)
    T2b = pose((0, 0, -15.0))
    p1, p2 = _pair(cam, T1, T2b, X, stereo1=True)
    st, P = _status(T1, T2b, p1, (p2[0], p2[1], 0, -1.0, -1.0))
    assert st == R.BEHIND_2 and abs(P[2] - 10.0) < 1e-3
    # reprojection misses of 12 px: x3D from the stereo depth of one key frame, the other key point moved along the
    # epipolar line's normal
    p1, p2 = _pair(cam, T1, T2, X, stereo2=True, d1=(0, 12.0))
    assert _status(T1, T2, p1, p2)[0] == R.REPROJ_1
    # ... and with key point 1 on level 7, whose tolerance (10 px) takes its share of the miss
    p1, p2 = _pair(cam, T1, T2, X, stereo1=True, oct1=7, d2=(0, 12.0))
    assert _status(T1, T2, p1, p2)[0] == R.REPROJ_2
    # scale consistency: same distance, octaves 0 and 7 (ratio 3.58 > 1.5 * 1.2)
    assert _status(T1, T2, *_pair(cam, T1, T2, X, oct1=7, oct2=0))[0] == R.SCALE
    assert _status(T1, T2, *_pair(cam, T1, T2, X, oct1=0, oct2=7))[0] == R.SCALE
    # w == 0 (:333): the cameras one above the other, the key points side by side on one row.  Column 3 of A is
    # (0, -h, 0, h) and stays exactly orthogonal to the others, whose rows 1 and 3 are bitwise equal; the smallest singular
    # value lies in the span of the first three columns, so the null vector has w == 0 exactly.
    Tu, Td = pose((0, 0.5, 0)), pose((0, -0.5, 0))
    pa = (KCX + 3.0, KCY + 2.0, 0, -1.0, -1.0)
    pb = (KCX + 3.0 + 0.03 * KFX, KCY + 2.0, 0, -1.0, -1.0)
    st, P = _status(Tu, Td, pa, pb)
    assert st == R.W_ZERO and not P.any()
    # dist == 0 (:422): x3D is the centre of camera 2 exactly (UnprojectStereo with a vanishing depth).  Its depth in
    # camera 2 is the rounding residual of R2*Ow2 + t2, so reaching the test needs a pose whose residual has z2 > 0 and
    # |x2| much smaller than z2 (the reprojection :405-411 divides by z2), and mbf = 0 (else mbf/z2 fails it): the first
    # such pose of a scan over the rotation angle is taken.
    cam0 = R.make_cam(KFX, KFY, KCX, KCY, 0.0, KBF / KFX)
    seen = set()
    for it in range(4000):
        th = 0.1 + 0.001 * it
        Ry = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]], f32)
        T2z = pose(-(Ry.astype(np.float64) @ np.array([0.7, 0.0, 5.0])), Ry)
        O2 = R.camera_centre(T2z)
        u1, v1, _ = project(cam0, T1, O2.astype(np.float64))
        st, P = _status(T1, T2z, (u1, v1, 0, -1.0, -1.0), (KCX, KCY, 7, KCX, 1e-30), cam0)
        seen.add(st)
        assert np.array_equal(P, O2)
        if st == R.ZERO_DIST:
            break
    assert st == R.ZERO_DIST, seen


def test_stereo_branches_pick_the_smaller_cos_parallax():
    """:340-347 with too little parallax between the rays for the linear method: the key frame whose stereo angle is
    larger (closer depth) gives x3D."""
    cam = kitti()
    T1, T2 = pose((0, 0, 0)), pose((-0.001, 0, 0))
    X = (0.5, 0.2, 6.0)
    p1, p2 = _pair(cam, T1, T2, X, stereo1=True)
    st, P = _status(T1, T2, p1, p2)
    assert st == R.CREATED and np.array_equal(P, R.unproject_stereo(T1, f32(p1[0]), f32(p1[1]), f32(p1[4]), cam))
    p1, p2 = _pair(cam, T1, T2, X, stereo2=True)
    st, P = _status(T1, T2, p1, p2)
    assert st == R.CREATED and np.array_equal(P, R.unproject_stereo(T2, f32(p2[0]), f32(p2[1]), f32(p2[4]), cam))
    # both stereo: only key frame 1's angle is evaluated (:311-314 `else if`), so key frame 1 is chosen
    p1, p2 = _pair(cam, T1, T2, X, stereo1=True, stereo2=True)
    st, P = _status(T1, T2, p1, p2)
    assert st == R.CREATED and np.array_equal(P, R.unproject_stereo(T1, f32(p1[0]), f32(p1[1]), f32(p1[4]), cam))
    assert R.cos_parallax_stereo(0.5372, 6.0) == f32(math.cos(2 * math.atan2(0.5372 / 2, 6.0)))


# ---- the Jacobi choice against a float64 SVD ---------------------------------------------------------------------------
def plane_pairs(seed, n=150):
    """Matched pairs of the construction the GPU scene uses: 376x240 views of a fronto-parallel plane at Z = 10 from
    cameras translated sideways by shift * Z / f (shifts of tests/test_triangulate_gpu.py), key points on the integer /
    level-scaled grid the extractor produces, half of them stereo, 12 % of those with an inconsistent depth."""
    rng = np.random.default_rng(seed)
    fx = fy = 250.0
    cx, cy, Z, mb = 188.0, 120.0, 10.0, 0.09
    cam = R.make_cam(fx, fy, cx, cy, mb * fx, mb)
    T1 = pose((0, 0.5, 0))
    for sx, sy in ((12, 0), (-15, 0), (9, 6), (3, 0)):
        T2 = pose((sx * Z / fx, 0.5 + sy * Z / fy, 0))
        for _ in range(n):
            o1, o2 = int(rng.integers(0, 8)), int(rng.integers(0, 8))
            u, v = rng.uniform(30, 340), rng.uniform(30, 210)
            k1 = (np.round(u / SF[o1]) * SF[o1], np.round(v / SF[o1]) * SF[o1])
            k2 = (np.round((u + sx) / SF[o2]) * SF[o2], np.round((v + sy) / SF[o2]) * SF[o2])

            def side(k):
                if rng.random() >= 0.5:
                    return -1.0, -1.0
                z = Z if rng.random() >= 0.12 else float(rng.choice([2.0, 4.0, 25.0, 60.0]))
                return k[0] - mb * fx / z, z
            yield T1, T2, (k1[0], k1[1], o1) + side(k1), (k2[0], k2[1], o2) + side(k2), cam, SIGMA2, SF


def gates64(T1, T2, p1, p2, cam, sigma2, sf):
    """The same gates evaluated in float64 with np.linalg.svd."""
    c = {k: float(v) for k, v in cam.items()}
    T1, T2 = np.asarray(T1, np.float64).reshape(3, 4), np.asarray(T2, np.float64).reshape(3, 4)
    s1, s2 = p1[3] >= 0, p2[3] >= 0
    xn = [np.array([(p[0] - c["cx"]) / c["fx"], (p[1] - c["cy"]) / c["fy"], 1.0]) for p in (p1, p2)]
    r1, r2 = T1[:, :3].T @ xn[0], T2[:, :3].T @ xn[1]
    cos_rays = r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2))
    cs1 = cs2 = cos_rays + 1
    if s1:
        cs1 = math.cos(2 * math.atan2(c["mb"] / 2, p1[4]))
    elif s2:
        cs2 = math.cos(2 * math.atan2(c["mb"] / 2, p2[4]))
    O = [-T[:, :3].T @ T[:, 3] for T in (T1, T2)]
    if cos_rays < min(cs1, cs2) and cos_rays > 0 and (s1 or s2 or cos_rays < 0.9998):
        A = np.stack([xn[0][0] * T1[2] - T1[0], xn[0][1] * T1[2] - T1[1], xn[1][0] * T2[2] - T2[0], xn[1][1] * T2[2] - T2[1]])
        x = np.linalg.svd(A)[2][3]
        if x[3] == 0:
            return R.W_ZERO
        X = x[:3] / x[3]
    elif s1 and cs1 < cs2:
        X = T1[:, :3].T @ (xn[0] * p1[4]) + O[0]
    elif s2 and cs2 < cs1:
        X = T2[:, :3].T @ (xn[1] * p2[4]) + O[1]
    else:
        return R.LOW_PARALLAX
    for code, T in ((R.BEHIND_1, T1), (R.BEHIND_2, T2)):
        if T[2, :3] @ X + T[2, 3] <= 0:
            return code
    for code, T, p, s in ((R.REPROJ_1, T1, p1, s1), (R.REPROJ_2, T2, p2, s2)):
        Xc = T[:, :3] @ X + T[:, 3]
        u, v = c["fx"] * Xc[0] / Xc[2] + c["cx"], c["fy"] * Xc[1] / Xc[2] + c["cy"]
        e2 = (u - p[0]) ** 2 + (v - p[1]) ** 2
        if s:
            e2 += (u - c["mbf"] / Xc[2] - p[3]) ** 2
        if e2 > (7.8 if s else 5.991) * float(sigma2[p[2]]):
            return code
    d1, d2 = np.linalg.norm(X - O[0]), np.linalg.norm(X - O[1])
    if d1 == 0 or d2 == 0:
        return R.ZERO_DIST
    rf, rd, ro = 1.5 * float(sf[1]), d2 / d1, float(sf[p1[2]]) / float(sf[p2[2]])
    return R.SCALE if rd * rf < ro or rd > ro * rf else R.CREATED


def test_jacobi_against_float64_svd():
    """x3D of the fp32 Jacobi against np.linalg.svd in float64 on the A of every pair that takes the linear branch, and
    the share of pairs whose status differs from the same gates in float64 (at most 2 %).  Most systems stop by the rule
    after 4 or 5 sweeps; about one in twelve never does (its null column is rounding noise, which no relative threshold
    calls orthogonal) and is ended by the cap JACOBI_SWEEPS.  The cap is justified here: with 30 sweeps allowed instead,
    x3D is the same bit for bit in every pair, and it has stopped changing after sweep 3."""
    for seed in (1, 2):
        worst, differ, total, linear, capped, settled = 0.0, 0, 0, 0, 0, 0
        for T1, T2, p1, p2, cam, sig, sf in plane_pairs(seed):
            info = {}
            st, _ = R.triangulate_pair(T1, T2, p1, p2, cam, sig, sf, info)
            total += 1
            differ += st != gates64(T1, T2, p1, p2, cam, sig, sf)
            if not info["linear"]:
                continue
            linear += 1
            A, _, _ = R.triangulation_matrix(T1, T2, p1[:2], p2[:2], cam)
            x, sweeps = R.jacobi_null4(A)
            x30, sweeps30 = R.jacobi_null4(A, 30)
            capped += sweeps30 == 30
            for s in range(1, R.JACOBI_SWEEPS + 1):          # the first sweep count from which x3D is the final one
                xs = R.jacobi_null4(A, s)[0]
                if np.array_equal(xs[:3] / xs[3], x30[:3] / x30[3]):
                    settled = max(settled, s)
                    break
            assert np.array_equal(x[:3] / x[3], x30[:3] / x30[3]), "the sweep cap changes x3D"
            v = np.linalg.svd(A.astype(np.float64))[2][3]
            X, Xr = x[:3].astype(np.float64) / float(x[3]), v[:3] / v[3]
            worst = max(worst, float(np.linalg.norm(X - Xr) / np.linalg.norm(Xr)))
        print("seed %d: %d pairs, %d linear, largest relative error of x3D %.3g, %d statuses differ from float64; "
              "%d never stop by the rule, x3D final after at most %d sweeps" % (seed, total, linear, worst, differ, capped, settled))
        assert 2 * settled <= R.JACOBI_SWEEPS
        assert linear > 0.5 * total
        assert worst <= JACOBI_BOUND
        assert differ <= 0.02 * total


# ---- the row-application rule ------------------------------------------------------------------------------------------
def test_rows_applied_in_order_equal_the_sequential_loop():
    """the reference adds the points of neighbour i before it searches neighbour i + 1.  With
    check_ori = 0 the batch rows (has_point as at call time), filtered in neighbour order, are exactly that."""
    rng = np.random.default_rng(3)
    cam = R.make_cam(250.0, 250.0, 188.0, 120.0, 22.5, 0.09)
    n, Z = 60, 10.0
    shifts = [(0, 0), (12, 0), (-15, 0), (12, 0)]
    kf_index = [1, 2, 1, 3, 2]                       # repeated targets
    base = np.stack([rng.uniform(40, 330, n), rng.uniform(40, 200, n)], 1)
    from orb_slam2_comment_amd.capi import KP_DTYPE
    frames = []
    for sx, sy in shifts:
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"] = np.round(base[:, 0] + sx), np.round(base[:, 1] + sy)
        frames.append(dict(keys=k, n=n, T=pose((sx * Z / 250.0, 0.5, 0)).reshape(12), u_right=None, depth=None))
    has0 = [(rng.random(n) < 0.3).astype(np.uint8) for _ in shifts]

    def searcher(hp):
        # a stand-in for SearchForTriangulation with the properties the rule relies on: queries are independent, a
        # query or a candidate with a map point takes no part; key point i of a frame matches i or its neighbour i ^ 1
        def search(k, f, F12, ex, ey):
            m = np.full(n, -1, np.int32)
            for i in range(n):
                if hp[0][i]:
                    continue
                for j in (i, i ^ 1):
                    if (i + k) % 3 and not hp[f][j]:
                        m[i] = j
                        break
            return m
        return search
    median = [Z] * len(kf_index)
    hp = [h.copy() for h in has0]
    rows = R.create_new_map_points(frames, 0, kf_index, cam, SIGMA2, SF, searcher(hp), median)
    batch = R.apply_rows(rows, hp[0], hp, kf_index)
    seq = sequential_loop(frames, kf_index, cam, searcher, [h.copy() for h in has0], median)
    assert len(seq) > 20 and batch == seq


def sequential_loop(frames, kf_index, cam, searcher, hp, median):
    """The reference: one neighbour at a time, searched once (:283), every CREATED pair given its point (:434-447: the
    second AddMapPoint on one neighbour slot overwrites the first), has_point as the next neighbour's search sees it."""
    seq = []
    for k, f in enumerate(kf_index):
        one = R.create_new_map_points(frames, 0, [f], cam, SIGMA2, SF,
                                      lambda _k, f_, F12, ex, ey: searcher(hp)(k, f_, F12, ex, ey), [median[k]])
        for i in range(frames[0]["n"]):
            j = int(one["matches12"][0, i])
            if j >= 0 and one["status"][0, i] == R.CREATED:
                hp[0][i] = 1
                hp[f][j] = 1
                seq.append((k, i, j))
    return seq


def test_two_queries_of_one_row_on_one_neighbour_slot_both_get_their_point():
    """SearchForTriangulation never sets vbMatched2, so two current key points (one corner found on two pyramid levels, at
    the same pixel) can match the same neighbour slot, and the reference creates a point for each.  The rule marks the
    neighbour slots when a row is finished, so both survive; the repeat of the target then gives nothing."""
    cam = R.make_cam(250.0, 250.0, 188.0, 120.0, 22.5, 0.09)
    n, Z, sx = 8, 10.0, 12
    from orb_slam2_comment_amd.capi import KP_DTYPE
    xs = np.repeat([60.0, 130.0, 210.0, 300.0], 2)
    ys = np.repeat([50.0, 90.0, 140.0, 190.0], 2)
    frames = []
    for s in (0, sx):
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"] = xs + s, ys
        frames.append(dict(keys=k, n=n, T=pose((s * Z / 250.0, 0.5, 0)).reshape(12), u_right=None, depth=None))
    has0 = [np.zeros(n, np.uint8), np.tile(np.array([0, 1], np.uint8), n // 2)]   # the odd neighbour slots are taken

    def searcher(hp):
        def search(k, f, F12, ex, ey):
            m = np.full(n, -1, np.int32)
            for i in range(n):
                if not hp[0][i]:
                    m[i] = next((j for j in (i, i ^ 1) if not hp[f][j]), -1)
            return m
        return search
    kf_index, median = [1, 1], [Z, Z]
    hp = [h.copy() for h in has0]
    rows = R.create_new_map_points(frames, 0, kf_index, cam, SIGMA2, SF, searcher(hp), median)
    assert (rows["status"] == R.CREATED).all() and np.array_equal(rows["matches12"][0], [0, 0, 2, 2, 4, 4, 6, 6])
    batch = R.apply_rows(rows, hp[0], hp, kf_index)
    assert batch == [(0, i, i & ~1) for i in range(n)]
    assert batch == sequential_loop(frames, kf_index, cam, searcher, [h.copy() for h in has0], median)


# ---- the C entries without a device -------------------------------------------------------------------------------------
def test_entries_are_exported_and_refuse_bad_arguments_before_any_device_work():
    from orb_slam2_comment_amd import capi
    from orb_slam2_comment_amd.matcher import make_camera
    import orb_slam2_comment_amd as pkg
    L, p = capi.lib(), capi.ptr
    cam = make_camera(500.0, 500.0, 320.0, 240.0, (0, 0, 640, 480), [1.0, 1.2], mbf=40.0, mb=0.08)
    a = dict(idx=np.zeros(2, np.int32), T=np.zeros((3, 12), f32), k=np.zeros((3, 8), capi.KP_DTYPE),
             d=np.zeros((3, 8, 32), np.uint8), n=np.zeros(3, np.int32), f=np.zeros((3, 8), f32),
             node=np.zeros((3, 8), np.uint32), sig=np.ones(2, f32), m=np.full((2, 8), -7, np.int32),
             nm=np.full(2, -7, np.int32), x=np.full((2, 8, 3), -7, f32), st=np.full((2, 8), 77, np.uint8),
             sk=np.full(2, 77, np.uint8))

    def dev(h, cur=0, K=2, cap=8, ur=True, z=True, med=False, sig=True, node=True):
        return L.orbhip_create_new_map_points_device(
            h, cur, K, p(a["idx"]), C.byref(cam), p(a["T"]), p(a["k"]), p(a["d"]), p(a["n"]), cap, p(a["f"]) if ur else None,
            p(a["f"]) if z else None, p(a["node"]) if node else None, None, p(a["f"]) if med else None, 0, 0,
            p(a["sig"]) if sig else None, p(a["m"]), p(a["nm"]), p(a["x"]), p(a["st"]), p(a["sk"]), None, None)
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    assert dev(None) == capi.E_ARG
    assert dev(h, cur=-1) == capi.E_ARG and dev(h, K=-1) == capi.E_ARG and dev(h, cap=0) == capi.E_ARG
    assert dev(h, z=False) == capi.E_ARG                       # u_right without depth
    assert dev(h, med=True) == capi.E_ARG                      # median depths are the monocular gate
    assert dev(h, ur=False, z=False) == capi.E_ARG             # monocular without median depths
    assert dev(h, sig=False) == capi.E_ARG and dev(h, node=False) == capi.E_ARG
    for levels in (0, 17):
        cam.n_levels = levels
        assert dev(h) == capi.E_ARG
    cam.n_levels = 2
    assert dev(h, cap=4097) == capi.E_CAPACITY and b"4096" in L.orbhip_last_error()
    assert dev(h, K=0) == capi.OK                              # nothing to do, nothing touched
    assert (a["m"] == -7).all() and (a["st"] == 77).all() and (a["sk"] == 77).all() and fake.raw == bytes(4096)
    # host twin
    big = np.zeros(4097, capi.KP_DTYPE)
    v, vb = capi.FrameView(), capi.FrameView()
    vb.n, vb.keys, vb.desc = 4097, p(big), p(np.zeros((4097, 32), np.uint8))
    nodes = np.zeros(4097, np.uint32)
    arr = (C.POINTER(capi.FrameView) * 1)(C.pointer(v))
    tab = (C.c_void_p * 1)(nodes.ctypes.data)

    def host(hh, cur_view, K=1, med=True):
        return L.orbhip_create_new_map_points(hh, C.byref(cur_view), p(nodes), None, None, p(a["T"]), K, arr, tab, None, None,
                                              p(a["T"]), p(a["f"]) if med else None, C.byref(cam), 0, 0, p(a["sig"]),
                                              p(a["m"]), p(a["nm"]), p(a["x"]), p(a["st"]), p(a["sk"]), None, None)
    assert host(None, v) == capi.E_ARG and host(h, v, K=-1) == capi.E_ARG
    assert host(h, v, med=False) == capi.E_ARG                 # monocular views without median depths
    assert host(h, vb) == capi.E_CAPACITY
    assert host(h, v) == capi.OK                               # empty current key frame
    assert (a["m"] == -7).all() and fake.raw == bytes(4096)
    for name in ("CreateNewMapPoints", "CreateNewMapPointsDevice"):
        assert callable(getattr(pkg.ORBmatcher, name))
    assert [capi.NEWPOINT_CREATED, capi.NEWPOINT_NO_MATCH, capi.NEWPOINT_SCALE] == [R.CREATED, R.NO_MATCH, R.SCALE]
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for text in ("int orbhip_create_new_map_points_device(orbhip_matcher *m, int cur, int K,",
                 "int orbhip_create_new_map_points(orbhip_matcher *m,", "src/LocalMapping.cc:207-452", ":536-553",
                 "#define ORBHIP_NEWPOINT_SCALE        9"):
        assert text in hdr
