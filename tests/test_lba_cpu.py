"""The sequential reference of Optimizer::LocalBundleAdjustment (tests/seqref/lba.py) on its own: hand-worked cases for the
rules it pins, the distance to a textbook restatement (full normal equations without Schur, rotation matrices,
numpy.linalg.solve, libm), a host build of orbhip_lba_core.h that must match it bit for bit, and the cases the GPU tests
replay (test_lba_gpu.py imports them from here; the reference answers are computed once per process).

Measured on the CPU (the asserted tolerances are four times the maxima), against the textbook restatement with the erase
lists equal; pose = max entry of R and of t (m), point = max coordinate (m), all in double before the write-back:
  scene S      R 2.8e-12  t 8.6e-12  X 1.1e-11        scene S, monocular  R 1.2e-14  t 1.5e-13  X 1.8e-13
  scene M      R 5.6e-16  t 8.9e-15  X 4.4e-13        rule-4 scene        R 2.8e-11  t 3.5e-10  X 2.3e-09
  (Levenberg-Marquardt stops on a relative gain of 1e-3, so a rounding difference early in a round is carried, not damped)
No chi2 of either check lies within 1e-6 relative of its threshold in these scenes (test_no_chi2_near_a_threshold).
"""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import with_fills
from seqref import lba as L
from seqref import poseopt as Q

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
CAM = (718.856, 718.856, 607.19, 185.2, 386.1)                                # KITTI: fx, fy, cx, cy, bf
INV_SIGMA2 = np.array([1.0 / 1.2 ** (2 * l) for l in range(8)], f32)
SENTINEL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = dict(R=2.84e-11, t=3.51e-10, X=2.27e-9)                             # what test_textbook_distance prints, see above
TOL = {k: 4 * v for k, v in MEASURED.items()}


def _rot(a):
    a = np.asarray(a, float)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


class Scene:
    """Key-frame rows with true poses, points with true positions, observations; tables() lays them out as the C ABI does.
    The observation table lists a point's observations in the order observe() was called."""

    def __init__(self, rows, cap, pcap, seed):
        self.rows, self.cap, self.pcap = rows, cap, pcap
        self.rng = np.random.default_rng(seed)
        self.R = [np.eye(3)] * rows
        self.t = [np.zeros(3)] * rows
        self.bad = np.zeros(rows, u8)
        self.X = np.zeros((pcap, 3))
        self.flags = np.zeros(pcap, u8)
        self.kps = np.zeros((rows, cap), KP_DTYPE)
        self.kps["x"], self.kps["y"] = self.rng.uniform(0, 1200, (rows, cap)), self.rng.uniform(0, 370, (rows, cap))
        self.kps["octave"] = self.rng.integers(0, 8, (rows, cap))
        self.ur = np.full((rows, cap), -1.0, f32)
        self.slot_point = np.full((rows, cap), -1, i32)
        self.n = np.zeros(rows, i32)
        self.obs = [[] for _ in range(pcap)]
        self.npts = 0

    def pose(self, r, rotvec, centre, bad=False):
        self.R[r] = _rot(rotvec)
        self.t[r] = -self.R[r] @ np.asarray(centre, float)
        self.bad[r] = 1 if bad else 0

    def point(self, X, present=True):
        p = self.npts
        self.npts += 1
        self.X[p] = X
        self.flags[p] = L.POINT_PRESENT if present else 0
        return p

    def observe(self, p, r, stereo=False, offset=(0.0, 0.0), noise=0.3, octave=None, in_slots=True, pix=None):
        fx, fy, cx, cy, bf = CAM
        Xc = self.R[r] @ self.X[p] + self.t[r]
        s = int(self.n[r])
        self.n[r] += 1
        if octave is not None:
            self.kps["octave"][r, s] = octave
        sig = 1.2 ** int(self.kps["octave"][r, s])
        z = Xc[2] if Xc[2] != 0 else 1.0
        u = fx * Xc[0] / z + cx + (self.rng.normal(0, noise) * sig if noise else 0.0) + offset[0]
        v = fy * Xc[1] / z + cy + (self.rng.normal(0, noise) * sig if noise else 0.0) + offset[1]
        if pix is not None:
            u, v = pix
        self.kps["x"][r, s], self.kps["y"][r, s] = u, v
        self.ur[r, s] = (u - bf / z) if stereo else -1.0
        if in_slots:
            self.slot_point[r, s] = p
        self.obs[p].append((r, s))

    def tables(self, cur, ord_list, pose_noise=(0.004, 0.03), point_noise=0.05, mono_only=False, exact=()):
        rows = self.rows
        Tcw = np.zeros((rows, 12), f32)
        for r in range(rows):
            if r in exact:
                Rn, tn = self.R[r], self.t[r]
            else:
                Rn = _rot(self.rng.normal(0, pose_noise[0], 3)) @ self.R[r]
                tn = self.t[r] + self.rng.normal(0, pose_noise[1], 3)
            Tcw[r] = np.c_[Rn, tn].reshape(12)
        world = (self.X + self.rng.normal(0, point_noise, self.X.shape)).astype(f32)
        world[self.npts:] = 0
        obs_start = np.zeros(self.npts + 1, i32)
        kf, idx = [], []
        for p in range(self.npts):
            for r, s in self.obs[p]:
                kf.append(r)
                idx.append(s)
            obs_start[p + 1] = len(kf)
        ord_kf = np.full((rows, rows), -1, i32)
        ord_kf[cur, :len(ord_list)] = ord_list
        n_ord = np.zeros(rows, i32)
        n_ord[cur] = len(ord_list)
        return dict(slot_point=self.slot_point, n=self.n, kf_bad=self.bad, obs_start=obs_start, obs_kf=np.array(kf + [0], i32)[:max(len(kf), 1)],
                    obs_idx=np.array(idx + [0], i32)[:max(len(idx), 1)], flags=self.flags, kps=self.kps,
                    u_right=None if mono_only else self.ur, ord_kf=ord_kf, n_ord=n_ord, Tcw=Tcw, world=world)


def _line_of_cameras(sc, rows, x0=0.0, step=0.8, bad=()):
    for k, r in enumerate(rows):
        sc.pose(r, sc.rng.normal(0, 0.02, 3), [x0 + step * k, sc.rng.normal(0, 0.05), sc.rng.normal(0, 0.05)], bad=r in bad)


def _case(tables, cur, id0_row, max_points, max_edges, stop=None):
    rows, cap = tables["slot_point"].shape
    return dict(tables=tables, cur=cur, id0_row=id0_row, rows=rows, cap=cap, np=len(tables["obs_start"]) - 1,
                pcap=len(tables["flags"]), max_points=max_points, max_edges=max_edges, stop=stop)


def scene_lists():
    """Rule 1, hand-worked.  Rows 0..8; cur = 3; covisible list [5 (bad), 1, 0 (mnId 0)]; so local = [3, 1, 0].  Row 6 sees a
    local point and is bad: stamped as fixed candidate, not listed, no edge.  Row 7 sees local points: fixed.  Row 2 sees only
    a point nobody local sees: nothing.  Row 8 is bad and observes a local point after row 7: never listed, no edge.  Point 4
    sits in two slots of row 3 and in row 1: listed once.  Point 5 is not PRESENT.  Row 5 (bad, stamped local) observes point 0:
    no edge."""
    sc = Scene(9, 12, 16, 11)
    _line_of_cameras(sc, range(9), bad=(5, 6, 8))
    for _ in range(8):
        sc.point([sc.rng.uniform(-2, 6), sc.rng.uniform(-1, 1), sc.rng.uniform(6, 12)])
    sc.flags[5] = 0
    sc.observe(2, 3); sc.observe(0, 3, stereo=True); sc.observe(4, 3); sc.observe(5, 3); sc.observe(4, 3, in_slots=True)
    sc.obs[4].pop()                                                       # the second slot of point 4 is no observation
    sc.observe(1, 1); sc.observe(4, 1, stereo=True); sc.observe(0, 1); sc.observe(3, 1)
    sc.observe(0, 0); sc.observe(2, 0, stereo=True); sc.observe(6, 0)
    sc.observe(0, 5); sc.observe(2, 6); sc.observe(1, 7); sc.observe(3, 7, stereo=True); sc.observe(3, 8); sc.observe(7, 2)
    sc.observe(6, 4)                                                      # row 4: not covisible, sees point 6 of row 0: fixed
    return _case(sc.tables(3, [5, 1, 0]), 3, 0, 16, 32)


LISTS_WANT = dict(local_kf=[3, 1, 0], fixed_kf=[7, 4], local_point=[2, 0, 4, 1, 3, 6])


def scene_S(seed=21, mono_only=False):
    """3 free local key frames, the row of mnId 0, 1 fixed camera, 12 points."""
    sc = Scene(6, 16, 12, seed)
    _line_of_cameras(sc, range(6))
    for _ in range(12):
        sc.point([sc.rng.uniform(-2, 5), sc.rng.uniform(-1.5, 1.5), sc.rng.uniform(6, 14)])
    for p in range(12):
        for r in (0, 1, 2, 3):
            if sc.rng.random() < 0.85:
                sc.observe(p, r, stereo=sc.rng.random() < 0.5)
        if p % 3 == 0:
            sc.observe(p, 4, stereo=p % 2 == 0)
    return _case(sc.tables(2, [1, 3, 0], mono_only=mono_only), 2, 0, 12, 64)


def scene_M(seed=5):
    """6 local (rows 0-5) and 3 fixed (6-8) key frames, 200 points, about 1200 edges, mixed; rows 9-17 are bad observers of
    point 0 (18 observations, 9 edges); row 5 has exactly 65 edges; point 1 has a single observation; about 5 % gross outliers; every
    edge of point 2 is one and every point is behind row 4 (9 edges, consistent but at negative depth), so round 2 drops a
    point and a pose."""
    sc = Scene(18, 200, 208, seed)
    _line_of_cameras(sc, range(9), step=0.6)
    _line_of_cameras(sc, range(9, 18), x0=0.3, step=0.5, bad=range(9, 18))
    sc.pose(4, [0.01, -0.02, 0.0], [2.0, 0.0, 30.0])                      # row 4 stands beyond the points: every depth is < 0
    for _ in range(200):
        sc.point([sc.rng.uniform(-3, 8), sc.rng.uniform(-2, 2), sc.rng.uniform(5, 20)])
    row4 = set(sc.rng.choice(np.arange(3, 200), 8, replace=False).tolist())
    row5 = set(sc.rng.choice(np.arange(3, 200), 64, replace=False).tolist())
    for p in range(200):
        for r in range(9):
            if p < 2:
                see = r == 0 or p == 0
            elif r == 4:
                see = p in row4
            elif r == 5:
                see = p in row5
            else:
                see = sc.rng.random() < 0.8
            if not see:
                continue
            gross = p == 2 or (r != 4 and sc.rng.random() < 0.045)
            ang, mag = sc.rng.uniform(0, 2 * np.pi), sc.rng.uniform(15, 40)
            sc.observe(p, r, stereo=sc.rng.random() < 0.5, offset=(mag * math.cos(ang), mag * math.sin(ang)) if gross else (0.0, 0.0))
        if p == 0:
            for r in range(9, 18):
                sc.observe(p, r)
    return _case(sc.tables(0, [3, 1, 4, 2, 5]), 0, -1, 208, 1400)


def scene_zero_depth():
    """Scene S with a point at the optical centre of row 1 in the input estimate: division by zero in its edge."""
    b = scene_S(23)
    t = b["tables"]
    p = int(t["slot_point"][1, 0])
    # the depth is exactly zero in the arithmetic of the edge: the camera at the origin with the identity rotation
    t["Tcw"][1] = np.c_[np.eye(3), np.zeros(3)].reshape(12).astype(f32)
    t["world"][p] = (0.0, 0.0, 0.0)
    return b


def scene_rule4(seed, behind=2e-3):
    """Rule 4.  Rows 0-3 local, 4-6 fixed, 16 ordinary points, and two special ones.
    Point 16 has one honest observation at octave 0 (row 1), three honest ones at octave 7 (rows 0, 2, 4) and two outliers
    displaced the same way (row 3 at octave 0, row 5 at octave 3): under Huber the outliers drag it a few pixels, the octave-0
    edge passes 5.991 and goes to level 1 with them, the octave-7 edges stay; round 2 brings the point back, so at the final
    estimate the octave-0 edge has a small chi2 and a positive depth, and is erased on its round-1 error alone.
    Point 17 lies `behind` metres behind the image plane of row 3 (which stands among the points), close to its centre, with
    a consistent observation: its edge leaves round 1 for its depth only; the seeds are chosen so that round 2 brings it to the
    front, and the final check does not erase it."""
    sc = Scene(7, 24, 18, seed)
    _line_of_cameras(sc, range(7), step=0.5)
    sc.pose(3, sc.rng.normal(0, 0.02, 3), [1.0, 0.2, 5.0])
    for _ in range(16):
        sc.point([sc.rng.uniform(-2, 4), sc.rng.uniform(-1.5, 1.5), sc.rng.uniform(7, 12)])
    for p in range(16):
        for r in range(7):
            if sc.rng.random() < 0.85:
                sc.observe(p, r, stereo=sc.rng.random() < 0.4)
    p = sc.point([1.2, 0.1, 8.0])
    sc.observe(p, 1, octave=0); sc.observe(p, 0, octave=7); sc.observe(p, 2, octave=7); sc.observe(p, 4, octave=7)
    sc.observe(p, 3, octave=0, offset=(25.0, 0.0)); sc.observe(p, 5, octave=3, offset=(25.0, 0.0))
    p = sc.point(-sc.R[3].T @ sc.t[3] + sc.R[3].T @ np.array([0.6 * behind, -0.4 * behind, -behind]))
    sc.observe(p, 0, octave=1); sc.observe(p, 1, octave=1); sc.observe(p, 2, octave=0); sc.observe(p, 3, octave=0, noise=0.0)
    sc.observe(p, 4, octave=1)
    return _case(sc.tables(0, [1, 2, 3], pose_noise=(0.002, 0.01), point_noise=0.02), 0, -1, 18, 160)


CASES = ["lists", "S", "S_mono", "M", "zero_depth", "edges_plus_one", "points_plus_one", "stop_set", "stop_clear", "no_edges",
         "rule4"]
RULE4_SEED = 205


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "lists":
        return scene_lists()
    if name == "S":
        return scene_S()
    if name == "S_mono":
        return scene_S(22, mono_only=True)
    if name == "M":
        return scene_M()
    if name == "zero_depth":
        return scene_zero_depth()
    if name == "edges_plus_one":
        b = scene_S()
        return dict(b, max_edges=reference("S")["report"][4] + reference("S")["report"][5] - 1)
    if name == "points_plus_one":
        return dict(scene_S(), max_points=11)
    if name == "stop_set":
        return dict(scene_S(), stop=1)
    if name == "stop_clear":
        return dict(scene_S(), stop=0)
    if name == "no_edges":
        b = scene_S()
        b["tables"]["flags"][:] = 0
        return b
    if name == "rule4":
        return scene_rule4(RULE4_SEED)
    raise KeyError(name)


def run_seqref(b, trace=None, stop="case"):
    return L.local_bundle_adjustment(b["cur"], b["id0_row"], CAM, b["tables"], INV_SIGMA2, b["max_points"], b["max_edges"],
                                     stop=b["stop"] if stop == "case" else stop, trace=trace)


def prefilled(b):
    """The caller's output arrays, full of sentinel bytes."""
    fill = lambda count: np.full(count * 4, SENTINEL, u8).view(i32)  # noqa: E731
    return dict(local_kf=fill(b["rows"]), fixed_kf=fill(b["rows"]), local_point=fill(b["max_points"]),
                erase=fill(b["max_edges"] * 3).reshape(-1, 3), report=fill(16))


def as_arrays(b, r):
    """A seqref answer in the layout of the C ABI: what the call does not write keeps the sentinel."""
    o = prefilled(b)
    for k in ("local_kf", "fixed_kf", "local_point"):
        if r[k] is not None:
            o[k][:len(r[k])] = r[k]
    if r["erase"]:
        o["erase"][:len(r["erase"])] = r["erase"]
    o["report"][:] = r["report"]
    o["Tcw"], o["world"] = r["Tcw"].reshape(-1, 12), r["world"].reshape(-1, 3)
    return o


@functools.lru_cache(maxsize=None)
def reference(name):
    r = run_seqref(case(name))
    return dict(as_arrays(case(name), r), raw=r)


def assert_same(got, ref, what):
    for k in ("report", "local_kf", "fixed_kf", "local_point", "erase", "Tcw", "world"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.tobytes() == w.tobytes(), "%s: %s differs\n%s\n%s" % (what, k, g.reshape(-1)[:24], w.reshape(-1)[:24])


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked rules
def test_rule1_the_three_lists():
    r = reference("lists")["raw"]
    for k, v in LISTS_WANT.items():
        assert r[k] == v, k
    # an edge for every observation whose key frame is not bad: points 2 (3, 0), 0 (3, 1, 0; not 5), 4 (3, 1), 1 (1, 7),
    # 3 (1, 7; not 8), 6 (0, 4); rows 6, 8 and 5 give none
    assert r["report"][:6] == [L.OK, 3, 2, 6, r["report"][4], r["report"][5]] and r["report"][4] + r["report"][5] == 13
    # mono iff u_right < 0
    assert r["report"][5] == 4


def test_rule2_fixed_row_keeps_its_pose_up_to_the_round_trip():
    """The row of mnId 0 is local and fixed: its Tcw is the input through toSE3Quat and toCvMat, nothing else; a fixed
    camera is not written at all."""
    b, r = case("S"), reference("S")["raw"]
    q, t = Q.pose_from_Tcw(b["tables"]["Tcw"][0])
    R = Q.to_R(q)
    want = np.array([R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]).astype(f32)
    assert r["Tcw"][0].tobytes() == want.tobytes()
    assert r["fixed_kf"] == [4] and r["Tcw"][4].tobytes() == b["tables"]["Tcw"][4].tobytes()
    assert r["Tcw"][5].tobytes() == b["tables"]["Tcw"][5].tobytes()          # row 5 takes no part
    assert r["Tcw"][2].tobytes() != b["tables"]["Tcw"][2].tobytes()


def test_rule2_huber_deltas_are_floats():
    assert Q.f32(math.sqrt(5.991)) != math.sqrt(5.991)
    tr = {}
    run_seqref(case("S"), trace=tr)
    assert set(tr["est"]) == {0, 1}


@pytest.mark.parametrize("stereo", [False, True])
def test_rule2_edge_terms_are_the_gradient_of_half_chi2(stereo):
    """b_l and b_p of an edge without kernel are minus the gradient of chi2 / 2 with respect to the point and to the pose
    increment (exp(u) * pose), taken numerically: both Jacobians, the sign of omega_r and the monocular / stereo split."""
    cam = tuple(float(f32(v)) for v in CAM)
    e = Q.Edge()
    e.stereo = stereo
    e.obs = [640.0, 200.0] + ([610.0] if stereo else [])
    e.inv, e.delta, e.dsqr = 0.5, 2.0, 4.0
    e.X = [0.7, -0.4, 9.0]
    pose = Q.pose_from_Tcw(np.c_[_rot([0.05, -0.1, 0.02]), [0.2, 0.1, -0.3]].reshape(12))
    _, _, Hll, bl, Hpp, bp, B = L.linearize(e, pose, cam, False, True)

    def half_chi2(dX, u):
        e2 = Q.Edge()
        e2.stereo, e2.obs, e2.inv = e.stereo, e.obs, e.inv
        e2.X = [e.X[k] + dX[k] for k in range(3)]
        return 0.5 * Q.edge_error(e2, Q.se3_mul(Q.se3_exp(u), pose), cam)[1]
    # the stereo projection rounds 1/z to float (types_six_dof_expmap.cpp:151): a wider step and bound keep that noise out
    h, tol = (1e-3, 2e-3) if stereo else (1e-6, 1e-5)
    for k in range(3):
        d = [h if j == k else 0.0 for j in range(3)]
        g = (half_chi2(d, [0.0] * 6) - half_chi2([-v for v in d], [0.0] * 6)) / (2 * h)
        assert abs(g + bl[k]) <= tol * max(1.0, abs(g)), (k, g, bl[k])
    for k in range(6):
        u = [h if j == k else 0.0 for j in range(6)]
        g = (half_chi2([0.0] * 3, u) - half_chi2([0.0] * 3, [-v for v in u])) / (2 * h)
        assert abs(g + bp[k]) <= tol * max(1.0, abs(g)), (k, g, bp[k])
    # Huber beyond delta: the terms shrink by rho[1] = delta / sqrt(chi2), rho[0] = 2 sqrt(chi2) delta - delta^2
    chi2, rho0, _, blk, _, _, _ = L.linearize(e, pose, cam, True, True)
    assert chi2 > e.dsqr and rho0 == 2 * math.sqrt(chi2) * e.delta - e.dsqr
    assert all(abs(blk[k] - bl[k] * (e.delta / math.sqrt(chi2))) <= 1e-12 * abs(bl[k]) for k in range(3))


def test_rule3_round_two_drops_edges_a_point_and_a_pose():
    r = reference("M")["raw"]
    rep = r["report"]
    assert rep[0] == L.OK and rep[1] == 6 and rep[2] == 3 and rep[3] == 200
    assert rep[6] > 40 and rep[12] == 6 and rep[13] == 5                        # the pose of row 4 leaves the system
    t = case("M")["tables"]
    assert int((t["obs_kf"] == 5).sum()) == 65 and int(t["obs_start"][2] - t["obs_start"][1]) == 1 and int(t["obs_start"][1]) == 18
    assert rep[7] >= rep[6] - 5


def test_rule3_vertex_outside_the_system_keeps_its_round_one_estimate():
    tr = {}
    b = case("M")
    r = run_seqref(b, trace=tr)
    v = r["local_kf"].index(4)
    assert tr["est"][0][v] == tr["est"][1][v]                                   # bit for bit: no zero update
    i = r["local_point"].index(2)
    nv = len(r["local_kf"]) + len(r["fixed_kf"])
    assert tr["est"][0][nv + i] == tr["est"][1][nv + i]
    assert tr["est"][0][0] != tr["est"][1][0]


def _final_chi2(b, r, tr):
    """chi2 of every erase candidate at the final estimate, recomputed: (row, idx, point) -> chi2."""
    out = {}
    t = b["tables"]
    nv = len(r["local_kf"]) + len(r["fixed_kf"])
    vrows = r["local_kf"] + r["fixed_kf"]
    for i, p in enumerate(r["local_point"]):
        for o in range(int(t["obs_start"][p]), int(t["obs_start"][p + 1])):
            kf, idx = int(t["obs_kf"][o]), int(t["obs_idx"][o])
            if kf not in vrows:
                continue
            e = Q.Edge()
            e.stereo = t["u_right"] is not None and not (float(t["u_right"][kf][idx]) < 0)
            e.obs = [float(t["kps"]["x"][kf][idx]), float(t["kps"]["y"][kf][idx])] + ([float(t["u_right"][kf][idx])] if e.stereo else [])
            e.inv = float(INV_SIGMA2[int(t["kps"]["octave"][kf][idx])])
            e.X = tr["est"][1][nv + i]
            pose = tr["est"][1][vrows.index(kf)]
            out[(kf, idx, p)] = (Q.edge_error(e, (pose[:4], pose[4:]), tuple(float(f32(v)) for v in CAM))[1], 7.815 if e.stereo else 5.991)
    return out


def test_rule4_an_edge_is_erased_on_its_stale_chi2():
    """A level-1 edge is not active in round 2, so the final check reads its round-1 error: in this scene at least one erase
    row has a chi2 below the threshold and a positive depth at the final estimate, and is erased all the same."""
    tr = {}
    b = case("rule4")
    r = run_seqref(b, trace=tr)
    chi = _final_chi2(b, r, tr)
    stale = [row for row in r["erase"] if chi[tuple(row)][0] <= chi[tuple(row)][1]]
    assert [1, 16, 16] in stale                                                 # the honest octave-0 edge of point 16
    assert all(x[4] for x in tr["level1"] if x[2] == 16)                        # every depth was positive: the chi2 alone


def test_rule4_an_edge_out_for_depth_only_comes_back_and_stays():
    """The edge of point 17 in row 3 goes to level 1 with a chi2 below the threshold, for its depth alone; isDepthPositive is
    evaluated at the current estimate, round 2 brings the point in front of the camera, and the final check keeps it."""
    tr = {}
    r = run_seqref(case("rule4"), trace=tr)
    out = [x for x in tr["level1"] if x[0] == 3 and x[2] == 17]
    assert len(out) == 1 and out[0][3] < 5.991 and not out[0][4]
    assert not [row for row in r["erase"] if row[0] == 3 and row[2] == 17]


def test_stop_byte_and_capacity():
    s = reference("S")["raw"]["report"]
    r = reference("stop_set")["raw"]
    assert r["report"][0] == L.STOPPED and r["local_kf"] is None and r["report"][15] == 1
    assert r["Tcw"].tobytes() == case("S")["tables"]["Tcw"].tobytes()
    r = reference("edges_plus_one")["raw"]
    assert r["report"][0] == L.CAPACITY and r["report"][4:6] == s[4:6]
    r = reference("points_plus_one")["raw"]
    assert r["report"][0] == L.CAPACITY and r["report"][3] == 12
    r = reference("stop_clear")["raw"]
    assert r["report"][0] == L.OK and r["report"][15] >= 4
    assert as_arrays(case("S"), r)["Tcw"].tobytes() == reference("S")["Tcw"].tobytes()
    r = reference("no_edges")["raw"]
    assert r["report"][0] == L.OK and r["report"][3] == 0 and r["report"][8] == 0 and r["local_kf"] == [2, 1, 3, 0]


def test_stop_sequence_samples():
    """The sampling points, through scripted sequences: :655, the top of iteration 0, the end of a rejected trial, the top of
    the next iterations, :664, then round 2."""
    b = case("S")
    r = run_seqref(b, stop=[0, 1, 1])                                           # terminate() at the top of iteration 0, then :664
    assert r["report"][0] == L.ONE_ROUND and r["report"][8] == 0 and r["report"][15] == 3
    r = run_seqref(b, stop=[0, 1, 0, 0])                                        # round 1 empty, :664 clear, round 2 runs
    assert r["report"][0] == L.OK and r["report"][8] == 0 and r["report"][10] > 0
    r = run_seqref(b, stop=[0, 0, 1, 1])                                        # one iteration, then stopped
    assert r["report"][0] == L.ONE_ROUND and r["report"][8] == 1


def test_no_chi2_near_a_threshold():
    """No chi2 either check reads (after round 1, after round 2; stale ones included), and none recomputed at the final
    estimate, lies within 1e-6 relative of its threshold, so the erase lists do not hang on rounding."""
    for name in ("S", "S_mono", "M", "rule4", "lists", "zero_depth"):
        tr = {}
        b = case(name)
        r = run_seqref(b, trace=tr)
        for (chi2, thr) in list(_final_chi2(b, r, tr).values()) + tr["check1"] + tr["check2"]:
            assert not abs(chi2 - thr) <= 1e-6 * thr, name                  # a NaN or an infinite chi2 (zero depth) is not near


# ---------------------------------------------------------------------------------------------------------------------
# the textbook restatement: full normal equations, rotation matrices, numpy.linalg.solve, libm
def _textbook(b):
    t = b["tables"]
    r0 = reference_lists(b)
    lkf, fkf, lpt = r0
    fx, fy, cx, cy, bf = [float(f32(v)) for v in CAM]
    vrows = lkf + fkf
    free = [v for v, r in enumerate(lkf) if r != b["id0_row"]]
    col = {v: k for k, v in enumerate(free)}
    Rs, ts = [], []
    for r in vrows:
        q, tt = Q.pose_from_Tcw(t["Tcw"][r])
        Rs.append(np.array(Q.to_R(q)).reshape(3, 3))
        ts.append(np.array(tt))
    X = [t["world"][p].astype(f64) for p in lpt]
    edges = []
    for i, p in enumerate(lpt):
        for o in range(int(t["obs_start"][p]), int(t["obs_start"][p + 1])):
            kf, idx = int(t["obs_kf"][o]), int(t["obs_idx"][o])
            if t["kf_bad"] is not None and t["kf_bad"][kf]:
                continue
            ur = -1.0 if t["u_right"] is None else float(t["u_right"][kf][idx])
            st = not (ur < 0)
            obs = np.array([float(t["kps"]["x"][kf][idx]), float(t["kps"]["y"][kf][idx])] + ([ur] if st else []))
            edges.append(dict(v=vrows.index(kf), i=i, st=st, obs=obs, inv=float(INV_SIGMA2[int(t["kps"]["octave"][kf][idx])]),
                              row=(kf, idx, p), lvl=0, chi2=0.0))
    np6 = 6 * len(free)

    def proj(e, Rs, ts, X):
        P = Rs[e["v"]] @ X[e["i"]] + ts[e["v"]]
        if e["st"]:
            invz = float(f32(1.0 / P[2]))
            p0, p1 = P[0] * invz * fx + cx, P[1] * invz * fy + cy
            return np.array([p0, p1, p0 - bf * invz]), P
        return np.array([P[0] / P[2] * fx + cx, P[1] / P[2] * fy + cy]), P

    def chi(e, Rs, ts, X, kernel):
        pr, P = proj(e, Rs, ts, X)
        err = e["obs"] - pr
        c = e["inv"] * float(err @ err)
        d = float(f32(math.sqrt(7.815 if e["st"] else 5.991)))
        if kernel and c > d * d:
            return c, 2 * math.sqrt(c) * d - d * d, d / math.sqrt(c), err, P
        return c, c, 1.0, err, P

    def skew(w):
        return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])

    def exp_se3(u):
        w, up = u[:3], u[3:]
        th = np.linalg.norm(w)
        Om = skew(w)
        if th < 1e-5:
            R = np.eye(3) + Om + Om @ Om
            V = R
        else:
            R = np.eye(3) + math.sin(th) / th * Om + (1 - math.cos(th)) / th ** 2 * Om @ Om
            V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * Om + (th - math.sin(th)) / th ** 3 * Om @ Om
        return R, V @ up

    def optimize(iters, kernel):
        nonlocal Rs, ts, X
        act = [e for e in edges if e["lvl"] == 0]
        if not act:
            return
        pts = sorted({e["i"] for e in act})
        pcol = {i: np6 + 3 * k for k, i in enumerate(pts)}
        pin = sorted({col[e["v"]] for e in act if e["v"] in col})
        keep = [6 * c + a for c in pin for a in range(6)] + list(range(np6, np6 + 3 * len(pts)))
        lam = ni = 0.0
        nbad = 0
        x = np.zeros(np6 + 3 * len(pts))
        for it in range(iters):
            H = np.zeros((len(x), len(x)))
            g = np.zeros(len(x))
            cur = 0.0
            for e in act:
                c, r0_, r1, err, P = chi(e, Rs, ts, X, kernel)
                e["chi2"] = c
                cur += r0_
                xx, yy, z = P
                Jc = np.array([[xx * yy / z ** 2 * fx, -(1 + xx * xx / z ** 2) * fx, yy / z * fx, -fx / z, 0, xx / z ** 2 * fx],
                               [(1 + yy * yy / z ** 2) * fy, -xx * yy / z ** 2 * fy, -xx / z * fy, 0, -fy / z, yy / z ** 2 * fy]])
                Jp = -np.array([[fx / z, 0, -xx / z ** 2 * fx], [0, fy / z, -yy / z ** 2 * fy]]) @ Rs[e["v"]]
                if e["st"]:
                    Jc = np.vstack([Jc, Jc[0] + np.array([-bf * yy / z ** 2, bf * xx / z ** 2, 0, 0, 0, -bf / z ** 2])])
                    Jp = np.vstack([Jp, Jp[0] - bf * Rs[e["v"]][2] / z ** 2])
                J = np.zeros((len(err), len(x)))
                if e["v"] in col:
                    J[:, 6 * col[e["v"]]:6 * col[e["v"]] + 6] = Jc
                J[:, pcol[e["i"]]:pcol[e["i"]] + 3] = Jp
                w = r1 * e["inv"]
                H += w * J.T @ J
                g += -w * J.T @ err
            ini = cur
            if it == 0:
                lam, ni, nbad = 1e-5 * np.abs(np.diag(H)[keep]).max(), 2.0, 0
            q, rho = 0, 0.0
            while True:
                Hk = H[np.ix_(keep, keep)] + lam * np.eye(len(keep))
                ok2 = True
                try:
                    np.linalg.cholesky(Hk)
                    x[:] = 0
                    x[keep] = np.linalg.solve(Hk, g[keep])
                except np.linalg.LinAlgError:
                    ok2 = False
                Rn, tn, Xn = list(Rs), list(ts), list(X)
                for c in pin:
                    v = free[c]
                    dR, dt = exp_se3(x[6 * c:6 * c + 6])
                    Rn[v], tn[v] = dR @ Rs[v], dR @ ts[v] + dt
                for i in pts:
                    Xn[i] = X[i] + x[pcol[i]:pcol[i] + 3]
                tmp = 0.0
                for e in act:
                    c, r0_, _, _, _ = chi(e, Rn, tn, Xn, kernel)
                    e["chi2"] = c
                    tmp += r0_
                if not ok2:
                    tmp = Q.DBL_MAX
                rho = (cur - tmp) / (float(x @ (lam * x + g)) + 1e-3)
                if rho > 0 and math.isfinite(tmp):
                    lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                    ni = 2.0
                    cur = tmp
                    Rs, ts, X = Rn, tn, Xn
                else:
                    lam *= ni
                    ni *= 2
                q += 1
                if not (rho < 0 and q < 10):
                    break
            if q == 10 or rho == 0:
                break
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                break

    def bad(e):
        P = Rs[e["v"]] @ X[e["i"]] + ts[e["v"]]
        return e["chi2"] > (7.815 if e["st"] else 5.991) or not P[2] > 0

    optimize(5, True)
    for e in edges:
        if bad(e):
            e["lvl"] = 1
    optimize(10, False)
    erase = [list(e["row"]) for want in (False, True) for e in edges if e["st"] == want and bad(e)]
    return dict(R={r: Rs[v] for v, r in enumerate(lkf)}, t={r: ts[v] for v, r in enumerate(lkf)}, X={p: X[i] for i, p in enumerate(lpt)},
                erase=erase)


def reference_lists(b):
    r = run_seqref(dict(b, stop=None))                                          # the lists are integer work: taken from the seqref
    return r["local_kf"], r["fixed_kf"], r["local_point"]


@pytest.mark.parametrize("name", ["S", "S_mono", "M", "rule4"])
def test_textbook_distance(name):
    b = case(name)
    tr = {}
    r = run_seqref(b, trace=tr)
    tb = _textbook(b)
    assert sorted(map(tuple, r["erase"])) == sorted(map(tuple, tb["erase"])) and r["erase"] == tb["erase"]
    nv = len(r["local_kf"]) + len(r["fixed_kf"])
    dR = dt = dX = 0.0
    for v, row in enumerate(r["local_kf"]):
        p = tr["est"][1][v]
        dR = max(dR, np.abs(np.array(Q.to_R(p[:4])).reshape(3, 3) - tb["R"][row]).max())
        dt = max(dt, np.abs(np.array(p[4:]) - tb["t"][row]).max())
    for i, p in enumerate(r["local_point"]):
        dX = max(dX, np.abs(np.array(tr["est"][1][nv + i]) - tb["X"][p]).max())
    print("textbook distance %s: R %.2e t %.2e X %.2e" % (name, dR, dt, dX))
    assert dR <= TOL["R"] and dt <= TOL["t"] and dX <= TOL["X"]


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the shared core
@functools.lru_cache(maxsize=None)
def host_program():
    d = tempfile.mkdtemp(prefix="lba_host_")
    exe = os.path.join(d, "lba_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lba_host.cpp"),
                    "-o", exe], check=True)
    return exe


def pack(b, o, script):
    t = b["tables"]
    total = int(t["obs_start"][-1])
    h = np.zeros(16, i32)
    h[:13] = [b["cur"], b["id0_row"], b["rows"], b["cap"], b["np"], b["pcap"], len(INV_SIGMA2), b["max_points"], b["max_edges"],
              t["kf_bad"] is not None, t["u_right"] is not None, script is not None, 0 if script is None else len(script)]
    parts = [h, np.array(CAM, f32), INV_SIGMA2, t["slot_point"], t["n"]]
    if t["kf_bad"] is not None:
        parts.append(t["kf_bad"])
    parts += [t["obs_start"], t["obs_kf"][:total], t["obs_idx"][:total], t["flags"], t["kps"]]
    if t["u_right"] is not None:
        parts.append(t["u_right"])
    parts += [t["ord_kf"], t["n_ord"], t["Tcw"], t["world"], np.array([] if script is None else script, u8)]
    parts += [o[k] for k in ("local_kf", "fixed_kf", "local_point", "erase", "report")]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def run_host(b, tmp_path, tag, script="case", fill=0):
    if script == "case":
        script = None if b["stop"] is None else [b["stop"]]
    o = prefilled(b)
    fin, fout = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    fin.write_bytes(pack(b, o, script))
    subprocess.run([host_program(), str(fin), str(fout), str(fill)], check=True)
    raw = fout.read_bytes()
    off = 0
    got = {}
    shapes = dict(Tcw=(f32, b["rows"] * 12), world=(f32, b["pcap"] * 3), local_kf=(i32, b["rows"]), fixed_kf=(i32, b["rows"]),
                  local_point=(i32, b["max_points"]), erase=(i32, b["max_edges"] * 3), report=(i32, 16))
    for k in ("Tcw", "world", "local_kf", "fixed_kf", "local_point", "erase", "report"):
        dt, cnt = shapes[k]
        got[k] = np.frombuffer(raw[off:off + cnt * dt().itemsize], dt)
        off += cnt * dt().itemsize
    snap = b["rows"] * 7 + b["max_points"] * 3
    got["trace"] = np.frombuffer(raw[off:], f64).reshape(4, snap)
    return got


def _trace_rows(b, r, tr, what, rnd):
    nv = len(r["local_kf"]) + len(r["fixed_kf"])
    out = np.zeros(b["rows"] * 7 + b["max_points"] * 3)
    vals = tr[what][rnd]
    for v in range(nv):
        out[v * 7:v * 7 + 7] = vals[v]
    for i in range(len(r["local_point"])):
        out[b["rows"] * 7 + 3 * i:b["rows"] * 7 + 3 * i + 3] = vals[nv + i]
    return out


@pytest.mark.parametrize("name,fill", with_fills(CASES))
def test_host_build_matches_seqref(name, fill, tmp_path):
    """`fill`: the byte the workspace holds before the run (the device's slot is never cleared)."""
    b = case(name)
    got = run_host(b, tmp_path, name, fill=fill)
    assert_same(got, reference(name), name)
    tr = {}
    r = run_seqref(b, trace=tr)
    if r["local_kf"] is not None:                                               # the estimate and the tried estimate of each round
        for k, (what, rnd) in enumerate((("est", 0), ("tried", 0), ("est", 1), ("tried", 1))):
            assert got["trace"][k].tobytes() == _trace_rows(b, r, tr, what, rnd).tobytes(), (name, what, rnd)


@pytest.mark.parametrize("script", [[0, 1, 1], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 1, 0], [0] * 9 + [1, 0, 0, 1],
                                    [1], [0]])
def test_host_build_samples_the_stop_byte_where_the_seqref_does(script, tmp_path):
    for name in ("S", "rule4"):
        b = case(name)
        got = run_host(b, tmp_path, name, script=script)
        r = run_seqref(b, stop=script)
        assert_same(got, as_arrays(b, r), (name, script))
