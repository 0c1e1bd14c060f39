"""The sequential reference of Optimizer::BundleAdjustment and of the map update of RunGlobalBundleAdjustment
(tests/seqref/gba.py) on its own: hand-worked cases for the rules it pins, the distance to a textbook restatement (full normal
equations without Schur, rotation matrices, numpy.linalg.solve, libm), a host build of orbhip_gba_core.h that must match it bit
for bit, and the cases the GPU tests replay (test_gba_gpu.py imports them from here; the reference answers are computed once per
process).

Measured on the CPU against the textbook restatement (the asserted tolerances are four times the maxima); pose = max entry of R
and of t (m), point = max coordinate (m), all in double before the write-back; in each scene the accept / reject decisions of
the two Levenberg-Marquardt loops agree trial by trial (asserted):
  scene base (mixed, no kernel)  R 4.01e-11  t 1.23e-10  X 2.40e-10     scene robust (Huber)  R 3.78e-16  t 1.32e-14  X 4.80e-14
  scene stereo                   R 3.26e-11  t 2.08e-10  X 1.01e-10     scene no_id0 (no fixed row)  R 3.68e-11  t 1.71e-10  X 7.84e-10
(Levenberg-Marquardt stops on a relative gain of 1e-3, so a rounding difference early on is carried, not damped; in no_id0 the
free gauge is held by the damping alone)

The scenes are small on purpose: the Python reference is sequential.  The panel-width scenes have 3, 4, 5, 8, 9 and 37 free
poses (the device factorises in panels of 4 poses); scene `wide` has a pose with more than 64 edges (more than one entry per lane
of its wavefront) and a point with more than 16.
"""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import test_lba_cpu as K
from helpers import with_fills
from seqref import gba as G
from seqref import lba as L
from seqref import poseopt as Q

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
CAM, INV_SIGMA2, SENTINEL, ROOT = K.CAM, K.INV_SIGMA2, K.SENTINEL, K.ROOT
MEASURED = dict(R=4.01e-11, t=2.08e-10, X=7.84e-10)                              # what test_textbook_distance prints, see above
TOL = {k: 4 * v for k, v in MEASURED.items()}
TABLE_KEYS = ("kf_bad", "kf_id", "obs_start", "obs_kf", "obs_idx", "flags", "kps", "u_right", "Tcw", "world")
OUT_KEYS = ("Tcw", "world", "TcwGBA", "posGBA", "kf_mark", "pt_mark", "point_list", "report")


def make_scene(seed, rows, npts, cap, see=0.8, stereo=0.5, bad=(), step=0.6, pcap=None, min_obs=2):
    """Cameras on a line looking along +z, points in front of them; every point is seen by at least min_obs rows."""
    sc = K.Scene(rows, cap, pcap or npts, seed)
    K._line_of_cameras(sc, range(rows), step=step, bad=bad)
    for _ in range(npts):
        sc.point([sc.rng.uniform(-2, step * rows + 2), sc.rng.uniform(-2, 2), sc.rng.uniform(6, 16)])
    for p in range(npts):
        seen = [r for r in range(rows) if sc.rng.random() < see]
        while len(seen) < min_obs:
            r = int(sc.rng.integers(0, rows))
            if r not in seen:
                seen.append(r)
        for r in sorted(seen):
            if sc.n[r] < cap:
                sc.observe(p, r, stereo=sc.rng.random() < stereo)
    return sc


def _case(sc, kf_id=None, iterations=10, robust=0, mode=G.STAGED, kf_list=None, pt_list=None, stop=None, max_points=None,
          max_edges=None, mono_only=False, pose_noise=(0.004, 0.03), point_noise=0.05):
    t = sc.tables(0, [], pose_noise=pose_noise, point_noise=point_noise, mono_only=mono_only)
    tables = {k: t[k] for k in TABLE_KEYS if k != "kf_id"}
    tables["kf_id"] = np.arange(sc.rows, dtype=i32) if kf_id is None else np.array(kf_id, i32)
    total = int(t["obs_start"][-1])
    return dict(tables=tables, rows=sc.rows, cap=sc.cap, np=len(t["obs_start"]) - 1, pcap=len(t["flags"]), iterations=iterations,
                robust=robust, mode=mode, kf_list=kf_list, pt_list=pt_list, stop=stop,
                max_points=max_points or max(sc.npts, 1), max_edges=max_edges or max(total, 1))


def scene_base():
    """5 rows (row 0 is mnId 0), 14 points, mixed monocular and stereo observations."""
    return make_scene(31, 5, 14, 16)


def scene_rules():
    """Rows 0..6, kf_id = row; row 3 is bad.  Points: 0..9 ordinary; 10 is not PRESENT; 11 is seen by row 3 (bad) only; 12 is
    seen by rows 1, 3 (bad) and 6; point 13 by rows 2 and 6."""
    sc = make_scene(32, 7, 10, 16, pcap=16, bad=(3,))
    for X in ([1.0, 0.2, 9.0], [2.0, -0.5, 11.0], [0.5, 0.4, 8.0], [3.0, 0.1, 10.0]):
        sc.point(X)
    sc.flags[10] = 0
    sc.observe(10, 0); sc.observe(10, 1)
    sc.observe(11, 3)
    sc.observe(12, 1); sc.observe(12, 3, stereo=True); sc.observe(12, 6, stereo=True)
    sc.observe(13, 2); sc.observe(13, 6)
    return sc


CASES = ["base", "in_place", "robust", "robust_off", "rules", "newer_row", "null_vertex", "mono", "stereo", "stop_set", "stop_clear",
         "no_id0", "points_plus_one", "edges_plus_one", "rows_513", "pt_list", "no_edges",
         "f3", "f4", "f5", "f8", "f9", "f37", "wide"]


def _outlier_scene():
    sc = make_scene(33, 5, 14, 16)
    sc.kps["x"][2, 0] += 35.0                                                   # a gross outlier: the first observation of row 2
    sc.kps["y"][3, 1] -= 28.0                                                   # and the second of row 3
    return sc


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "base":
        return _case(scene_base())
    if name == "in_place":
        return _case(scene_base(), mode=G.IN_PLACE)
    if name == "robust":
        return _case(_outlier_scene(), robust=1)
    if name == "robust_off":
        return _case(_outlier_scene(), robust=0)
    if name == "rules":
        return _case(scene_rules())
    if name == "newer_row":                                                     # kf_list omits the newest row: kf_id > maxKFid
        return _case(scene_rules(), kf_list=[5, 0, 1, 2, 3, 4])
    if name == "null_vertex":                                                   # kf_list omits row 2, older than the newest listed
        return _case(scene_rules(), kf_list=[0, 1, 3, 4, 5, 6])
    if name == "mono":
        return _case(make_scene(34, 5, 14, 16), mono_only=True)
    if name == "stereo":
        return _case(make_scene(35, 5, 14, 16, stereo=1.0))
    if name == "stop_set":
        return dict(case("base"), stop=1)
    if name == "stop_clear":
        return dict(case("base"), stop=0)
    if name == "no_id0":
        return _case(scene_base(), kf_id=[7, 3, 4, 5, 6])
    if name == "points_plus_one":
        return dict(case("base"), max_points=13)
    if name == "edges_plus_one":
        return dict(case("base"), max_edges=int(case("base")["tables"]["obs_start"][-1]) - 1)
    if name == "rows_513":
        return _case(K.Scene(513, 1, 1, 1), iterations=2)
    if name == "pt_list":                                                       # vpMP in an order of its own, one point left out
        return _case(scene_base(), pt_list=[5, 3, 13, 0, 1, 2, 4, 6, 7, 8, 9, 10, 11], mode=G.IN_PLACE)
    if name == "no_edges":
        b = _case(scene_base())
        b["tables"]["flags"][:] = 0
        return b
    if name in ("f3", "f4", "f5", "f8", "f9"):
        nf = int(name[1:])
        return _case(make_scene(40 + nf, nf + 1, 6 * nf, 24, see=0.6), iterations=4)
    if name == "f37":
        return _case(make_scene(77, 38, 110, 16, see=0.09, min_obs=3), iterations=3)
    if name == "wide":                                                          # row 1: 70 edges; point 0: 18 edges
        sc = K.Scene(19, 80, 100, 78)
        K._line_of_cameras(sc, range(19), step=0.4)
        for _ in range(100):
            sc.point([sc.rng.uniform(-1, 8), sc.rng.uniform(-2, 2), sc.rng.uniform(6, 16)])
        for r in range(1, 19):
            sc.observe(0, r, stereo=r % 2 == 0)
        for p in range(1, 100):
            rows = [1] if p < 70 else []
            rows += [int(r) for r in sc.rng.choice([0] + list(range(2, 19)), 2, replace=False)]
            for r in sorted(rows):
                sc.observe(p, r, stereo=sc.rng.random() < 0.5)
        return _case(sc, iterations=3)
    raise KeyError(name)


def prefilled(b):
    """The caller's output arrays: sentinel bytes, and clear marks."""
    fill = lambda count, dt: np.full(count * np.dtype(dt).itemsize, SENTINEL, u8).view(dt)  # noqa: E731
    return dict(TcwGBA=fill(b["rows"] * 12, f32).reshape(-1, 12), posGBA=fill(b["pcap"] * 3, f32).reshape(-1, 3),
                kf_mark=np.zeros(b["rows"], u8), pt_mark=np.zeros(b["pcap"], u8), point_list=fill(b["max_points"], i32),
                report=fill(16, i32))


def run_seqref(b, trace=None, stop="case", refuse_null=False):
    o = prefilled(b)
    r = G.global_bundle_adjustment(CAM, b["tables"], INV_SIGMA2, b["iterations"], b["robust"], b["mode"], b["max_points"], b["max_edges"],
                                   kf_list=b["kf_list"], pt_list=b["pt_list"], stop=b["stop"] if stop == "case" else stop, out=o,
                                   refuse_null=refuse_null, trace=trace)
    r["report"] = np.array(r["report"], i32)
    return r


@functools.lru_cache(maxsize=None)
def reference(name):
    return run_seqref(case(name))


def assert_same(got, ref, what):
    for k in OUT_KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.tobytes() == w.tobytes(), "%s: %s differs\n%s\n%s" % (what, k, g.reshape(-1)[:24], w.reshape(-1)[:24])


def _round_trip(T):
    q, t = Q.pose_from_Tcw(T)
    R = Q.to_R(q)
    return np.array([R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked rules
def test_fixed_row_is_written_as_its_round_trip():
    b, r = case("base"), reference("base")
    assert r["report"][:4].tolist() == [G.OK, 5, 4, 14] and r["report"][11] == 24
    assert r["TcwGBA"][0].tobytes() == _round_trip(b["tables"]["Tcw"][0]).tobytes() and r["kf_mark"][0] == 1
    assert r["TcwGBA"][1].tobytes() != _round_trip(b["tables"]["Tcw"][1]).tobytes()
    assert r["report"][9] >= 1 and r["report"][10] >= r["report"][9]


def test_staged_and_in_place_write_the_same_numbers_to_different_places():
    b, s, p = case("base"), reference("base"), reference("in_place")
    t = b["tables"]
    assert s["Tcw"].tobytes() == t["Tcw"].tobytes() and s["world"].tobytes() == t["world"].tobytes()          # STAGED: untouched
    assert s["kf_mark"].tolist() == [1] * 5 and s["pt_mark"].tolist() == [1] * 14
    assert s["point_list"].tobytes() == prefilled(b)["point_list"].tobytes() and s["report"][12] == 0
    assert p["Tcw"].tobytes() == s["TcwGBA"].tobytes() and p["world"].tobytes() == s["posGBA"].tobytes()
    assert p["kf_mark"].sum() == 0 and p["pt_mark"].sum() == 0 and p["TcwGBA"].tobytes() == prefilled(b)["TcwGBA"].tobytes()
    assert p["point_list"].tolist() == list(range(14)) and p["report"][12] == 14


def test_bad_row_bad_point_and_point_with_bad_observers_only():
    b, r = case("rules"), reference("rules")
    t = b["tables"]
    rep = r["report"]
    # vertices: rows 0, 1, 2, 4, 5, 6; row 0 fixed
    assert rep[0] == G.OK and rep[1] == 6 and rep[2] == 5
    assert r["kf_mark"].tolist() == [1, 1, 1, 0, 1, 1, 1]
    assert r["TcwGBA"][3].tobytes() == prefilled(b)["TcwGBA"][3].tobytes()
    # points 0..9, 12, 13 included; 10 not PRESENT (its observations are not even looked at); 11 removed
    assert rep[3] == 12 and rep[4] == 1
    assert r["pt_mark"][:14].tolist() == [1] * 10 + [0, 0, 1, 1] and r["pt_mark"][14:].sum() == 0
    for p in (10, 11, 14, 15):
        assert r["posGBA"][p].tobytes() == prefilled(b)["posGBA"][p].tobytes()
    # skipped by the bad rule: every observation by row 3 of an included or removed point
    by3 = sum(1 for p in range(14) if p != 10 for o in range(t["obs_start"][p], t["obs_start"][p + 1]) if t["obs_kf"][o] == 3)
    assert rep[7] == by3 and by3 >= 2 and rep[8] == 0
    # mono iff u_right < 0
    n_st = sum(1 for p in range(14) if p != 10 for o in range(t["obs_start"][p], t["obs_start"][p + 1])
               if t["obs_kf"][o] != 3 and not t["u_right"][t["obs_kf"][o], t["obs_idx"][o]] < 0)
    assert rep[6] == n_st and rep[5] + rep[6] == int(t["obs_start"][14]) - 2 - by3


def test_observations_of_a_row_newer_than_max_kfid_are_skipped():
    b, r = case("newer_row"), reference("newer_row")
    t = b["tables"]
    by6 = sum(1 for p in range(14) if p != 10 for o in range(t["obs_start"][p], t["obs_start"][p + 1]) if t["obs_kf"][o] == 6)
    full = reference("rules")["report"]
    assert r["report"][1] == 5 and r["report"][7] == full[7] + by6 and r["report"][8] == 0
    assert r["kf_mark"].tolist() == [1, 1, 1, 0, 1, 1, 0]
    # point 12 keeps its edge of row 1; point 13 its edge of row 2: one edge each, still included
    assert r["pt_mark"][12] == 1 and r["pt_mark"][13] == 1
    # list order is vertex order: the free poses are rows 5, 1, 2, 4
    tr = {}
    run_seqref(b, trace=tr)
    assert tr["vtx_rows"] == [5, 0, 1, 2, 4]


def test_null_vertex_is_counted_or_refused():
    b, r = case("null_vertex"), reference("null_vertex")
    t = b["tables"]
    by2 = sum(1 for p in range(14) if p != 10 for o in range(t["obs_start"][p], t["obs_start"][p + 1]) if t["obs_kf"][o] == 2)
    assert r["report"][8] == by2 and by2 >= 1 and r["kf_mark"][2] == 0
    with pytest.raises(ValueError):
        run_seqref(b, refuse_null=True)


def test_mono_and_stereo_scenes_count_their_edges():
    m, s = reference("mono")["report"], reference("stereo")["report"]
    assert m[6] == 0 and m[5] > 20 and s[5] == 0 and s[6] > 20


def test_huber_kernels_change_the_result_and_their_deltas_are_floats():
    assert Q.f32(math.sqrt(5.99)) != math.sqrt(5.99) and Q.f32(math.sqrt(5.99)) != Q.f32(math.sqrt(5.991))
    on, off = reference("robust"), reference("robust_off")
    assert on["report"][:9].tolist() == off["report"][:9].tolist()
    assert on["TcwGBA"].tobytes() != off["TcwGBA"].tobytes() and on["posGBA"].tobytes() != off["posGBA"].tobytes()


def test_stop_byte_set_on_entry_still_writes_the_round_trip():
    b, r = case("stop_set"), reference("stop_set")
    assert r["report"][0] == G.STOPPED and r["report"][9] == 0 and r["report"][10] == 0 and r["report"][15] == 1
    for row in range(5):
        assert r["TcwGBA"][row].tobytes() == _round_trip(b["tables"]["Tcw"][row]).tobytes()
    assert r["posGBA"][:14].tobytes() == b["tables"]["world"][:14].tobytes() and r["kf_mark"].sum() == 5 and r["pt_mark"].sum() == 14
    c = reference("stop_clear")
    assert c["report"][0] == G.OK and c["report"][15] >= c["report"][9] and c["TcwGBA"].tobytes() == reference("base")["TcwGBA"].tobytes()


def test_without_an_id0_row_nothing_is_fixed():
    r = reference("no_id0")
    assert r["report"][0] == G.OK and r["report"][1] == 5 and r["report"][2] == 5 and r["report"][11] == 30
    assert r["TcwGBA"][0].tobytes() != _round_trip(case("no_id0")["tables"]["Tcw"][0]).tobytes()


def test_capacity_refusals_write_only_the_report():
    for name in ("points_plus_one", "edges_plus_one", "rows_513"):
        b, r = case(name), reference(name)
        assert r["report"][0] == G.CAPACITY and r["report"][9] == 0, name
        o = prefilled(b)
        for k in ("TcwGBA", "posGBA", "kf_mark", "pt_mark", "point_list"):
            assert r[k].tobytes() == o[k].tobytes(), (name, k)
    assert reference("rows_513")["report"][1] == 513
    assert reference("points_plus_one")["report"][3] == 14 and reference("edges_plus_one")["report"][3] == 14


def test_point_list_order_is_the_order_of_the_points():
    r = reference("pt_list")
    assert r["point_list"][:13].tolist() == [5, 3, 13, 0, 1, 2, 4, 6, 7, 8, 9, 10, 11] and r["report"][3] == 13
    assert r["world"][12].tobytes() == case("pt_list")["tables"]["world"][12].tobytes()


def test_no_point_no_iteration():
    r = reference("no_edges")
    assert r["report"].tolist() == [G.OK, 5, 4, 0, 0, 0, 0, 0, 0, 0, 0, 24, 0, 0, 0, 0] and r["kf_mark"].sum() == 5


def test_panel_scenes_have_the_free_poses_their_names_say():
    for name in ("f3", "f4", "f5", "f8", "f9", "f37"):
        assert reference(name)["report"][2] == int(name[1:]) and reference(name)["report"][0] == G.OK, name
    t = case("wide")["tables"]
    assert int((t["obs_kf"] == 1).sum()) == 70 and int(t["obs_start"][1]) == 18


def test_vectorised_ldlt_equals_the_sequential_one():
    rng = np.random.default_rng(3)
    M = rng.normal(size=(60, 60))
    A = M @ M.T + 60 * np.eye(60)
    b = rng.normal(size=60)
    ok1, x1 = L.ldlt_solve([list(map(float, row)) for row in A], [float(v) for v in b])
    ok2, x2 = G.ldlt_solve_rows([list(map(float, row)) for row in A], [float(v) for v in b])
    assert ok1 and ok2 and np.array(x1).tobytes() == np.array(x2).tobytes()
    A[7, 7] = -1.0
    assert G.ldlt_solve_rows(A.tolist(), b.tolist())[0] is False and L.ldlt_solve(A.tolist(), b.tolist())[0] is False


# ---------------------------------------------------------------------------------------------------------------------
# a textbook restatement
def _textbook(b):
    """Full normal equations over (free poses, points), rotation matrices, numpy.linalg.solve, libm; the vertices and edges are
    taken from the seqref's trace (integer work)."""
    fx, fy, cx, cy, bf = (float(f32(v)) for v in CAM)
    t = b["tables"]
    tr = {}
    run_seqref(b, trace=tr)
    vrows, lpt = tr["vtx_rows"], tr["points"]
    vtx = {r: v for v, r in enumerate(vrows)}
    free = [v for v, r in enumerate(vrows) if t["kf_id"][r] != 0]
    col = {v: c for c, v in enumerate(free)}
    Rs, ts = [], []
    for r in vrows:                                                             # toSE3Quat: the estimate starts from a quaternion
        q, tt = Q.pose_from_Tcw(t["Tcw"][r])
        Rs.append(np.array(Q.to_R(q)).reshape(3, 3))
        ts.append(np.array(tt))
    X = [np.array(t["world"][p], f64) for p in lpt]
    max_id = max(int(t["kf_id"][r]) for r in vrows)
    edges = []
    for i, p in enumerate(lpt):
        for o in range(int(t["obs_start"][p]), int(t["obs_start"][p + 1])):
            r, idx = int(t["obs_kf"][o]), int(t["obs_idx"][o])
            if (t["kf_bad"] is not None and t["kf_bad"][r]) or int(t["kf_id"][r]) > max_id or r not in vtx:
                continue
            st = t["u_right"] is not None and not t["u_right"][r, idx] < 0
            obs = [float(t["kps"]["x"][r, idx]), float(t["kps"]["y"][r, idx])] + ([float(t["u_right"][r, idx])] if st else [])
            edges.append(dict(v=vtx[r], i=i, st=st, obs=np.array(obs), inv=float(INV_SIGMA2[int(t["kps"]["octave"][r, idx])])))
    np6 = 6 * len(free)
    n = np6 + 3 * len(lpt)
    kernel = bool(b["robust"])

    def chi(e, Rs, ts, X):
        P = Rs[e["v"]] @ X[e["i"]] + ts[e["v"]]
        if e["st"]:
            invz = float(f32(1.0 / P[2]))
            p0 = P[0] * invz * fx + cx
            pr = np.array([p0, P[1] * invz * fy + cy, p0 - bf * invz])
        else:
            pr = np.array([P[0] / P[2] * fx + cx, P[1] / P[2] * fy + cy])
        err = e["obs"] - pr
        c = e["inv"] * float(err @ err)
        d = float(f32(math.sqrt(7.815 if e["st"] else 5.99)))
        if kernel and c > d * d:
            return 2 * math.sqrt(c) * d - d * d, d / math.sqrt(c), err, P
        return c, 1.0, err, P

    def skew(w):
        return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])

    def exp_se3(u):
        w, up = u[:3], u[3:]
        th = np.linalg.norm(w)
        Om = skew(w)
        if th < 1e-5:
            R = np.eye(3) + Om + Om @ Om
            return R, R @ up
        R = np.eye(3) + math.sin(th) / th * Om + (1 - math.cos(th)) / th ** 2 * Om @ Om
        V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * Om + (th - math.sin(th)) / th ** 3 * Om @ Om
        return R, V @ up

    lam = ni = 0.0
    nbad = 0
    x = np.zeros(n)
    decisions = []
    for it in range(b["iterations"]):
        H = np.zeros((n, n))
        g = np.zeros(n)
        cur = 0.0
        for e in edges:
            r0, r1, err, P = chi(e, Rs, ts, X)
            cur += r0
            xx, yy, z = P
            Jc = np.array([[xx * yy / z ** 2 * fx, -(1 + xx * xx / z ** 2) * fx, yy / z * fx, -fx / z, 0, xx / z ** 2 * fx],
                           [(1 + yy * yy / z ** 2) * fy, -xx * yy / z ** 2 * fy, -xx / z * fy, 0, -fy / z, yy / z ** 2 * fy]])
            Jp = -np.array([[fx / z, 0, -xx / z ** 2 * fx], [0, fy / z, -yy / z ** 2 * fy]]) @ Rs[e["v"]]
            if e["st"]:
                Jc = np.vstack([Jc, Jc[0] + np.array([-bf * yy / z ** 2, bf * xx / z ** 2, 0, 0, 0, -bf / z ** 2])])
                Jp = np.vstack([Jp, Jp[0] - bf * Rs[e["v"]][2] / z ** 2])
            J = np.zeros((len(err), n))
            if e["v"] in col:
                J[:, 6 * col[e["v"]]:6 * col[e["v"]] + 6] = Jc
            J[:, np6 + 3 * e["i"]:np6 + 3 * e["i"] + 3] = Jp
            w = r1 * e["inv"]
            H += w * J.T @ J
            g += -w * J.T @ err
        ini = cur
        if it == 0:
            lam, ni, nbad = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
        q, rho = 0, 0.0
        while True:
            Hk = H + lam * np.eye(n)
            ok2 = True
            try:
                np.linalg.cholesky(Hk)
                x = np.linalg.solve(Hk, g)
            except np.linalg.LinAlgError:
                ok2 = False
            Rn, tn = list(Rs), list(ts)
            for v, c in col.items():
                dR, dt = exp_se3(x[6 * c:6 * c + 6])
                Rn[v], tn[v] = dR @ Rs[v], dR @ ts[v] + dt
            Xn = [X[i] + x[np6 + 3 * i:np6 + 3 * i + 3] for i in range(len(lpt))]
            tmp = sum(chi(e, Rn, tn, Xn)[0] for e in edges)
            if not ok2:
                tmp = Q.DBL_MAX
            rho = (cur - tmp) / (float(x @ (lam * x + g)) + 1e-3)
            acc = rho > 0 and math.isfinite(tmp)
            decisions.append(acc)
            if acc:
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
    return dict(R=Rs, t=ts, X=X, decisions=decisions)


@pytest.mark.parametrize("name", ["base", "robust", "stereo", "no_id0"])
def test_textbook_distance(name):
    b = case(name)
    tr = {}
    run_seqref(b, trace=tr)
    tb = _textbook(b)
    assert [d[0] for d in tr["decisions"]] == tb["decisions"], "the accept / reject decisions differ: the scene is not fit for this test"
    dR = dt = dX = 0.0
    for v in range(len(tr["vtx_rows"])):
        p = tr["pose"][v]
        dR = max(dR, np.abs(np.array(Q.to_R(p[:4])).reshape(3, 3) - tb["R"][v]).max())
        dt = max(dt, np.abs(np.array(p[4:]) - tb["t"][v]).max())
    for i in range(len(tr["points"])):
        dX = max(dX, np.abs(np.array(tr["pt"][i]) - tb["X"][i]).max())
    print("textbook distance %s: R %.2e t %.2e X %.2e (%d trials)" % (name, dR, dt, dX, len(tb["decisions"])))
    assert dR <= TOL["R"] and dt <= TOL["t"] and dX <= TOL["X"]


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the shared core
@functools.lru_cache(maxsize=None)
def host_program():
    d = tempfile.mkdtemp(prefix="gba_host_")
    exe = os.path.join(d, "gba_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "gba_host.cpp"),
                    "-o", exe], check=True)
    return exe


def pack(b, o, script):
    t = b["tables"]
    total = int(t["obs_start"][-1])
    kl, pl = b["kf_list"], b["pt_list"]
    h = np.zeros(24, i32)
    h[:18] = [b["rows"], b["cap"], b["np"], b["pcap"], len(INV_SIGMA2), b["max_points"], b["max_edges"], t["kf_bad"] is not None,
              t["u_right"] is not None, script is not None, 0 if script is None else len(script), kl is not None,
              0 if kl is None else len(kl), pl is not None, 0 if pl is None else len(pl), b["iterations"], b["robust"], b["mode"]]
    parts = [h, np.array(CAM, f32), INV_SIGMA2]
    if t["kf_bad"] is not None:
        parts.append(t["kf_bad"])
    parts += [t["kf_id"], t["obs_start"], t["obs_kf"][:total], t["obs_idx"][:total], t["flags"], t["kps"]]
    if t["u_right"] is not None:
        parts.append(t["u_right"])
    parts += [t["Tcw"], t["world"], np.array([] if script is None else script, u8), np.array([] if kl is None else kl, i32),
              np.array([] if pl is None else pl, i32)]
    parts += [o[k] for k in ("TcwGBA", "posGBA", "kf_mark", "pt_mark", "point_list", "report")]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def unpack(b, raw):
    shapes = dict(Tcw=(f32, b["rows"] * 12), world=(f32, b["pcap"] * 3), TcwGBA=(f32, b["rows"] * 12), posGBA=(f32, b["pcap"] * 3),
                  kf_mark=(u8, b["rows"]), pt_mark=(u8, b["pcap"]), point_list=(i32, b["max_points"]), report=(i32, 16))
    off, got = 0, {}
    for k in OUT_KEYS:
        dt, cnt = shapes[k]
        got[k] = np.frombuffer(raw, dt, cnt, off)
        off += got[k].nbytes
    assert off == len(raw)
    return got


def run_host(b, tmp_path, tag, script="case", fill=0):
    if script == "case":
        script = None if b["stop"] is None else [b["stop"]]
    fin, fout = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    fin.write_bytes(pack(b, prefilled(b), script))
    subprocess.run([host_program(), "ba", str(fin), str(fout), str(fill)], check=True)
    return unpack(b, fout.read_bytes())


@pytest.mark.parametrize("name,fill", with_fills(CASES))
def test_host_build_matches_seqref(name, fill, tmp_path):
    """`fill`: the byte the workspace holds before the run (the device's slot is never cleared)."""
    assert_same(run_host(case(name), tmp_path, name, fill=fill), reference(name), name)


@pytest.mark.parametrize("script", [[0, 1], [0, 0, 1, 0], [0, 0, 0, 1], [0] * 6 + [1], [1], [0]])
def test_host_build_samples_the_stop_byte_where_the_seqref_does(script, tmp_path):
    for name in ("base", "robust"):
        b = case(name)
        assert_same(run_host(b, tmp_path, name, script=script), run_seqref(b, stop=script), (name, script))


# ---------------------------------------------------------------------------------------------------------------------
# the apply step
APPLY_KEYS = ("kf_mark", "TcwGBA", "Tcw", "world", "TcwBefGBA", "report")


def _pose12(rng, centre):
    R = K._rot(rng.normal(0, 0.3, 3))
    return np.c_[R, -R @ np.asarray(centre, float)].reshape(12).astype(f32)


@functools.lru_cache(maxsize=None)
def apply_case(name="tree"):
    """Rows 0..8.  0 is an origin (marked) with children 1 (marked) and 2 (unmarked); 3 is the unmarked child of 2 (a
    grandchild); 4 is bad with parent 0 and 5 is its child: never reached; 6 is a second origin (marked) with the unmarked
    child 7; 8 is marked, in nobody's tree: never popped.
    Points: 0 marked (posGBA); 1 reference row 1 (marked, popped): moved; 2 reference row 3 (marked by the walk): moved; 3
    reference row 5 (unmarked): left; 4 reference -1: left; 5 not PRESENT (and marked): untouched; 6 reference row 8 (marked,
    never popped, so without a TcwBefGBA): left."""
    rng = np.random.default_rng(91)
    rows, pcap = 9, 8
    parent = np.array([-1, 0, 0, 2, 0, 4, -1, 6, -1], i32)
    kf_bad = np.zeros(rows, u8)
    kf_bad[4] = 1
    kf_mark = np.array([1, 1, 0, 0, 0, 0, 1, 0, 1], u8)
    Tcw = np.stack([_pose12(rng, rng.uniform(-3, 3, 3)) for _ in range(rows)])
    TcwGBA = np.stack([_pose12(rng, rng.uniform(-3, 3, 3)) for _ in range(rows)])
    flags = np.array([1, 1, 1, 1, 1, 0, 1, 0], u8)
    pt_mark = np.array([1, 0, 0, 0, 0, 1, 0, 0], u8)
    ref_kf = np.array([0, 1, 3, 5, -1, 0, 8, 0], i32)
    world = rng.uniform(-5, 5, (pcap, 3)).astype(f32)
    posGBA = rng.uniform(-5, 5, (pcap, 3)).astype(f32)
    a = dict(origins=np.array([0, 6], i32), parent=parent, kf_bad=kf_bad, kf_mark=kf_mark, TcwGBA=TcwGBA, Tcw=Tcw, pt_mark=pt_mark,
             posGBA=posGBA, flags=flags, ref_kf=ref_kf, world=world)
    if name == "no_bad":
        a = dict(a, kf_bad=None)
    return a


def apply_prefilled(a):
    rows = len(a["parent"])
    return dict(TcwBefGBA=np.full(rows * 48, SENTINEL, u8).view(f32).reshape(rows, 12), report=np.full(32, SENTINEL, u8).view(i32))


@functools.lru_cache(maxsize=None)
def apply_reference(name="tree"):
    a = apply_case(name)
    r = G.apply_global_ba(dict(a, TcwBefGBA=apply_prefilled(a)["TcwBefGBA"]))
    r["report"] = np.array(r["report"], i32)
    return r


def assert_same_apply(got, ref, what):
    for k in APPLY_KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.tobytes() == w.tobytes(), "%s: %s differs\n%s\n%s" % (what, k, g.reshape(-1)[:24], w.reshape(-1)[:24])


def _T4(T):
    return np.vstack([np.array(T, f64).reshape(3, 4), [0, 0, 0, 1]])


def test_apply_walks_the_trees_and_moves_the_points():
    a, r = apply_case(), apply_reference()
    assert r["report"].tolist() == [6, 3, 1, 2, 3, 6, 0, 0]                       # popped: 0, 6, 1, 2, 7, 3
    assert r["kf_mark"].tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1]
    sent = apply_prefilled(a)["TcwBefGBA"]
    for k in (0, 1, 2, 3, 6, 7):
        assert r["TcwBefGBA"][k].tobytes() == a["Tcw"][k].tobytes() and r["Tcw"][k].tobytes() == r["TcwGBA"][k].tobytes()
    for k in (4, 5, 8):
        assert r["TcwBefGBA"][k].tobytes() == sent[k].tobytes() and r["Tcw"][k].tobytes() == a["Tcw"][k].tobytes()
    assert r["TcwGBA"][1].tobytes() == a["TcwGBA"][1].tobytes()                   # a marked child keeps its own
    # the unmarked child and the grandchild, against float64 matrices: the parent's OLD pose is inverted
    want2 = _T4(a["Tcw"][2]) @ np.linalg.inv(_T4(a["Tcw"][0])) @ _T4(a["TcwGBA"][0])
    assert np.abs(_T4(r["TcwGBA"][2]) - want2).max() < 2e-5
    want3 = _T4(a["Tcw"][3]) @ np.linalg.inv(_T4(a["Tcw"][2])) @ want2
    assert np.abs(_T4(r["TcwGBA"][3]) - want3).max() < 4e-5
    assert np.abs(_T4(r["TcwGBA"][3]) - _T4(a["Tcw"][3]) @ np.linalg.inv(want2) @ want2).max() > 1e-2    # not the new pose's inverse
    # points
    assert r["world"][0].tobytes() == a["posGBA"][0].tobytes()
    for p, row in ((1, 1), (2, 3)):
        Xc = _T4(a["Tcw"][row]) @ np.r_[a["world"][p].astype(f64), 1]
        want = np.linalg.inv(_T4(r["Tcw"][row])) @ Xc
        assert np.abs(r["world"][p] - want[:3]).max() < 1e-4 and r["world"][p].tobytes() != a["world"][p].tobytes()
    for p in (3, 4, 5, 6, 7):
        assert r["world"][p].tobytes() == a["world"][p].tobytes()


def test_apply_refuses_an_unmarked_origin_in_the_host_form():
    a = apply_case()
    with pytest.raises(ValueError):
        G.apply_global_ba(dict(a, origins=np.array([0, 2], i32)), refuse=True)
    r = G.apply_global_ba(dict(a, origins=np.array([2, 0, 6], i32)))           # the device form leaves it out
    assert r["report"] == apply_reference()["report"].tolist()


def pack_apply(a, o):
    rows, pcap = len(a["parent"]), len(a["flags"])
    h = np.zeros(8, i32)
    h[:4] = [rows, pcap, len(a["origins"]), a["kf_bad"] is not None]
    parts = [h, a["origins"], a["parent"]] + ([a["kf_bad"]] if a["kf_bad"] is not None else [])
    parts += [a["kf_mark"], a["TcwGBA"], a["Tcw"], a["pt_mark"], a["posGBA"], a["flags"], a["ref_kf"], a["world"], o["TcwBefGBA"], o["report"]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.mark.parametrize("name,fill", with_fills(["tree", "no_bad"]))
def test_host_build_of_the_apply_step_matches_seqref(name, fill, tmp_path):
    a = apply_case(name)
    rows, pcap = len(a["parent"]), len(a["flags"])
    fin, fout = tmp_path / "a.in", tmp_path / "a.out"
    fin.write_bytes(pack_apply(a, apply_prefilled(a)))
    subprocess.run([host_program(), "apply", str(fin), str(fout), str(fill)], check=True)
    raw, off, got = fout.read_bytes(), 0, {}
    for k, dt, cnt in (("kf_mark", u8, rows), ("TcwGBA", f32, rows * 12), ("Tcw", f32, rows * 12), ("world", f32, pcap * 3),
                       ("TcwBefGBA", f32, rows * 12), ("report", i32, 8)):
        got[k] = np.frombuffer(raw, dt, cnt, off)
        off += got[k].nbytes
    assert off == len(raw)
    assert_same_apply(got, apply_reference(name), name)
    if name == "no_bad":                                                        # row 4 is in the map now: 4 and 5 are reached
        assert got["report"][:2].tolist() == [8, 5]
