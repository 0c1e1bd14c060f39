"""Optimizer::OptimizeEssentialGraph: the sequential reference (tests/seqref/essgraph.py), its rules, the one-thread host build of
csrc/orbhip_essgraph_core.h (bit for bit), and a textbook restatement in numpy (same numeric Jacobian, libm, numpy.linalg.solve).

The cases are built here and shared with the GPU tests; every reference answer is computed once per process.
  H        the hand-built graph of 10 rows: every rule of :863 and :956-961 is hit once, the edge list is written out below
  r6, r6_fix   6 rows, one loop connection; the fix_scale pair
  p4, p5, r6   3, 4 and 5 free vertices: one less than, equal to and one more than a panel of 4 poses
  p8, p9, p10  7, 8 and 9 free vertices: the same around two panels (p10 spans three and is no multiple of a panel)
  r37      37 rows, 36 free vertices: nine panels
  bad9     a bad row inside the ring; pts is r6 with points on both branches of :1021-1029 and points with no usable reference
  nullv    a bad parent, a bad old-loop partner and a bad loop-connection partner: the device form skips and counts them
  edges_plus_one   max_edges exceeded by one; cap513: 513 rows that are not bad, no points: ORBHIP_EG_CAPACITY both ways
  singular a pose holding a NaN: no pivot is > 0 on any trial, ORBHIP_EG_SINGULAR (compared NaN for NaN, bytes elsewhere)
From lambda 1e-16 every trial is a Gauss-Newton step in all but name: the first is accepted and brings chi2 to within the 1e-7 noise of the numeric Jacobian of
its minimum, the following ones are rejected (lambda only reaches 3.5e-3) until the tenth trial ends the optimisation through
qmax == 10, as g2o does; in H and r37 that tenth trial is accepted, in the others rejected.  So accepted trials, rejected
trials and that stop are all reached by the scenes; the judge is also checked on a hand-worked state
(test_judge_rejects_on_a_hand_worked_state), as s3o_classify was.

Textbook distance (test_textbook_distance prints it; DESIGN.md section 3 and profiles/essgraph_stage.json quote it): the
largest differences over all scenes were R 4.4e-6, t 6.2e-5, s 2.9e-6 (MEASURED, scene r37; the numeric Jacobian with delta
1e-9 carries a relative noise of 1e-7 into either solve); the bound is ten times that.  The
decisions and the iteration counts are equal on every scene but nullv (TEXTBOOK_EXEMPT says why: a step at the floor of chi2).  On the noise-free ring of 12 key frames the restatement comes
within RING_MEASURED of ground truth; the code under test must come within ten times that."""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import FILLS, with_fills
from seqref import essgraph as E
from seqref.poseopt import quat_from_R, to_R
from seqref.sim3opt import sim3_exp, sim3_inverse, sim3_mul

i32, f32, f64, u8 = np.int32, np.float32, np.float64, np.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
MEASURED = dict(R=4.41e-06, t=6.15e-05, s=2.91e-06)                               # what test_textbook_distance prints, see above
TOL = {k: 10 * v for k, v in MEASURED.items()}
RING_MEASURED = dict(R=7.60e-03, t=3.98e-02)                                       # the restatement against ground truth, ring12
RING_TOL = {k: 10 * v for k, v in RING_MEASURED.items()}
TABLE_KEYS = ("kf_bad", "kf_id", "parent", "conn_w", "ord_kf", "ord_w", "n_ord", "loop_start", "loop_kf", "lc_start", "lc_kf", "corrected",
              "non_corrected", "in_corrected", "in_non_corrected", "flags", "ref_kf", "corrected_by_kf", "corrected_ref", "Tcw", "world")
OUT_KEYS = ("point_list", "Scw", "Swc", "report")


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def _sim3_of(R, t, s=1.0):
    return quat_from_R([float(v) for v in np.asarray(R, f64).reshape(9)]) + [float(v) for v in t] + [float(s)]


def _tcw_of(S):
    R = np.array(to_R(S[0:4]), f64).reshape(3, 3)
    return np.hstack([R, (np.array(S[4:7]) / S[7])[:, None]]).astype(f32).reshape(12)


def _csr(lists, rows):
    start = np.zeros(rows + 1, i32)
    flat = []
    for r in range(rows):
        flat += sorted(lists.get(r, []))
        start[r + 1] = len(flat)
    return start, np.array(flat if flat else [0], i32)[:max(len(flat), 1)], len(flat)


def _ordered(conn_w):
    rows = len(conn_w)
    ord_kf, ord_w, n_ord = np.zeros((rows, rows), i32), np.zeros((rows, rows), i32), np.zeros(rows, i32)
    for r in range(rows):
        nz = [(int(conn_w[r][c]), c) for c in range(rows) if conn_w[r][c] > 0]
        nz.sort(key=lambda wc: (-wc[0], wc[1]))
        n_ord[r] = len(nz)
        for k, (w, c) in enumerate(nz):
            ord_kf[r][k], ord_w[r][k] = c, w
    return ord_kf, ord_w, n_ord


def ring(rows, seed, band=2, bad=(), fix_scale=False, npts=24, drift=(0.004, -0.003, 0.006, 0.02), noise=0.0, loops=None, group=2,
         max_edges=None, nan_row=None, null_entries=False):
    """Key frames on a circle looking inwards, a chain of relative motions with a rotation and scale drift per step, closed
    between the last row (cur) and row 0 with the true loop Sim3; cur's `group` predecessors travel with it."""
    rng = np.random.default_rng(seed)
    truth = []
    for k in range(rows):
        a = 2 * math.pi * k / (rows + 1.5)
        c = np.array([6 * math.cos(a), 0.3 * math.sin(3 * a), 6 * math.sin(a)])
        Rwc = _rodrigues(np.array([0.0, -a + math.pi / 2, 0.0])) @ _rodrigues(np.array([0.05 * math.sin(a), 0.0, 0.03]))
        Rcw = Rwc.T
        truth.append(_sim3_of(Rcw, -Rcw @ c))
    # the drifted map: SE3 poses in one world frame; step k turns by the drift rotation and is measured in a local scale that
    # has drifted to sigma_k, so the relative translations grow with it
    d = sim3_exp([drift[0], drift[1], drift[2], 0.0, 0.0, 0.0, 0.0])
    est, sigma = [truth[0]], [1.0]
    for k in range(1, rows):
        n = sim3_exp(list(rng.normal(0, noise, 6)) + [0.0]) if noise else sim3_exp([0.0] * 7)
        rel = sim3_mul(truth[k], sim3_inverse(truth[k - 1]))
        sigma.append(sigma[-1] * math.exp(drift[3]))
        rel = rel[0:4] + [sigma[-1] * v for v in rel[4:7]] + [1.0]
        est.append(sim3_mul(sim3_mul(n, d), sim3_mul(rel, est[k - 1])))
    Tcw = np.stack([_tcw_of(S) for S in est])
    cur, loop_row = rows - 1, 0
    kf_bad = np.zeros(rows, u8)
    for r in bad:
        kf_bad[r] = 1
    conn_w = np.zeros((rows, rows), i32)
    for a in range(rows):
        for b in range(a):
            if a - b <= band:
                conn_w[a][b] = conn_w[b][a] = 160 - 45 * (a - b) + int(rng.integers(0, 9))
            elif a - b == band + 1:
                conn_w[a][b] = conn_w[b][a] = 30 + int(rng.integers(0, 9))
    lc = {cur: [0, 1], cur - 1: [0, 1] if rows > 6 else [0]}
    conn_w[cur][0] = conn_w[0][cur] = 60                                     # the exempt pair, below the gate
    conn_w[cur][1] = conn_w[1][cur] = 120
    conn_w[cur - 1][0] = conn_w[0][cur - 1] = 110
    if rows > 6:
        conn_w[cur - 1][1] = conn_w[1][cur - 1] = 70                         # gated
    parent = np.arange(-1, rows - 1).astype(i32)
    for r in range(rows):                                                      # a bad row's child hangs on the row before it
        while parent[r] >= 0 and kf_bad[parent[r]]:
            parent[r] -= 1
    loop_lists = dict(loops or {})
    if null_entries:
        b0 = int(bad[0])
        parent[b0 + 1] = b0
        loop_lists.setdefault(rows - 2, []).append(b0)
        loop_lists.setdefault(b0, []).append(rows - 2)
        lc[cur] = sorted(lc[cur] + [b0])
    ord_kf, ord_w, n_ord = _ordered(conn_w)
    loop_start, loop_kf, _ = _csr(loop_lists, rows)
    lc_start, lc_kf, _ = _csr(lc, rows)
    # the loop: cur's corrected Sim3 is its true pose at the scale its part of the map has; its group follows (:445-512)
    s_cur = sigma[cur]
    corrected, non_corrected = np.zeros((rows, 8), f64), np.zeros((rows, 8), f64)
    corrected[:, 3] = non_corrected[:, 3] = corrected[:, 7] = non_corrected[:, 7] = 1.0
    in_c, in_nc = np.zeros(rows, u8), np.zeros(rows, u8)
    g_cw = truth[cur][0:4] + [s_cur * v for v in truth[cur][4:7]] + [s_cur]
    nc_cur = E.sim3_from_Tcw(Tcw[cur])
    for r in range(cur - group, cur + 1):
        if kf_bad[r]:
            continue
        nc = E.sim3_from_Tcw(Tcw[r])
        non_corrected[r], in_nc[r] = nc, 1
        corrected[r], in_c[r] = (g_cw if r == cur else sim3_mul(sim3_mul(nc, sim3_inverse(nc_cur)), g_cw)), 1
    pcap = npts + 3 if npts else 0
    world, flags = np.zeros((max(pcap, 1), 3), f32)[:pcap], np.zeros(pcap, u8)
    ref_kf, cby, cref = np.full(pcap, -1, i32), np.full(pcap, -1, i32), np.full(pcap, -1, i32)
    good = [r for r in range(rows) if not kf_bad[r]]
    for p in range(npts):
        world[p] = rng.normal(0, 2.0, 3)
        flags[p] = 0 if p % 7 == 3 else 1
        ref_kf[p] = good[int(rng.integers(0, len(good)))]
        if p % 5 == 1:
            cby[p], cref[p] = cur, good[int(rng.integers(0, len(good)))]
        elif p % 5 == 2:
            cby[p], cref[p] = cur - 1, 0                                       # corrected by another key frame: the reference row counts
    if npts:
        flags[npts:] = 1
        world[npts:] = rng.normal(0, 2.0, (3, 3))
        ref_kf[npts] = -1
        ref_kf[npts + 1] = bad[0] if len(bad) else -1
        cby[npts + 2], cref[npts + 2], ref_kf[npts + 2] = cur, -1, 2
    if nan_row is not None:
        Tcw[nan_row][3] = np.nan
    T = dict(kf_bad=kf_bad, kf_id=(3 * np.arange(rows) + 1).astype(i32), parent=parent, conn_w=conn_w, ord_kf=ord_kf, ord_w=ord_w, n_ord=n_ord,
             loop_start=loop_start, loop_kf=loop_kf, lc_start=lc_start, lc_kf=lc_kf, corrected=corrected, non_corrected=non_corrected,
             in_corrected=in_c, in_non_corrected=in_nc, flags=flags, ref_kf=ref_kf, corrected_by_kf=cby, corrected_ref=cref, Tcw=Tcw,
             world=world)
    return dict(tables=T, cur=cur, loop_row=loop_row, fix_scale=int(fix_scale), rows=rows, pcap=pcap,
                max_edges=max_edges or 8 * rows + 16, truth=truth)


H_WANT = [(8, 2, E.K_LC), (9, 0, E.K_LC), (9, 1, E.K_LC), (1, 0, E.K_TREE), (2, 1, E.K_TREE), (2, 0, E.K_COVIS), (3, 2, E.K_TREE),
          (4, 3, E.K_TREE), (5, 4, E.K_TREE), (5, 3, E.K_LOOP), (5, 8, E.K_COVIS), (7, 5, E.K_TREE), (7, 4, E.K_COVIS), (8, 7, E.K_TREE),
          (9, 8, E.K_TREE), (9, 7, E.K_COVIS)]
H_REPORT = [E.OK, 9, 3, 8, 1, 4, 2, 1]                                         # status, vertices, the four kinds, inserted, gated


def scene_H():
    """Row 6 is bad; rows 5 and 8 have swapped mnIds; (5, 3) is an old loop edge; row 4's weights are all >= 100."""
    b = ring(10, 3, npts=12)
    T = b["tables"]
    rows = 10
    W = {(1, 0): 120, (2, 1): 130, (3, 2): 110, (4, 3): 105, (5, 4): 140, (7, 5): 150, (8, 7): 125, (9, 8): 135, (2, 0): 101, (3, 1): 99,
         (4, 2): 100, (5, 3): 115, (7, 4): 102, (8, 5): 108, (9, 7): 111, (7, 6): 130, (9, 0): 40, (9, 1): 105, (8, 1): 90, (8, 2): 100,
         (5, 2): 20, (7, 3): 30}
    conn_w = np.zeros((rows, rows), i32)
    for (a, c), w in W.items():
        conn_w[a][c] = conn_w[c][a] = w
    T["conn_w"] = conn_w
    T["ord_kf"], T["ord_w"], T["n_ord"] = _ordered(conn_w)
    T["kf_bad"] = np.array([0, 0, 0, 0, 0, 0, 1, 0, 0, 0], u8)
    T["kf_id"] = np.array([0, 1, 2, 3, 4, 8, 6, 7, 5, 9], i32)
    T["parent"] = np.array([-1, 0, 1, 2, 3, 4, 5, 5, 7, 8], i32)
    T["loop_start"], T["loop_kf"], _ = _csr({5: [3], 3: [5]}, rows)
    T["lc_start"], T["lc_kf"], _ = _csr({8: [1, 2], 9: [0, 1]}, rows)
    for k in ("corrected", "non_corrected", "in_corrected", "in_non_corrected"):
        T[k] = T[k].copy()
    T["in_corrected"][6] = T["in_non_corrected"][6] = 0
    for k in ("ref_kf", "corrected_ref"):
        T[k] = np.where(T[k] == 6, 5, T[k]).astype(i32)
    return b


CASES = ["H", "r6", "r6_fix", "p4", "p5", "p8", "p9", "p10", "r37", "bad9", "pts", "nullv", "edges_plus_one", "cap513"]
HOST_FORM_CASES = [c for c in CASES if c != "nullv"]
SLOW = {"r37"}


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "H":
        return scene_H()
    if name in ("r6", "r6_fix", "pts"):
        return ring(6, 11, band=1, fix_scale=name == "r6_fix", npts=40 if name == "pts" else 8, group=1)
    if name in ("p4", "p5"):
        return ring(int(name[1:]), 20 + int(name[1:]), band=1, npts=6, group=1)
    if name in ("p8", "p9", "p10"):
        return ring(int(name[1:]), 20 + int(name[1:]), npts=6)
    if name == "r37":
        return ring(37, 37, band=3, npts=30, loops={20: [4], 4: [20]})
    if name == "bad9":
        return ring(9, 9, bad=(4,), npts=16)
    if name == "nullv":
        return ring(9, 9, bad=(4,), npts=16, null_entries=True)
    if name == "edges_plus_one":
        b = ring(8, 28, npts=6)
        full = run_seqref(b)["report"]
        return dict(b, max_edges=sum(full[2:6]) - 1)
    if name == "cap513":
        b = ring(513, 1, band=0, npts=0, group=0)
        return b
    if name == "singular":
        return ring(7, 5, npts=6, nan_row=3)
    if name == "ring12":
        return ring(12, 12, band=2, npts=0, drift=(0.002, -0.004, 0.001, 0.01))
    raise KeyError(name)


def run_seqref(b, info=None):
    return E.optimize_essential_graph(b["tables"], b["cur"], b["loop_row"], bool(b["fix_scale"]), max_edges=b["max_edges"], info=info)


def prefilled(b):
    fill = lambda count, dt: np.full(max(count, 1) * np.dtype(dt).itemsize, SENTINEL, u8).view(dt)[:count]  # noqa: E731
    return dict(point_list=fill(b["pcap"], i32), Scw=fill(b["rows"] * 8, f64).reshape(-1, 8), Swc=fill(b["rows"] * 8, f64).reshape(-1, 8),
                report=fill(16, i32))


def as_arrays(b, r):
    """The seqref's answer as the arrays a call leaves: what it does not write keeps the sentinel / the input."""
    o = prefilled(b)
    o["Tcw"], o["world"] = b["tables"]["Tcw"].copy(), b["tables"]["world"].copy()
    o["report"][:] = r["report"]
    if r["report"][0] != E.CAPACITY:
        for row, v in r["Tcw"].items():
            o["Tcw"][row] = v
        for p, v in r["world"].items():
            o["world"][p] = v
        o["point_list"][:len(r["point_list"])] = r["point_list"]
        for row in r["Scw"]:
            o["Scw"][row], o["Swc"][row] = r["Scw"][row], r["Swc"][row]
    return o


@functools.lru_cache(maxsize=None)
def reference(name):
    b = case(name)
    info = {}
    r = run_seqref(b, info)
    o = as_arrays(b, r)
    o["raw"], o["info"] = r, info
    return o


def assert_same(got, ref, what, nan_ok=False):
    for k in ("report", "point_list", "Tcw", "world", "Scw", "Swc"):
        g, w = np.ascontiguousarray(got[k]).reshape(-1), np.ascontiguousarray(ref[k]).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if nan_ok and g.dtype.kind == "f":
            both = np.isnan(g) & np.isnan(w)
            g, w = np.where(both, 0, g), np.where(both, 0, w)
        assert g.tobytes() == w.tobytes(), "%s: %s differs (%s vs %s)" % (what, k, g[:12], w[:12])


# ---------------------------------------------------------------------------------------------------------------------
# the rules
def test_hand_built_graph_edge_list_and_counts():
    ref = reference("H")
    got = [(i, j, k) for (i, j, _m, k) in ref["info"]["edges"]]
    assert got == H_WANT
    assert ref["raw"]["report"][:8] == H_REPORT and ref["raw"]["report"][10] == 56 and ref["raw"]["report"][12] == 0


def test_covisibles_by_weight_returns_nothing_when_no_weight_is_below_100():
    T = case("H")["tables"]
    assert E.covisibles_by_weight(T, 4) == []                                  # 140, 105, 102, 100: upper_bound finds end()
    assert E.covisibles_by_weight(T, 2) == [1, 3, 0, 4, 8]                     # ... | 20


def test_six_rows_one_loop_connection_and_the_gate():
    r = reference("r6")["raw"]["report"]
    assert r[:8] == [E.OK, 6, 3, 5, 0, 0, 2, 0]                                # (5, 1) and (4, 0) are covisible at >= 100, and inserted
    r = reference("p9")["raw"]["report"]
    assert r[2] == 3 and r[7] == 1 and r[3] == 8                               # (cur - 1, 1) is gated, (cur, 0) is exempt at weight 60


def test_null_vertices_are_skipped_and_counted():
    r, r0 = reference("nullv")["raw"]["report"], reference("bad9")["raw"]["report"]
    assert r[12] == 3 and r0[12] == 0
    assert r[3] == r0[3] - 1 and r[2] == r0[2] and r[4] == 0


def test_bad_row_keeps_its_bytes_and_its_children_hang_elsewhere():
    ref, b = reference("bad9"), case("bad9")
    assert ref["raw"]["report"][1] == 8 and 4 not in ref["raw"]["Tcw"]
    assert ref["Tcw"][4].tobytes() == b["tables"]["Tcw"][4].tobytes()
    assert ref["Scw"][4].tobytes() == prefilled(b)["Scw"][4].tobytes()


@pytest.mark.parametrize("sigma,theta", [(0.0, 0.0), (0.0, 0.7), (0.3, 0.0), (-0.2, 1.9), (3e-6, 2e-6), (0.4, 3.0)])
def test_sim3_log_inverts_exp_on_all_four_branches(sigma, theta):
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    u = list(axis * theta) + [0.4, -1.1, 0.25, sigma]
    S = sim3_exp(u)
    back = E.sim3_log(S)
    assert np.allclose(back, u, rtol=0, atol=2e-9 if theta > 2.5 else 1e-11)
    R = np.array(to_R(S[0:4])).reshape(3, 3)
    d = 0.5 * (np.trace(R) - 1)
    assert (abs(back[6]) < 1e-5) == (abs(sigma) < 1e-5) and (d > 1 - 1e-5) == (theta < 4e-3)


def _ulps(a, b):
    return abs(a - b) / math.ulp(b) if b == b and abs(b) != float("inf") else (0.0 if (a == b or (a != a and b != b)) else float("inf"))


def test_det_log64_and_det_acos64_within_one_ulp_of_libm():
    rng = np.random.default_rng(0)
    xs = list(np.exp(rng.uniform(-30, 30, 20000))) + list(1 + rng.uniform(-1e-5, 1e-5, 5000)) + list(rng.uniform(0.5, 2.0, 20000))
    xs += [1.0, 0.5, 2.0, 1.38, 1.42, 1.4142112731933594, 5e-324, 1e-310, 1.7976931348623157e308, 1 + 2.0 ** -21, 1 - 2.0 ** -21]
    assert max(_ulps(E.det_log64(float(x)), math.log(float(x))) for x in xs) <= 1.0
    assert E.det_log64(0.0) == -math.inf and math.isnan(E.det_log64(-1.0)) and E.det_log64(math.inf) == math.inf
    ys = list(rng.uniform(-1, 1, 40000)) + list(1 - np.exp(rng.uniform(-30, 0, 5000))) + [0.0, 0.5, -0.5, 1.0, -1.0, 1e-20, 0.99999, -0.99999]
    assert max(_ulps(E.det_acos64(float(y)), math.acos(float(y))) for y in ys) <= 1.0
    assert math.isnan(E.det_acos64(1.5))


def test_fix_scale_keeps_every_scale_and_the_scale_unknown_sees_lambda_alone():
    ref, free = reference("r6_fix"), reference("r6")
    b = case("r6_fix")
    s_in = {r: (b["tables"]["corrected"][r][7] if b["tables"]["in_corrected"][r] else 1.0) for r in range(6)}
    for r, S in ref["info"]["est"].items():
        assert S[7] == s_in[r]
    assert any(S[7] != s_in[r] for r, S in free["info"]["est"].items())
    D = E.perturbations(True)
    assert D[12] == D[13] == sim3_exp([0.0] * 7)                               # the scale column of every Jacobian is exactly zero


def test_points_take_both_branches_and_a_point_without_reference_stays():
    ref, b = reference("pts"), case("pts")
    T = b["tables"]
    moved = [p for p in ref["raw"]["world"]]
    by_ref = [p for p in moved if T["corrected_by_kf"][p] == b["cur"]]
    assert by_ref and len(by_ref) < len(moved)
    n = b["pcap"] - 3
    assert ref["raw"]["point_list"] == [p for p in range(b["pcap"]) if T["flags"][p] & 1]
    for p in (n, n + 2):
        assert p in ref["raw"]["point_list"] and p not in ref["raw"]["world"]
    for p in range(b["pcap"]):
        if not T["flags"][p] & 1:
            assert ref["world"][p].tobytes() == T["world"][p].tobytes()
    # the corrected-reference branch reads corrected_ref, not ref_kf
    p = by_ref[0]
    r = int(T["corrected_ref"][p])
    Y = E.sim3_map(ref["raw"]["Swc"][r], E.sim3_map(ref["raw"]["Scw"][r], [float(v) for v in T["world"][p]]))
    assert np.array(Y, f32).tobytes() == ref["world"][p].tobytes()


def test_the_three_statuses():
    assert reference("r37")["raw"]["report"][0] == E.OK
    for name in ("edges_plus_one", "cap513"):
        ref, b = reference(name), case(name)
        assert ref["raw"]["report"][0] == E.CAPACITY and set(ref["raw"]) == {"report"}
        assert ref["Tcw"].tobytes() == b["tables"]["Tcw"].tobytes()
    assert reference("cap513")["raw"]["report"][:3] == [E.CAPACITY, 513, 0]
    r = reference("singular")["raw"]
    assert r["report"][0] == E.SINGULAR and r["report"][9] == r["report"][8]   # one trial per iteration: rho is a NaN
    b = case("singular")
    for row in (0, 1, 5, 6):                                                   # the estimates are unchanged and are written back
        S = E.sim3_from_Tcw(b["tables"]["Tcw"][row]) if not b["tables"]["in_corrected"][row] else list(b["tables"]["corrected"][row])
        assert reference("singular")["info"]["est"][row] == S


def test_scenes_reach_accepted_and_rejected_trials_and_the_qmax_stop():
    for name in ("H", "r37", "p9"):
        ref = reference(name)
        tr = ref["info"]["trace"]
        good = [g for (_i, _q, g) in tr]
        assert good[0] and not all(good) and tr[-1][1] == 9, name               # the tenth trial of an iteration ends it: qmax == 10
        assert ref["raw"]["report"][8:10] == [tr[-1][0] + 1, len(tr)], name


def test_judge_rejects_on_a_hand_worked_state(tmp_path):
    """current 2.0, the trial's chi2 3.0, computeScale 0.5 - 1e-3: rho = (2 - 3) / 0.5 = -2: lambda 0.25 * 2, ni 4, the estimate
    stays, another trial; with qmax already 9 the iteration ends and the optimisation stops (qmax == 10)."""
    exe = _compile(tmp_path, "judge", JUDGE_MAIN, [])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0.5", "4", "2", "0", "1", "2", "-2", "1", "0"], out


JUDGE_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "orbhip.h"
#include "orbhip_essgraph_core.h"
using namespace orbhip;
int main()
{
    EgWs W; EgState S; memset(&W, 0, sizeof W); memset(&S, 0, sizeof S); W.S = &S;
    S.phase = kEgTrial; S.ok2 = 1; S.it = 1; S.lam = 0.25; S.ni = 2.0; S.current = S.ini = 2.0; S.qmax = 0; S.cur = 0;
    eg_lm_judge(W, 3.0, 0.5 - 1e-3);
    printf("%.17g %.17g %.17g %d %d %d %.17g ", S.lam, S.ni, S.current, S.cur, S.qmax, S.phase, S.rho);
    S.qmax = 9; eg_lm_judge(W, 3.0, 0.5 - 1e-3);
    printf("%d %d\n", S.phase == kEgFinal, S.status);
    return 0;
}
"""


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the shared core
def _compile(tmp_path, name, text, extra):
    src = os.path.join(str(tmp_path), name + ".cpp")
    with open(src, "w") as f:
        f.write(text)
    exe = os.path.join(str(tmp_path), name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), src, "-o", exe] + extra, check=True)
    return exe


@functools.lru_cache(maxsize=None)
def host_program(sanitize=False):
    d = tempfile.mkdtemp(prefix="essgraph_host_")
    exe = os.path.join(d, "essgraph_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "essgraph_host.cpp"),
                    "-o", exe], check=True)
    return exe


def pack(b, o, max_trials=0):
    t = b["tables"]
    n_loop, n_lc = int(t["loop_start"][-1]), int(t["lc_start"][-1])
    h = np.zeros(16, i32)
    h[:9] = [b["rows"], b["pcap"], b["cur"], b["loop_row"], b["fix_scale"], b["max_edges"], n_loop, n_lc, max_trials]
    parts = [h, t["kf_bad"], t["kf_id"], t["parent"], t["conn_w"], t["ord_kf"], t["ord_w"], t["n_ord"], t["loop_start"], t["loop_kf"][:n_loop],
             t["lc_start"], t["lc_kf"][:n_lc], t["corrected"], t["non_corrected"], t["in_corrected"], t["in_non_corrected"], t["flags"],
             t["ref_kf"], t["corrected_by_kf"], t["corrected_ref"], t["Tcw"], t["world"]]
    parts += [o[k] for k in OUT_KEYS]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def unpack(b, raw):
    off = 0
    got = {}
    for k, dt, cnt in (("Tcw", f32, b["rows"] * 12), ("world", f32, b["pcap"] * 3), ("point_list", i32, b["pcap"]), ("Scw", f64, b["rows"] * 8),
                       ("Swc", f64, b["rows"] * 8), ("report", i32, 16)):
        got[k] = np.frombuffer(raw, dt, cnt, off)
        off += got[k].nbytes
    got["Tcw"], got["world"] = got["Tcw"].reshape(-1, 12), got["world"].reshape(-1, 3)
    got["Scw"], got["Swc"] = got["Scw"].reshape(-1, 8), got["Swc"].reshape(-1, 8)
    return got, off


def run_host(b, tmp_path, tag, sanitize=False, fill=0):
    fin, fout = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    fin.write_bytes(pack(b, prefilled(b), max_trials=200))
    subprocess.run([host_program(sanitize), str(fin), str(fout), str(fill)], check=True)
    raw = fout.read_bytes()
    got, off = unpack(b, raw)
    nt = int(np.frombuffer(raw, i32, 1, off)[0])
    got["tried"] = np.frombuffer(raw, f64, -1, off + 4).reshape(nt, -1, 8) if nt else np.zeros((0, 0, 8))
    return got


@pytest.mark.parametrize("name,fill", with_fills(CASES + ["singular"]))
def test_host_build_matches_seqref(name, fill, tmp_path):
    """`fill`: the byte the workspace holds before the run (the device's slot is never cleared)."""
    b, ref = case(name), reference(name)
    got = run_host(b, tmp_path, name, fill=fill)
    assert_same(got, ref, name, nan_ok=name == "singular")
    tried = ref["info"].get("tried", [])
    want = np.array(tried, f64).reshape(len(tried), -1, 8) if tried else np.zeros((0, 0, 8))
    assert got["tried"].shape == want.shape, name
    if name == "singular":
        assert np.array_equal(got["tried"], want, equal_nan=True)
    else:
        assert got["tried"].tobytes() == want.tobytes(), name


def test_host_program_runs_clean_under_asan_and_ubsan(tmp_path):
    for name in CASES + ["singular"]:
        if name in SLOW:
            continue
        for fill in FILLS:
            got = run_host(case(name), tmp_path, "san_" + name, sanitize=True, fill=fill)
            assert_same(got, reference(name), (name, fill), nan_ok=name == "singular")


# ---------------------------------------------------------------------------------------------------------------------
# the textbook restatement: matrices, libm, numpy.linalg.solve
def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)


def _tb_from(S):
    return np.array(to_R(S[0:4]), f64).reshape(3, 3), np.array(S[4:7], f64), float(S[7])


def _tb_mul(a, b):
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def _tb_inv(a):
    return a[0].T, a[0].T @ (-1.0 / a[2] * a[1]), 1.0 / a[2]


def _tb_coeffs(theta, sigma, s):
    eps = 1e-5
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            return 0.5, 1.0 / 6.0, C
        return (1 - math.cos(theta)) / theta ** 2, (theta - math.sin(theta)) / theta ** 3, C
    C = (s - 1) / sigma
    if theta < eps:
        return ((sigma - 1) * s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3, C
    a, b, c = s * math.sin(theta), s * math.cos(theta), theta ** 2 + sigma ** 2
    return (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2, C


def _tb_exp(u):
    w, up, sigma = np.array(u[0:3]), np.array(u[3:6]), u[6]
    theta, s, Om = float(np.linalg.norm(w)), math.exp(sigma), _skew(u[0:3])
    if theta < 1e-5:
        R = np.eye(3) + Om + Om @ Om
    else:
        R = np.eye(3) + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / theta ** 2 * (Om @ Om)
    A, B, C = _tb_coeffs(theta, sigma, s)
    return R, (A * Om + B * (Om @ Om) + C * np.eye(3)) @ up, s


def _tb_log(S):
    R, t, s = S
    sigma = math.log(s)
    d = 0.5 * (np.trace(R) - 1)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if d > 1 - 1e-5:
        omega, theta = 0.5 * dR, 0.0
    else:
        theta = math.acos(d)
        omega = theta / (2 * math.sqrt(1 - d * d)) * dR
    A, B, C = _tb_coeffs(theta if d <= 1 - 1e-5 else 0.0, sigma, s)
    Om = _skew(omega)
    return np.concatenate([omega, np.linalg.solve(A * Om + B * (Om @ Om) + C * np.eye(3), t), [sigma]])


def _textbook(b, ref):
    edges = [(i, j, _tb_from(m)) for (i, j, m, _k) in ref["info"]["edges"]]
    vrows = sorted(ref["raw"]["Scw"])
    est = {r: _tb_from(ref["raw"]["Scw"][r]) for r in vrows}
    free = [r for r in vrows if r != b["loop_row"]]
    fidx = {r: f for f, r in enumerate(free)}
    n = 7 * len(free)
    fix = bool(b["fix_scale"])

    def err(e, X):
        return _tb_log(_tb_mul(_tb_mul(e[2], X[e[0]]), _tb_inv(X[e[1]])))

    def chi(X):
        return sum(float(err(e, X) @ err(e, X)) for e in edges)

    def plus(u, S):
        u = list(u)
        if fix:
            u[6] = 0.0
        return _tb_mul(_tb_exp(u), S)

    lam, ni, n_bad, its, trace = 1e-16, 2.0, 0, 0, []
    for it in range(20):
        H, g = np.zeros((n, n)), np.zeros(n)
        for e in edges:
            r0 = err(e, est)
            Js = {}
            for end in (0, 1):
                row = e[end]
                if row not in fidx:
                    continue
                J = np.zeros((7, 7))
                for d in range(7):
                    u = np.zeros(7)
                    u[d] = 1e-9
                    Xp, Xm = dict(est), dict(est)
                    Xp[row], Xm[row] = plus(u, est[row]), plus(-u, est[row])
                    J[:, d] = (err(e, Xp) - err(e, Xm)) / 2e-9
                Js[fidx[row]] = J
            for f1, J1 in Js.items():
                g[7 * f1:7 * f1 + 7] += J1.T @ -r0
                for f2, J2 in Js.items():
                    H[7 * f1:7 * f1 + 7, 7 * f2:7 * f2 + 7] += J1.T @ J2
        current = ini = chi(est)
        rho, qmax = 0.0, 0
        while True:
            x = np.linalg.solve(H + lam * np.eye(n), g)
            if fix:
                x[6::7] = 0.0
            tried = dict(est)
            for r in free:
                tried[r] = plus(x[7 * fidx[r]:7 * fidx[r] + 7], est[r])
            temp = chi(tried)
            rho = (current - temp) / (float(x @ (lam * x + g)) + 1e-3)
            good = rho > 0 and math.isfinite(temp)
            trace.append((it, qmax, good))
            if good:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam, ni, current, est = lam * max(1.0 / 3.0, alpha), 2.0, temp, tried
            else:
                lam, ni = lam * ni, ni * 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        its += 1
        if qmax == 10 or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    return est, trace, its


TEXTBOOK_CASES = ["H", "r6", "r6_fix", "p4", "p5", "p8", "p9", "p10", "bad9", "nullv", "r37"]
# scene: (trials whose decisions must agree, why the later ones need not)
TEXTBOOK_EXEMPT = {"nullv": (3, "the null parent cuts the graph in two, the loop connections alone hold rows 5-8, and chi2 reaches its floor of "
                               "3.0e-14 in three steps; the fourth step moves it in the ninth digit, below the 1e-7 noise of the numeric "
                               "Jacobian, so its sign -- accept or reject -- is not determined")}
_worst = dict(R=0.0, t=0.0, s=0.0)


@pytest.mark.parametrize("name", TEXTBOOK_CASES)
def test_textbook_distance(name):
    b, ref = case(name), reference(name)
    est, trace, its = _textbook(b, ref)
    if name in TEXTBOOK_EXEMPT:
        k = TEXTBOOK_EXEMPT[name][0]
        assert trace[:k] == ref["info"]["trace"][:k], name
    else:
        assert trace == ref["info"]["trace"] and its == ref["raw"]["report"][8], name
    dR = dt = ds = 0.0
    for r, S in ref["info"]["est"].items():
        R, t, s = _tb_from(S)
        dR, dt, ds = max(dR, float(np.abs(R - est[r][0]).max())), max(dt, float(np.abs(t - est[r][1]).max())), max(ds, abs(s - est[r][2]))
    for k, v in (("R", dR), ("t", dt), ("s", ds)):
        _worst[k] = max(_worst[k], v)
    print("textbook distance %s: R %.2e t %.2e s %.2e (worst so far R %.2e t %.2e s %.2e)" % (name, dR, dt, ds, _worst["R"], _worst["t"], _worst["s"]))
    assert dR <= TOL["R"] and dt <= TOL["t"] and ds <= TOL["s"]


def _truth_distance(b, est):
    dR = dt = 0.0
    for r, S in est.items():
        R, t, s = S if isinstance(S, tuple) else _tb_from(S)
        Rt, tt, _ = _tb_from(b["truth"][r])
        dR, dt = max(dR, float(np.abs(R - Rt).max())), max(dt, float(np.abs(t / s - tt).max()))
    return dR, dt


def test_noise_free_ring_returns_to_ground_truth():
    """12 key frames, a rotation drift of 0.0046 rad and a scale drift of 1 % per step, closed with the true loop Sim3."""
    b, ref = case("ring12"), reference("ring12")
    before = _truth_distance(b, {r: E.sim3_from_Tcw(b["tables"]["Tcw"][r]) for r in ref["info"]["est"]})
    tb = _truth_distance(b, _textbook(b, ref)[0])
    got = _truth_distance(b, ref["info"]["est"])
    print("ring12 against ground truth: before R %.2e t %.2e, restatement R %.2e t %.2e, seqref R %.2e t %.2e" % (before + tb + got))
    assert tb[0] <= RING_MEASURED["R"] and tb[1] <= RING_MEASURED["t"]         # the bound below is the restatement's own residual
    assert got[0] <= RING_TOL["R"] and got[1] <= RING_TOL["t"]
    assert before[0] > 4 * got[0] and before[1] > 10 * got[1]              # before: R 4.0e-2, t 0.88: most of the drift is gone
