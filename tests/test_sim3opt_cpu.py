"""Optimizer::OptimizeSim3 over tables: the sequential reference (tests/seqref/sim3opt.py) alone, no GPU.

The rules of src/Optimizer.cc:1046-1241 are pinned by hand-worked cases: every skip reason (and the one Sim3Solver has that
this function has not), i2 taken from the observation table, a pair bad through e21 only, a NaN pair kept, exactly 10
survivors against 9, no pair at all, the fixed scale, the iteration allowance of round 2.  Scenes with a known Sim3 check the
whole and are the inputs of test_sim3opt_gpu.py and test_cpp_sim3opt_gpu.py, with the reference answers computed once per
process.  An independent restatement (analytic Jacobians, rotation matrices, numpy.linalg.solve, libm exp) must find the
same inlier sets; its distance in R, t and s is printed and bounded (MEASURED below).  A host build of
orbhip_sim3opt_core.h (tests/cpp/sim3opt_host.cpp) must match the reference bit for bit, det_exp64 included.

One rule could not be made to show in an output of a scene and is held below the outputs: the check reads the error at the
last TRIED estimate.  After a rejected last trial the two estimates are too close to move a chi2 across th2 in every scene
tried.  classify() is checked on a hand-worked state (an estimate that keeps every pair, a tried estimate that removes some),
in the seqref and through the host program; optimize_sim3 is checked to hand it the tried estimate; and the host build must
leave the seqref's estimate and tried estimate bit for bit.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import test_sim3_cpu as K
from orb_slam2_comment_amd import capi
from helpers import with_fills
from seqref import sim3 as S3
from seqref import sim3opt as Q

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (K.CAM["fx"], K.CAM["fy"], K.CAM["cx"], K.CAM["cy"])
INV_SIGMA2 = (1.0 / K.SIGMA2.astype(f64)).astype(f32)
SENTINEL = 0xA5
TH2 = 10.0
# What test_textbook_distance prints: the largest distance of the textbook restatement over the scene cases (DESIGN.md
# section 3).  Where both routes run into the noise floor of the numeric Jacobian the distance is 1.6e-8 (R), 1.6e-8 m (t) and
# 6e-8 (s); where both stop on g2o's rule "three iterations that gain less than 0.1 %" they stop at different points of a
# valley that is as flat as that rule (candidate 2 of both batches with the scale free), which is what the maxima show.
MEASURED = dict(R=4.4e-6, t=5.5e-5, s=2.6e-4)
TOL = {k: 10 * v for k, v in MEASURED.items()}


# ---- scenes -------------------------------------------------------------------------------------------------------------
def observe(sc, seed, noise=0.3):
    """Fills the key points of a scene of test_sim3_cpu.build: every slot that holds a point sees it where its key frame
    projects it, plus `noise` pixels (uniform), so that pairs under the scene's Sim3 are inliers of a few tenths of a pixel."""
    rng = np.random.default_rng(seed)
    T = sc["T"]
    kps = T["kps"].copy()
    fx, fy, cx, cy = CAM
    for row in range(sc["rows"]):
        Tr = T["Tcw"][row].astype(f64).reshape(3, 4)
        for j in range(sc["cap"]):
            p = int(T["slot_point"][row, j])
            if p < 0:
                continue
            X = Tr[:, :3] @ T["world"][p].astype(f64) + Tr[:, 3]
            kps["x"][row, j] = fx * X[0] / X[2] + cx + rng.uniform(-noise, noise)
            kps["y"][row, j] = fy * X[1] / X[2] + cy + rng.uniform(-noise, noise)
    sc = dict(sc)
    sc["T"] = dict(T, kps=kps)
    return sc


def sim3_record(model, d_angle=0.0, d_t=0.0, d_s=1.0, C=1):
    """[C, 16] float32: the model (s, R, t) of test_sim3_cpu turned by d_angle, moved by d_t and scaled by d_s."""
    s, R, t = model
    R = K.rot([0.5, -0.3, 0.8], d_angle) @ R
    rec = np.zeros(16, f32)
    rec[:9] = R.reshape(9)
    rec[9:12] = t + d_t
    rec[12] = s * d_s
    return np.tile(rec, (C, 1))


def scene(counts, n1, cap, seed, model=K.SIM3_A, seed_obs=5):
    """One candidate per entry of counts = (pairs under the model, random partners)."""
    cands = [K._seq(0, g, model) + K._seq(g, b, None) for g, b in counts]
    return observe(K.build(cands, n1, cap, seed), seed_obs)


def run_seqref(sc, sim3, form=S3.MATCH_POINTS, fix_scale=False, select=None, infos=None, team=Q.TEAM):
    """dict(matched12, S12, Scw, report) with the sentinel where nothing is written."""
    Cn, cap = sc["C"], sc["cap"]
    m = (sc["m_points"] if form == S3.MATCH_POINTS else sc["m_slots"]).copy()
    S12 = np.full(Cn * 64, SENTINEL, u8).view(f64).reshape(Cn, 8).copy()
    Scw = np.full(Cn * 48, SENTINEL, u8).view(f32).reshape(Cn, 12).copy()
    rep = np.full(Cn * 32, SENTINEL, u8).view(i32).reshape(Cn, 8).copy()
    for c in range(Cn):
        if select is not None and not select[c]:
            rep[c, 0] = Q.SKIPPED
            continue
        info = {}
        r, s12, scw = Q.optimize_sim3(sc["T"], sc["cur"], int(sc["kf_index"][c]), CAM, m[c], form, INV_SIGMA2, sim3[c], TH2,
                                      fix_scale, team, info)
        rep[c], S12[c] = r, s12
        if scw is not None:
            Scw[c] = scw
        if infos is not None:
            infos.append(info)
    return dict(matched12=m, S12=S12, Scw=Scw, report=rep)


BATCH_A = ((0, 0), (9, 0), (11, 1))                  # 0, 9 and 12 pairs
BATCH_B = ((50, 14), (65, 0), (200, 57))             # 64, 65 (the second wavefront holds one pair) and 257 (lane 0 holds two)


def _case(name):
    if name in ("A", "B"):
        sc = scene(BATCH_A if name == "A" else BATCH_B, 300, 512, 61 if name == "A" else 62)
        return sc, sim3_record(K.SIM3_A, 0.01, 0.02, 1.01, 3)
    if name == "A_alone":                            # candidate 2 of A as a batch of one
        sc, sim3 = case("A")
        one = dict(sc, C=1, kf_index=sc["kf_index"][2:3], m_points=sc["m_points"][2:3], m_slots=sc["m_slots"][2:3])
        return one, sim3[2:3]
    if name == "nan_pair":                           # the scene of test_nan_pair_is_kept: no factorisation succeeds
        sc = small()
        sc["T"]["world"][int(sc["m_points"][0][3])] = np.nan
        return sc, sim3_record(K.SIM3_A)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    return _case(name)


@functools.lru_cache(maxsize=None)
def reference(name, form=S3.MATCH_POINTS, fix_scale=False, select=None):
    sc, sim3 = case(name)
    return run_seqref(sc, sim3, form, fix_scale, select)


def assert_same(got, want, what):
    for k in ("matched12", "S12", "Scw", "report"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (what, k)


# ---- rule 1: the pairs ----------------------------------------------------------------------------------------------------
def small(counts=((20, 0),), seed=70, **kw):
    return scene(counts, 40, 64, seed, **kw)


def test_every_skip_reason_and_the_slot_order():
    skip = ([(0, K.SIM3_A, {"nomatch"}), (1, K.SIM3_A, set()), (2, K.SIM3_A, set()), (3, K.SIM3_A, set()),
             (4, K.SIM3_A, {"absent"}), (5, K.SIM3_A, {"unobserved"}), (6, K.SIM3_A, {"empty_slot"}), (7, K.SIM3_A, set())]
            + K._seq(8, 12, K.SIM3_A))
    sc = observe(K.build([skip], 24, 64, 11, no_point={1}, p1_absent={2}, p1_unobserved={3}, p1_twice={7}), 5)
    sc["T"]["n"][sc["cur"]] = 18                     # slots 18, 19 lie behind n[cur]
    for form, m in ((S3.MATCH_POINTS, sc["m_points"]), (S3.MATCH_SLOTS, sc["m_slots"])):
        pairs = Q.build_pairs(sc["T"], sc["cur"], 2, m[0], form, INV_SIGMA2)
        # 3: the first point has no observation in the current key frame, which Sim3Solver skips and this function keeps
        assert [p.slot for p in pairs] == [3, 7] + list(range(8, 18)), form
    solver = S3.setup(sc["T"], sc["cur"], 2, sc["m_points"][0], S3.MATCH_POINTS, K.cam_dict(), K.SIGMA2)
    assert 3 not in solver["slot1"].tolist()
    # obs1 is key point i itself (for slot 7 the observation table names slot 14 first)
    p7 = [p for p in pairs if p.slot == 7][0]
    k = sc["T"]["kps"][sc["cur"]][7]
    assert p7.o1 == [float(k["x"]), float(k["y"])] and p7.inv1 == float(INV_SIGMA2[int(k["octave"])])


def test_i2_comes_from_the_observation_table():
    sc = small()
    T = sc["T"]
    kf = 2
    j = int(sc["m_slots"][0][4])
    p2 = int(T["slot_point"][kf][j])
    free = [s for s in range(sc["cap"]) if T["slot_point"][kf][s] < 0][0]
    o = int(T["obs_start"][p2])
    assert T["obs_kf"][o] == kf and T["obs_idx"][o] == j
    T["obs_idx"][o] = free
    T["kps"][kf][free] = T["kps"][kf][j]
    T["kps"]["octave"][kf][free] = (int(T["kps"]["octave"][kf][j]) + 1) % 8
    T["kps"]["x"][kf][j] += 50.0                     # what the slot holds would make the pair an outlier
    pairs = Q.build_pairs(T, sc["cur"], kf, sc["m_slots"][0], S3.MATCH_SLOTS, INV_SIGMA2)
    p = [q for q in pairs if q.slot == 4][0]
    assert p.i2 == free and p.inv2 == float(INV_SIGMA2[int(T["kps"]["octave"][kf][free])])
    out = run_seqref(sc, sim3_record(K.SIM3_A), S3.MATCH_SLOTS)
    assert out["report"][0].tolist()[:4] == [Q.OK, 20, 0, 20] and out["matched12"][0][4] == j


# ---- rule 2, 7: errors and the check ----------------------------------------------------------------------------------
def test_sim3_algebra():
    S = Q.from_sim3(sim3_record(K.SIM3_A)[0])
    s, R, t = K.SIM3_A
    X = [0.3, -0.2, 4.0]
    r = Q.quat_rot(S[0:4], X)
    got = np.array([S[7] * r[i] + S[4 + i] for i in range(3)])
    assert np.allclose(got, f32(s) * (R.astype(f32).astype(f64) @ X) + t.astype(f32), atol=1e-6)
    Si = Q.sim3_inverse(S)
    r = Q.quat_rot(Si[0:4], got.tolist())
    assert np.allclose([Si[7] * r[i] + Si[4 + i] for i in range(3)], X, atol=1e-6)
    I = Q.sim3_mul(S, Si)
    assert np.allclose(I, [0, 0, 0, 1, 0, 0, 0, 1], atol=1e-6)
    # the four branches of Sim3(update) against the closed form exp of the 4x4 generator
    for u in ([1e-7, 0, 0, 0.1, 0.2, 0.3, 0.0], [0.2, -0.1, 0.3, 0.1, 0.2, 0.3, 1e-7], [1e-7, 0, 0, 0.1, 0.2, 0.3, 0.2],
              [0.2, -0.1, 0.3, 0.1, 0.2, 0.3, -0.4]):
        E = Q.sim3_exp(u)
        G = np.zeros((4, 4))
        G[:3, :3] = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]) + u[6] * np.eye(3)
        G[:3, 3] = u[3:6]
        M, term = np.eye(4), np.eye(4)
        for k in range(1, 30):
            term = term @ G / k
            M = M + term
        got = np.eye(4)
        got[:3, :3] = E[7] * np.array(Q.to_R(E[0:4])).reshape(3, 3)
        got[:3, 3] = E[4:7]
        assert np.allclose(got, M, atol=1e-9), u
    assert Q.sim3_exp([0.0] * 7) == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def test_pair_bad_through_e21_only():
    sc = small()
    kf, slot = 2, 6
    i2 = int(sc["m_slots"][0][slot])
    sc["T"]["kps"]["x"][kf][i2] += 6.0
    sc["T"]["kps"]["octave"][kf][i2] = 0
    infos = []
    out = run_seqref(sc, sim3_record(K.SIM3_A), infos=infos)
    assert out["report"][0].tolist()[:4] == [Q.OK, 20, 1, 19]
    assert out["matched12"][0][slot] == -1 and (out["matched12"][0][:20] >= 0).sum() == 19
    # at the estimate of round 1 the pair's e12 is an inlier of its own
    info = infos[0]
    j = [p.slot for p in info["pairs"]].index(slot)
    assert info["history"][0][j] and sum(info["history"][0]) == 1
    p = info["pairs"][j]
    S = Q.from_sim3(sim3_record(K.SIM3_A)[0])
    assert Q.chi2_of(Q.edge_error(S, p.P2, p.o1, CAM), p.inv1) < 1.0
    assert Q.chi2_of(Q.edge_error(Q.sim3_inverse(S), p.P1, p.o2, CAM), p.inv2) > 20.0


def test_nan_pair_is_kept():
    sc = small()
    slot = 3
    p2 = int(sc["m_points"][0][slot])
    sc["T"]["world"][p2] = np.nan
    out = run_seqref(sc, sim3_record(K.SIM3_A))
    rep = out["report"][0].tolist()
    assert rep[:4] == [Q.OK, 20, 0, 20]              # chi2 is NaN, NaN > th2 is false
    assert out["matched12"][0][slot] == p2
    assert rep[4] == 5 and rep[5] == 5               # no factorisation succeeds, no stopping rule fires on NaN
    assert out["S12"][0].tobytes() == np.array(Q.from_sim3(sim3_record(K.SIM3_A)[0])).tobytes()
    # a zero depth: x / 0 is an infinity, 0 / 0 a NaN, neither raises
    S = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    e = Q.edge_error(S, [1.0, 0.0, 0.0], [0.0, 0.0], (500.0, 500.0, 320.0, 240.0))
    assert e[0] == -math.inf and math.isnan(e[1])
    assert not (Q.chi2_of(e, 1.0) > 10.0)


def test_strict_double_comparison():
    p = Q.Pair()
    p.P1, p.P2, p.inv1, p.inv2 = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], 1.0, 1.0
    S = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    cam = (1.0, 1.0, 0.0, 0.0)
    th2 = float(f32(10.0))
    r = math.sqrt(10.0)
    for ox, bad in ((r, r * r > th2), (math.nextafter(r, 0.0), False), (math.nextafter(math.nextafter(r, 4.0), 4.0), True)):
        p.o1, p.o2 = [ox, 0.0], [0.0, 0.0]
        assert (Q.classify([p], [False], S, cam, th2) == [0]) == bad, ox
        assert bad == (ox * ox > th2)


# ---- rule 8 and the two rounds ----------------------------------------------------------------------------------------
def test_ten_survivors_run_round_two_nine_return_early():
    ten = run_seqref(small(((10, 2),), seed=71), sim3_record(K.SIM3_A, 0.005, 0.01, 1.005))
    assert ten["report"][0].tolist()[:4] == [Q.OK, 12, 2, 10] and ten["report"][0][5] > 0
    sc = small(((9, 2),), seed=71)
    sim3 = sim3_record(K.SIM3_A, 0.005, 0.01, 1.005)
    nine = run_seqref(sc, sim3)
    rep = nine["report"][0].tolist()
    assert rep[:4] == [Q.TOO_FEW, 11, 2, 0] and rep[4] > 0 and rep[5] == 0
    assert nine["S12"][0].tobytes() == np.array(Q.from_sim3(sim3[0])).tobytes()     # the input, not the estimate of round 1
    assert (nine["Scw"][0].view(u8) == SENTINEL).all()
    assert nine["matched12"][0][9] == -1 and nine["matched12"][0][10] == -1 and (nine["matched12"][0][:9] >= 0).all()


def test_no_pair_at_all():
    sc = small(((0, 0),))
    sim3 = sim3_record(K.SIM3_A)
    out = run_seqref(sc, sim3)
    assert out["report"][0].tolist() == [Q.TOO_FEW, 0, 0, 0, 0, 0, 0, 0]
    assert out["S12"][0].tobytes() == np.array(Q.from_sim3(sim3[0])).tobytes()
    # one to nine pairs: round 1 still runs
    out = run_seqref(small(((1, 0),)), sim3)
    assert out["report"][0].tolist()[:4] == [Q.TOO_FEW, 1, 0, 0] and out["report"][0][4] > 0


def test_fixed_scale_keeps_the_bits_of_s():
    sc = small(((30, 3),), seed=72)
    sim3 = sim3_record(K.SIM3_A, 0.01, 0.02, 1.01)
    s_in = float(sim3[0][12])
    free = run_seqref(sc, sim3)
    fixed = run_seqref(sc, sim3, fix_scale=True)
    assert fixed["S12"][0][7] == s_in and fixed["report"][0][0] == Q.OK
    assert free["S12"][0][7] != s_in and abs(free["S12"][0][7] - 1.7) < abs(s_in - 1.7)
    # column 6 of every Jacobian is exactly zero, H[6][6] is lambda alone, x[6] is zero
    S = Q.from_sim3(sim3[0])
    E, Ei = Q.linearisation(S, True)
    assert E[12] == E[13] and Ei[12] == Ei[13]
    pairs = Q.build_pairs(sc["T"], sc["cur"], 2, sc["m_points"][0], S3.MATCH_POINTS, INV_SIGMA2)
    acc = [0.0] * Q.NSUM
    for p in pairs:
        Q.edge_terms(E, p.P2, p.o1, p.inv1, CAM, 3.0, 9.0, acc)
        Q.edge_terms(Ei, p.P1, p.o2, p.inv2, CAM, 3.0, 9.0, acc)
    H = Q.unpack_H(acc)
    assert all(H[a][6] == 0.0 for a in range(7)) and acc[34] == 0.0
    A = [row[:] for row in H]
    for a in range(7):
        A[a][a] = H[a][a] + 0.5
    ok, x = Q.ldlt_solve(A, acc[28:35])
    assert ok and x[6] == 0.0 and A[6][6] == 0.5


def test_round2_allowance():
    """nBad > 0 allows ten iterations in round 2, nBad == 0 five: optimize() is handed 10 or 5, and candidate 0 of batch B
    (nBad = 15) uses a sixth iteration."""
    seen = []
    real = Q.optimize

    def spy(S, pairs, out, est, cam, delta, dsqr, fix_scale, team, max_it, rnd):
        seen.append((rnd, max_it, sum(out)))
        return real(S, pairs, out, est, cam, delta, dsqr, fix_scale, team, max_it, rnd)
    Q.optimize = spy
    try:
        run_seqref(small(((20, 0),)), sim3_record(K.SIM3_A, 0.002, 0.0, 1.0))
        run_seqref(small(((20, 3),), seed=73), sim3_record(K.SIM3_A, 0.002, 0.0, 1.0))
    finally:
        Q.optimize = real
    assert seen == [(0, 5, 0), (1, 5, 0), (0, 5, 0), (1, 10, 3)]
    # round 1 does run into its cap of five when it starts far away
    far = run_seqref(small(((30, 0),), seed=74), sim3_record(K.SIM3_A, 0.05, 0.1, 1.1))
    assert far["report"][0][4] == 5
    rep = reference("B")["report"][0]
    assert rep[2] > 0 and rep[5] == 6


def test_lm_state_restarts_and_the_estimate_does_not():
    infos = []
    sc = small(((30, 3),), seed=72)
    run_seqref(sc, sim3_record(K.SIM3_A, 0.01, 0.02, 1.01), infos=infos)
    tr = infos[0]["trace"]
    assert [t[1] for t in tr if t[0] == 1][0] == 0                              # iteration numbers restart
    one = {}
    m = sc["m_points"][0].copy()
    Q.optimize_sim3(sc["T"], sc["cur"], 2, CAM, m, S3.MATCH_POINTS, INV_SIGMA2, sim3_record(K.SIM3_A, 0.01, 0.02, 1.01)[0],
                    TH2, False, Q.TEAM, one)
    assert one["est"] != Q.from_sim3(sim3_record(K.SIM3_A, 0.01, 0.02, 1.01)[0])


# ---- rule 7: the check reads the tried estimate -------------------------------------------------------------------------
def _classify_state():
    """An estimate that keeps every pair and a tried estimate (turned by 0.01) that removes most."""
    sc = small(((20, 0),))
    pairs = Q.build_pairs(sc["T"], sc["cur"], 2, sc["m_points"][0], S3.MATCH_POINTS, INV_SIGMA2)
    est = Q.from_sim3(sim3_record(K.SIM3_A)[0])
    tried = Q.from_sim3(sim3_record(K.SIM3_A, 0.01)[0])
    return sc, pairs, est, tried


def test_classify_reads_the_tried_estimate():
    sc, pairs, est, tried = _classify_state()
    th2 = float(f32(TH2))
    at_est = Q.classify(pairs, [False] * 20, est, CAM, th2)
    at_tried = Q.classify(pairs, [False] * 20, tried, CAM, th2)
    assert at_est == [] and len(at_tried) >= 5
    out = [False] * 20
    out[at_tried[0]] = True                          # a pair already removed is not looked at again
    assert Q.classify(pairs, out, tried, CAM, th2) == at_tried[1:]
    # optimize_sim3 hands classify() the tried estimate of optimize()
    seen = []
    real_o, real_c = Q.optimize, Q.classify
    marker = [0.1, 0.2, 0.3, 0.9, 1.0, 2.0, 3.0, 1.5]

    def fake_o(S, pairs, out, est, *a):
        return est, marker, 1

    def spy_c(pairs, out, tried, cam, th2):
        seen.append(tried)
        return []
    Q.optimize, Q.classify = fake_o, spy_c
    try:
        run_seqref(sc, sim3_record(K.SIM3_A))
    finally:
        Q.optimize, Q.classify = real_o, real_c
    assert seen == [marker, marker]


# ---- the scene cases --------------------------------------------------------------------------------------------------
def test_batches_cover_the_boundaries():
    a, b = reference("A"), reference("B")
    assert a["report"][:, 1].tolist() == [0, 9, 12] and b["report"][:, 1].tolist() == [64, 65, 257]
    assert a["report"][:, 0].tolist() == [Q.TOO_FEW, Q.TOO_FEW, Q.OK]
    assert b["report"][:, 0].tolist() == [Q.OK, Q.OK, Q.OK]
    assert a["report"][2].tolist()[1:4] == [12, 1, 11]
    # round 1 ends on an estimate the random partners still pull at, so it may take a pair of the model with them
    assert all(b["report"][c][2] >= BATCH_B[c][1] for c in range(3)) and b["report"][1][2] == 0
    for out, counts in ((a, BATCH_A), (b, BATCH_B)):
        for c in range(3):
            g, rep = counts[c][0], out["report"][c]
            if rep[0] != Q.OK:
                continue
            assert (out["matched12"][c][g:] == -1).all() and (out["matched12"][c][:g] >= 0).sum() == rep[3] >= g - 2
            s, R, t = K.SIM3_A
            assert abs(out["S12"][c][7] - s) < 2e-3 and np.abs(out["S12"][c][4:7] - t).max() < 5e-3


def test_batch_row_equals_candidate_alone():
    alone, batch = reference("A_alone"), reference("A")
    for k in ("matched12", "S12", "Scw", "report"):
        assert alone[k][0].tobytes() == batch[k][2].tobytes(), k


def test_both_match_forms_and_select():
    sc, sim3 = case("A")
    pts, slots = reference("A"), reference("A", S3.MATCH_SLOTS)
    for k in ("S12", "Scw", "report"):
        assert pts[k].tobytes() == slots[k].tobytes(), k
    assert ((pts["matched12"] == -1) == (slots["matched12"] == -1)).all()
    keep = slots["matched12"] >= 0
    assert (slots["matched12"][keep] == sc["m_slots"][keep]).all()
    sel = reference("A", S3.MATCH_POINTS, False, (1, 0, 1))
    assert sel["report"][1][0] == Q.SKIPPED and (sel["report"][1][1:].view(u8) == SENTINEL).all()
    assert sel["matched12"][1].tobytes() == sc["m_points"][1].tobytes() and (sel["S12"][1].view(u8) == SENTINEL).all()
    assert sel["S12"][2].tobytes() == pts["S12"][2].tobytes()


def test_scw_is_the_product_with_the_candidate_pose():
    sc, _ = case("B")
    out = reference("B")
    Tkf = sc["T"]["Tcw"][int(sc["kf_index"][0])].astype(f64).reshape(3, 4)
    S = out["S12"][0]
    R = np.array(Q.to_R(list(S[0:4]))).reshape(3, 3)
    want = np.hstack([S[7] * R @ Tkf[:, :3], (S[7] * R @ Tkf[:, 3] + S[4:7])[:, None]])
    assert np.allclose(out["Scw"][0].reshape(3, 4), want, atol=2e-6)


def test_team_width_is_part_of_the_arithmetic():
    sc, sim3 = case("A_alone")
    a, b = run_seqref(sc, sim3, team=256), run_seqref(sc, sim3, team=64)
    assert a["report"].tobytes() == b["report"].tobytes()                         # 12 pairs: one wavefront either way
    sc, sim3 = case("B")
    one = dict(sc, C=1, kf_index=sc["kf_index"][1:2], m_points=sc["m_points"][1:2], m_slots=sc["m_slots"][1:2])
    a, b = run_seqref(one, sim3[1:2], team=256), run_seqref(one, sim3[1:2], team=64)
    assert a["report"][0][:4].tolist() == b["report"][0][:4].tolist()
    assert np.abs(a["S12"] - b["S12"]).max() < 1e-6


# ---- the independent restatement ----------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _exp_sim3(u):
    """exp of the Sim3 generator, through the 4x4 matrix exponential (scipy-free: scaling and squaring by hand)."""
    G = np.zeros((4, 4))
    G[:3, :3] = _skew(u[0:3]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    k = 8
    G = G / 2 ** k
    M, term = np.eye(4), np.eye(4)
    for i in range(1, 14):
        term = term @ G / i
        M = M + term
    for _ in range(k):
        M = M @ M
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    return M[:3, :3] / s, M[:3, 3], s


def textbook(sc, c, sim3, fix_scale):
    """The same function with textbook tools: rotation matrices, analytic Jacobians of the left perturbation, libm exp,
    numpy.linalg.solve, sequential numpy sums.  The control flow (rounds, Huber, LM, the check at the tried estimate) is
    g2o's.  Returns (inlier slots, nIn, R, t, s) or None on the early return."""
    fx, fy, cx, cy = [float(f32(v)) for v in CAM]
    m = sc["m_points"][c].copy()
    pairs = Q.build_pairs(sc["T"], sc["cur"], int(sc["kf_index"][c]), m, S3.MATCH_POINTS, INV_SIGMA2)
    if not pairs:
        return None
    P1, P2 = np.array([p.P1 for p in pairs]), np.array([p.P2 for p in pairs])
    o1, o2 = np.array([p.o1 for p in pairs]), np.array([p.o2 for p in pairs])
    w1, w2 = np.array([p.inv1 for p in pairs]), np.array([p.inv2 for p in pairs])
    rec = sim3.astype(f64)
    R, t, s = rec[:9].reshape(3, 3), rec[9:12], rec[12]
    delta = float(np.sqrt(f32(TH2)))
    th2 = float(f32(TH2))
    active = np.ones(len(pairs), bool)

    def proj(Y):
        return np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1)

    def dproj(Y):
        J = np.zeros((len(Y), 2, 3))
        J[:, 0, 0], J[:, 0, 2] = fx / Y[:, 2], -fx * Y[:, 0] / Y[:, 2] ** 2
        J[:, 1, 1], J[:, 1, 2] = fy / Y[:, 2], -fy * Y[:, 1] / Y[:, 2] ** 2
        return J

    def errors(R, t, s):
        Y1 = s * P2 @ R.T + t
        Y2 = (P1 - t) @ R / s
        return o1 - proj(Y1), o2 - proj(Y2), Y1, Y2

    def robust(e, w):
        chi = w * (e ** 2).sum(1)
        big = chi > delta * delta
        rho0 = np.where(big, 2 * np.sqrt(chi) * delta - delta * delta, chi)
        rho1 = np.where(big, delta / np.sqrt(np.where(big, chi, 1.0)), 1.0)
        return chi, rho0, rho1

    def cost(R, t, s):
        e12, e21, _, _ = errors(R, t, s)
        return robust(e12, w1)[1][active].sum() + robust(e21, w2)[1][active].sum()

    def system(R, t, s):
        e12, e21, Y1, Y2 = errors(R, t, s)
        H, b = np.zeros((7, 7)), np.zeros(7)
        # left perturbation exp(u) S: d(map X2) = [-[Y1]x | I | Y1] u;  d(inverse map X1) = (R^T / s) [[X1]x | -I | -X1] u
        for e, Y, X, w, inverse in ((e12, Y1, P2, w1, False), (e21, Y2, P1, w2, True)):
            _, _, rho1 = robust(e, w)
            dp = dproj(Y)
            for j in np.nonzero(active)[0]:
                if inverse:
                    D = (R.T / s) @ np.hstack([_skew(X[j]), -np.eye(3), -X[j][:, None]])
                else:
                    D = np.hstack([-_skew(Y[j]), np.eye(3), Y[j][:, None]])
                J = -dp[j] @ D
                if fix_scale:
                    J[:, 6] = 0.0
                H += rho1[j] * w[j] * J.T @ J
                b += -rho1[j] * w[j] * J.T @ e[j]
        return H, b

    def optimize(R, t, s, max_it):
        tried = (R, t, s)
        lam = ni = 0.0
        n_bad = 0
        for it in range(max_it):
            its.append(0)
            H, b = system(R, t, s)
            current = ini = cost(R, t, s)
            if it == 0:
                lam, ni, n_bad = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
            qmax, rho = 0, 0.0
            while True:
                x = np.linalg.solve(H + lam * np.eye(7), b)
                if fix_scale:
                    x[6] = 0.0
                its[-1] += 1
                dR, dt, ds = _exp_sim3(x)
                tried = (dR @ R, ds * dR @ t + dt, ds * s)
                temp = cost(*tried)
                rho = (current - temp) / (x @ (lam * x + b) + 1e-3)
                if rho > 0 and math.isfinite(temp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam, ni, current = lam * max(1.0 / 3.0, alpha), 2.0, temp
                    R, t, s = tried
                else:
                    lam, ni = lam * ni, ni * 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                break
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                break
        return (R, t, s), tried

    def check(tried):
        e12, e21, _, _ = errors(*tried)
        return active & ((robust(e12, w1)[0] > th2) | (robust(e21, w2)[0] > th2))

    its = []                                         # trials per iteration, both rounds
    (R, t, s), tried = optimize(R, t, s, 5)
    bad = check(tried)
    n_bad = int(bad.sum())
    active &= ~bad
    if len(pairs) - n_bad < 10:
        return None
    (R, t, s), tried = optimize(R, t, s, 10 if n_bad > 0 else 5)
    active &= ~check(tried)
    return [p.slot for j, p in enumerate(pairs) if active[j]], int(active.sum()), R, t, s, its


def test_textbook_distance():
    worst = dict(R=0.0, t=0.0, s=0.0)
    for name in ("A", "B"):
        sc, sim3 = case(name)
        for fix in (False, True):
            ref = reference(name, S3.MATCH_POINTS, fix)
            for c in range(sc["C"]):
                tb = textbook(sc, c, sim3[c], fix)
                if ref["report"][c][0] != Q.OK:
                    assert tb is None, (name, fix, c)
                    continue
                slots, n_in, R, t, s, its = tb
                assert n_in == ref["report"][c][3], (name, fix, c)
                assert slots == np.nonzero(ref["matched12"][c] >= 0)[0].tolist(), (name, fix, c)
                S = ref["S12"][c]
                Rq = np.array(Q.to_R(list(S[0:4]))).reshape(3, 3) / (S[0:4] @ S[0:4])
                d = dict(R=np.abs(Rq - R).max(), t=np.abs(S[4:7] - t).max(), s=abs(S[7] - s))
                print("textbook", name, fix, c, {k: "%.3g" % v for k, v in d.items()}, "trials", its, "seqref iterations",
                      ref["report"][c][4:6].tolist())
                for k in worst:
                    worst[k] = max(worst[k], d[k])
    print("textbook worst", {k: "%.3g" % v for k, v in worst.items()})
    for k in worst:
        assert worst[k] <= TOL[k], (k, worst[k])


# ---- det_exp64 --------------------------------------------------------------------------------------------------------
def _grid():
    rng = np.random.default_rng(9)
    return np.concatenate([np.linspace(-1.0, 1.0, 20001), rng.uniform(-1, 1, 20000), rng.uniform(-1e-6, 1e-6, 2000),
                           [0.0, -0.0, 1e-9, -1e-9, 2.0 ** -28, -2.0 ** -28, 0.34657359027997264, 0.3465735902799727, 1.0397207708399179,
                            1.039720770839918, -1.0397207708399179, 5.5, -5.5, 20.0, -20.0, 700.0, -700.0, 709.7, -745.0]])


def test_det_exp64_against_libm():
    """Within 1 ulp of libm's exp over [-1, 1] (fdlibm states < 1 ulp for its own); the largest distance is printed."""
    worst = 0.0
    for x in _grid():
        x = float(x)
        got, want = Q.det_exp64(x), math.exp(x)
        ulp = math.ulp(want)
        worst = max(worst, abs(got - want) / ulp)
    print("det_exp64: max distance from libm %.3g ulp" % worst)
    assert worst <= 1.0
    assert Q.det_exp64(0.0) == 1.0 and Q.det_exp64(-0.0) == 1.0 and Q.det_exp64(1e-9) == 1.0 + 1e-9
    assert Q.det_exp64(710.0) == math.inf and Q.det_exp64(-746.0) == 0.0 and math.isnan(Q.det_exp64(math.nan))


# ---- the host build of orbhip_sim3opt_core.h ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program():
    import tempfile
    d = tempfile.mkdtemp(prefix="sim3opt_host_")
    exe = os.path.join(d, "sim3opt_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sim3opt_host.cpp"),
                    "-o", exe], check=True)
    return exe


def pack(sc, sim3, form, fix_scale, select, o):
    T = sc["T"]
    head = [sc["C"], sc["cur"], sc["rows"], sc["cap"], sc["np"], sc["pcap"], form, len(INV_SIGMA2), int(fix_scale),
            int(select is not None), 1, len(T["obs_kf"])]
    parts = [np.array(head, i32), np.array(CAM, f32), np.array([TH2], f32), INV_SIGMA2, T["slot_point"], T["n"], T["obs_start"],
             T["obs_kf"], T["obs_idx"], T["flags"], T["world"], T["Tcw"], T["kps"], sc["kf_index"]]
    parts += [np.array(select, u8)] if select is not None else []
    parts += [o["matched12"], sim3, o["S12"], o["Scw"], o["report"]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def prefilled(sc, form):
    Cn = sc["C"]
    return dict(matched12=(sc["m_points"] if form == S3.MATCH_POINTS else sc["m_slots"]).copy(),
                S12=np.full(Cn * 64, SENTINEL, u8).view(f64).reshape(Cn, 8).copy(),
                Scw=np.full(Cn * 48, SENTINEL, u8).view(f32).reshape(Cn, 12).copy(),
                report=np.full(Cn * 32, SENTINEL, u8).view(i32).reshape(Cn, 8).copy())


def run_host(sc, sim3, form, fix_scale, select, tmp_path, tag, fill=0):
    o = prefilled(sc, form)
    fin, fout = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    fin.write_bytes(pack(sc, sim3, form, fix_scale, select, o))
    subprocess.run([host_program(), "run", str(fin), str(fout), str(fill)], check=True)
    raw = fout.read_bytes()
    off = 0
    for k in ("matched12", "S12", "Scw", "report"):
        cnt = o[k].nbytes
        o[k] = np.frombuffer(raw[off:off + cnt], o[k].dtype).reshape(o[k].shape)
        off += cnt
    o["last64"] = np.frombuffer(raw[off:], f64)
    assert o["last64"].size == 16
    return o


HOST_CASES = [("A", S3.MATCH_POINTS, False, None), ("A", S3.MATCH_SLOTS, True, None), ("A", S3.MATCH_POINTS, False, (1, 0, 1)),
              ("B", S3.MATCH_POINTS, False, None), ("B", S3.MATCH_POINTS, True, None), ("A_alone", S3.MATCH_POINTS, False, None),
              ("nan_pair", S3.MATCH_POINTS, False, None)]


@pytest.mark.parametrize("k,fill", with_fills(range(len(HOST_CASES))))
def test_host_build_matches_seqref(k, fill, tmp_path):
    """`fill`: the byte the team's record and the compacted lists hold before the run (on the device they are LDS and registers)."""
    name, form, fix, select = HOST_CASES[k]
    sc, sim3 = case(name)
    assert_same(run_host(sc, sim3, form, fix, select, tmp_path, "c%d" % k, fill), reference(name, form, fix, select), HOST_CASES[k])


def test_host_build_on_the_hand_cases(tmp_path):
    """The hand-worked scenes once more through the host program, with the estimate and the tried estimate it leaves."""
    todo = []
    sc = small()
    sc["T"]["world"][int(sc["m_points"][0][3])] = np.nan
    todo.append((sc, sim3_record(K.SIM3_A), False))
    todo.append((small(((9, 2),), seed=71), sim3_record(K.SIM3_A, 0.005, 0.01, 1.005), False))
    todo.append((small(((10, 2),), seed=71), sim3_record(K.SIM3_A, 0.005, 0.01, 1.005), False))
    todo.append((small(((30, 3),), seed=72), sim3_record(K.SIM3_A, 0.01, 0.02, 1.01), True))
    todo.append((small(((0, 0),)), sim3_record(K.SIM3_A), False))
    todo.append((small(((30, 0),), seed=74), sim3_record(K.SIM3_A, 0.05, 0.1, 1.1), False))
    for k, (sc, sim3, fix) in enumerate(todo):
        infos = []
        want = run_seqref(sc, sim3, fix_scale=fix, infos=infos)
        got = run_host(sc, sim3, S3.MATCH_POINTS, fix, None, tmp_path, "h%d" % k)
        assert_same(got, want, k)
        if want["report"][0][1] > 0:
            assert got["last64"].tobytes() == np.array(infos[0]["est"] + infos[0]["tried"], f64).tobytes(), k


def test_host_classification_reads_the_tried_estimate(tmp_path):
    sc, pairs, est, tried = _classify_state()
    th2 = float(f32(TH2))
    want = Q.classify(pairs, [False] * 20, tried, CAM, th2)
    o = prefilled(sc, S3.MATCH_POINTS)
    flags = np.zeros(sc["cap"], u8)
    flags[want[0]] = 1                               # already removed: stays, is not counted again
    fin, fout = tmp_path / "cl.in", tmp_path / "cl.out"
    fin.write_bytes(pack(sc, sim3_record(K.SIM3_A), S3.MATCH_POINTS, False, None, o) + np.array(tried, f64).tobytes() + flags.tobytes())
    subprocess.run([host_program(), "classify", str(fin), str(fout)], check=True)
    raw = fout.read_bytes()
    cap = sc["cap"]
    e_out = np.frombuffer(raw[:cap], u8)
    matched = np.frombuffer(raw[cap:cap + 4 * cap], i32)
    removed, ne = np.frombuffer(raw[cap + 4 * cap:], i32).tolist()
    assert ne == 20 and removed == len(want) - 1 and np.nonzero(e_out[:20])[0].tolist() == want
    slots = [pairs[j].slot for j in want[1:]]
    assert np.nonzero(matched[:40] == -1)[0].tolist() == sorted(slots + np.nonzero(sc["m_points"][0][:40] == -1)[0].tolist())
    assert matched[pairs[want[0]].slot] == sc["m_points"][0][pairs[want[0]].slot]


def test_host_exp_matches_seqref(tmp_path):
    x = _grid().astype(f64)
    fin, fout = tmp_path / "x.in", tmp_path / "x.out"
    fin.write_bytes(x.tobytes())
    subprocess.run([host_program(), "exp", str(fin), str(fout)], check=True)
    got = np.frombuffer(fout.read_bytes(), f64)
    want = np.array([Q.det_exp64(float(v)) for v in x], f64)
    assert got.tobytes() == want.tobytes()


def test_python_mirror_declares_the_constants():
    assert (capi.SIM3OPT_OK, capi.SIM3OPT_TOO_FEW, capi.SIM3OPT_SKIPPED) == (Q.OK, Q.TOO_FEW, Q.SKIPPED)
    assert len(capi.SIM3OPT_REPORT) == 8
    names = [n for n, _, _ in capi.SYMBOLS]
    assert "orbhip_optimize_sim3_device" in names and "orbhip_optimize_sim3" in names
