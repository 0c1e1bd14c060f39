"""The sequential reference of PnPsolver (tests/seqref/pnp.py) on its own: hand-worked cases for every rule of the state
machine and of the EPnP core that is easy to get wrong, the Jacobi routines against LAPACK, and the scenes the GPU tests
replay (test_pnp_gpu.py imports them from here; the reference answers are computed once per process).

Measured on the CPU (the asserted tolerances are four times these, the margin is for LAPACK builds that differ):
  eigenvalues of MtM against numpy.linalg.eigh, relative to the largest          1.3e-15
  residual ||A v - lambda v|| relative to the largest eigenvalue                   9.6e-16
  projector onto the four smallest eigenvectors of a four-point MtM (max entry)    3.7e-15
  refined pose against the LAPACK restatement: R (max entry), t (max entry, m)     3.3e-14, 1.8e-13
"""
import contextlib
import functools
import math

import numpy as np
import pytest

from seqref import pnp as P

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)                 # KITTI 00-02
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], f32)
PARAMS = dict(prob=0.99, min_inliers=10, max_its=65, min_set=4, epsilon=0.4, th2=5.991)
MEASURED = dict(eigenvalues=1.3e-15, residual=9.6e-16, projector=3.7e-15, R=3.3e-14, t=1.8e-13)
TOL = {k: 4 * v for k, v in MEASURED.items()}


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def _rot(a):
    a = np.asarray(a, float)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(seed, spec, cap, repeat=None, planar=()):
    """One frame of cap - 1 key-point slots against len(spec) candidates.  spec[c] = (N, outliers, pixel noise): N matched
    slots whose points are present, of which `outliers` carry the world position of an unrelated point.  Every candidate
    also gets one match to a point that is not present and (slot form) one match to a slot without a point, which the
    constructor must drop.  `repeat` = (c, c0): candidate c shares the bank row of c0 and keeps every second match of it.
    Candidates in `planar` get world points on one plane (and consistent projections): every sample is degenerate."""
    rng = np.random.default_rng(seed)
    C, n = len(spec), cap - 1
    R, t = _rot([0.1, -0.2, 0.05]), np.array([0.3, -0.1, 0.5])
    kps = np.zeros(n, KP_DTYPE)
    kps["octave"] = rng.integers(0, 8, n)
    world, flags = [], []
    m_points = np.full((C, cap), -1, i32)
    m_slots = np.full((C, cap), -1, i32)
    slot_point = np.full((C, cap), -1, i32)
    # the frame's key points are the projections of one set of camera points; candidates match subsets of the slots
    Xc = np.c_[rng.uniform(-5, 5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 25, n)]
    kps["x"] = CAM["fx"] * Xc[:, 0] / Xc[:, 2] + CAM["cx"]
    kps["y"] = CAM["fy"] * Xc[:, 1] / Xc[:, 2] + CAM["cy"]
    kf_index = np.arange(C, dtype=i32)
    for c, (N, n_out, noise) in enumerate(spec):
        if repeat and repeat[0] == c:
            continue
        assert N + 2 <= n
        chosen = rng.choice(n, N + 2, replace=False)
        slots, drop = np.sort(chosen[:N]), chosen[N:]
        out = set(rng.choice(N, n_out, replace=False).tolist()) if n_out else set()
        bank = rng.permutation(cap)
        for k, s in enumerate(slots):
            x = Xc[s] + (0 if not noise else np.r_[rng.normal(0, noise, 2) * Xc[s][2] / CAM["fx"], 0])
            w = np.array([Xc[s][0], Xc[s][1], 1.0]) if c in planar else (x - t) @ R
            if k in out:
                w = rng.uniform(-30, 30, 3)
            m_points[c, s] = len(world)
            m_slots[c, s] = bank[k]
            slot_point[c, bank[k]] = len(world)
            world.append(w)
            flags.append(P.POINT_PRESENT)
        for j, s in enumerate(drop):
            if j == 0:                                                           # a point that is bad
                m_points[c, s] = len(world)
                m_slots[c, s] = bank[N]
                slot_point[c, bank[N]] = len(world)
                world.append(rng.uniform(-1, 1, 3))
                flags.append(0)
            else:                                                                # a slot of the key frame without a point
                m_slots[c, s] = bank[N + 1]
    if repeat:
        c, c0 = repeat
        kf_index[c] = c0
        keep = np.flatnonzero(m_points[c0] >= 0)[::2]
        m_points[c, keep] = m_points[c0, keep]
        m_slots[c, keep] = m_slots[c0, keep]
    world.append([0, 0, 0])
    flags.append(0)
    return dict(C=C, n=n, cap=cap, kps=kps, m_points=m_points, m_slots=m_slots, kf_index=kf_index,
                map=dict(flags=np.array(flags, u8), world=np.array(world, f32), slot_point=slot_point), R=R, t=t)


# name -> (scene arguments, parameters, seed of the draws, calls of five after the first)
SCENES = {
    # N = 0, below the minimum, equal to it twice (limit 1: one BEST, one NO_MORE), and ordinary
    "edge": (dict(seed=11, spec=[(0, 0, 0), (7, 0, 0), (10, 0, 0), (10, 1, 0), (40, 12, 0.5)], cap=64), PARAMS, 2, 2),
    # ordinary candidates; candidate 3 repeats the row of candidate 1; limits 35 .. 65, teams cross wavefronts and blocks
    "plain": (dict(seed=8, spec=[(24, 6, 0.3), (40, 12, 0.5), (60, 18, 0.5), (0, 0, 0)], cap=64, repeat=(3, 1)), PARAMS, 3, 3),
    # exact refinement sets of 15, 16, 17, 63, 64 and 65 correspondences: no noise, gross outliers
    "sizes": (dict(seed=8, spec=[(k + 8, 8, 0) for k in (15, 16, 17, 63, 64, 65)], cap=80), PARAMS, 2, 1),
    # a refinement set of 300: crosses the stride of the refinement workgroup
    "large": (dict(seed=9, spec=[(380, 80, 0)], cap=512), dict(PARAMS, max_its=20), 5, 0),
    # every sample is coplanar
    "planar": (dict(seed=13, spec=[(20, 0, 0), (24, 6, 0.3)], cap=64, planar=(0,)), dict(PARAMS, max_its=12), 6, 1),
}
EXTRA_ROWS = 20                                                                  # draws behind max_its for the resumed calls


@functools.lru_cache(maxsize=None)
def case(name):
    args, prm, seed, more = SCENES[name]
    sc = make_scene(**args)
    solvers = setups(name)
    rng = np.random.default_rng(seed)
    rows = prm["max_its"] + EXTRA_ROWS
    draws = np.zeros((sc["C"], rows, 4), i32)
    for c, S in enumerate(solvers):
        if S["n_corr"] >= 4:
            for k in range(4):
                draws[c, :, k] = rng.integers(0, S["n_corr"] - k, rows)
    return sc, draws, prm, more


@functools.lru_cache(maxsize=None)
def setups(name):
    args, prm, _, _ = SCENES[name]
    sc = make_scene(**args)
    return [P.setup(sc["kps"], sc["m_points"][c], P.MATCH_POINTS, None, sc["map"]["flags"], sc["map"]["world"], SIGMA2, **prm)
            for c in range(sc["C"])]


def snapshot(S):
    bi = None if S["best_inliers"] is None else np.array(S["best_inliers"], u8)
    bt = None if S["best_Tcw"] is None else np.array(S["best_Tcw"], f32)
    return dict(state=list(S["state"]), best_inliers=bi, best_Tcw=bt)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The calls the GPU tests replay: iterate(5) on fresh solvers (runs to the limit unless it returns), then `more` calls of
    five.  Returns [call][candidate] = (report, Tcw or None, inliers or None, snapshot of the solver after the call)."""
    sc, draws, prm, more = case(name)
    cam = P.make_cam(**CAM)
    out = []
    solvers = [dict(S, state=[0, 0]) for S in setups(name)]
    caches = [{} for _ in solvers]
    for _ in range(1 + more):
        call = []
        for c, S in enumerate(solvers):
            rep, tcw, inl = P.iterate(S, draws[c], 5, cam, cache=caches[c])
            call.append((rep, tcw, inl, snapshot(S)))
        out.append(call)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked rule cases
def test_parameter_table_by_hand():
    # N = 24: (int)(24 * 0.5f) = 12; epsilon stays 0.5; ceil(log(0.01) / log(1 - 0.5^3)) = ceil(34.49) = 35.  With the sample
    # size 4 as the exponent it would be ceil(71.4) = 72.
    assert P.ransac_parameters(24) == (12, 35)
    assert math.ceil(math.log(0.01) / math.log(1 - 0.5 ** 4)) == 72
    assert P.ransac_parameters(100) == (50, 35)
    # N = 15: 7 is raised to 10; epsilon = 10/15; ceil(log(0.01) / log(1 - 0.2963)) = ceil(13.1) = 14
    assert P.ransac_parameters(15) == (10, 14)
    assert P.ransac_parameters(10) == (10, 1)                                   # N == minInliers -> 1
    assert P.ransac_parameters(9) == (10, 0)                                    # iterate never runs
    assert P.ransac_parameters(0) == (10, 0)
    assert P.ransac_parameters(6, min_inliers=2) == (4, 14)                     # 3 is raised to minSet; eps = 4/6 as for N = 15
    assert P.ransac_parameters(24, max_its=20) == (12, 20)                      # clamped
    # epsilon 0.99 -> (int)23.76 = 23, epsilon stays 0.99 (> 23/24): ceil(log(0.01) / log(1 - 0.970299)) = ceil(1.31) = 2
    assert P.ransac_parameters(24, epsilon=0.99) == (23, 2)


def _solver(N, n_min, limit, n=None):
    return dict(n_corr=N, n=n or N, min_inliers=n_min, limit=limit, state=[0, 0], best_inliers=None, best_Tcw=None,
                kp_index=np.arange(N, dtype=i32))


def _mask(N, *idx):
    m = np.zeros(N, u8)
    m[list(idx)] = 1
    return m


def _machine(S, seq, refined, n_iterations):
    """iterate over scripted hypotheses: seq[it] = mask, refined = {mask bytes: refined count}; counts the Refine() calls."""
    calls = []

    def hyp(it):
        return seq[it], np.full(12, it, f32)

    def ref(best):
        calls.append(best.tobytes())
        cnt = refined[best.tobytes()]
        return cnt > S["min_inliers"], _mask(len(best), *range(cnt)), cnt, np.full(12, 100 + cnt, f32)
    rep, tcw, inl = P.iterate(S, None, n_iterations, None, hypothesis=hyp, refine_fn=ref)
    return rep, tcw, inl, calls


def test_loop_condition_is_an_or():
    N = 12
    none = [_mask(N)] * 40
    S = _solver(N, 6, 8)
    rep, _, _, _ = _machine(S, none, {}, 5)                                      # limit 8 > 5: runs to the limit
    assert rep.tolist() == [P.NO_MORE, N, 8, 8, 0, -1, 0, 6]
    rep, _, _, _ = _machine(S, none, {}, 5)                                      # at the limit: five more
    assert rep[3] == 13 and rep[0] == P.NO_MORE
    S = _solver(N, 6, 3)
    rep, _, _, _ = _machine(S, none, {}, 5)                                      # limit 3 < 5: five
    assert rep[3] == 5


def test_gates():
    N = 12
    six, six_b, five, seven = _mask(N, 0, 1, 2, 3, 4, 5), _mask(N, 6, 7, 8, 9, 10, 11), _mask(N, 0, 1, 2, 3, 4), _mask(N, *range(7))
    # 5 < 6: the gate never opens, Refine() is never called
    S = _solver(N, 6, 2)
    rep, tcw, _, calls = _machine(S, [five, five], {}, 1)
    assert rep[0] == P.NO_MORE and calls == [] and S["state"] == [2, 0] and tcw is None
    # 6 >= 6 opens the gate and 6 > 0 sets the best; a refinement of 6 inliers is not > 6.  The second 6 does not replace the
    # best (not >), yet Refine() runs again on the same set.  At the limit the unrefined best returns.
    S = _solver(N, 6, 2)
    rep, tcw, inl, calls = _machine(S, [six, six_b], {six.tobytes(): 6}, 1)
    assert calls == [six.tobytes()] * 2
    assert rep.tolist() == [P.BEST, N, 2, 2, 6, -1, 6, 6] and tcw.tolist() == [0] * 12 and inl.tolist() == six.tolist()
    # a refinement of 7 inliers succeeds
    S = _solver(N, 6, 2)
    rep, tcw, inl, calls = _machine(S, [six, six_b], {six.tobytes(): 7}, 1)
    assert rep.tolist() == [P.REFINED, N, 2, 1, 6, 0, 7, 6] and tcw[0] == 107 and inl.tolist() == seven.tolist()


def test_failed_record_then_non_improving_then_higher_record():
    N = 12
    a, b, c = _mask(N, *range(7)), _mask(N, *range(5, 12)), _mask(N, *range(9))
    S = _solver(N, 6, 5)
    rep, tcw, inl, calls = _machine(S, [a, b, c, a, a], {a.tobytes(): 6, c.tobytes(): 8}, 5)
    assert calls == [a.tobytes(), a.tobytes(), c.tobytes()]                      # b never reaches Refine()
    assert rep.tolist() == [P.REFINED, N, 5, 3, 9, 2, 8, 6] and tcw[0] == 108
    assert S["best_inliers"].tolist() == c.tolist() and S["best_Tcw"][0] == 2
    # the solver goes on: the next iteration that passes the gate refines the same best set again and returns at once
    rep, _, _, calls = _machine(S, [a, b, c, a, a], {c.tobytes(): 8}, 1)
    assert rep.tolist() == [P.REFINED, N, 5, 4, 9, 3, 8, 6] and calls == [c.tobytes()]


def test_best_from_an_earlier_call():
    N = 12
    a, none = _mask(N, *range(7)), _mask(N)
    S = _solver(N, 6, 2, n=20)
    S["kp_index"] = np.arange(N, dtype=i32) + 3
    rep, _, _, _ = _machine(S, [a, none], {a.tobytes(): 6}, 1)
    assert rep[0] == P.BEST
    rep, tcw, inl, calls = _machine(S, [a, none, none, none], {}, 2)             # two more, none passes the gate
    assert rep.tolist() == [P.BEST, N, 2, 4, 7, -1, 7, 6] and calls == []
    assert tcw.tolist() == [0] * 12 and np.flatnonzero(inl).tolist() == list(range(3, 10)) and len(inl) == 20
    S = _solver(5, 6, 0)
    assert P.iterate(S, None, 5, None)[0].tolist() == [P.TOO_FEW, 5, 0, 0, 0, -1, 0, 6]


def test_qr_solve_pivot_scan_and_zero_pivot():
    # Column 0 holds its only entry in the last row.  The scan of :881-885 reads rows 0 .. 4, finds eta == 0 and returns
    # although the matrix has full rank: X keeps what it held.
    A = [f64(0)] * 24
    A[5 * 4 + 0] = f64(5)
    for r, c in ((0, 1), (1, 2), (2, 3)):
        A[r * 4 + c] = f64(1)
    X = [f64(v) for v in (1, 2, 3, 4)]
    assert P.qr_solve(list(A), [f64(1)] * 6, X, 6, 4) is False and X == [1, 2, 3, 4]
    # a dense matrix whose largest entry of column 0 sits in the last row: eta is 3, not 9, which only changes the
    # scaling; the solve goes through and x is the least-squares solution
    full = np.array([[1, 2, 0, 1], [0, 1, 3, 1], [2, 0, 1, 1], [1, 1, 1, 0], [3, 1, 0, 2], [9, 1, 2, 1]], f64)
    rhs = [3, 2, 4, 0, 1, 10]
    assert P.qr_solve([f64(v) for v in full.ravel()], [f64(v) for v in rhs], X, 6, 4) is True
    assert np.allclose(full.T @ full @ np.array(X), full.T @ np.array(rhs, f64), atol=1e-12)
    # gauss_newton on L = 0: every step returns early, X is zeros from the first step on, the betas stay
    be = P.gauss_newton([[f64(0)] * 10] * 6, [f64(1)] * 6, [f64(v) for v in (1, 2, 3, 4)])
    assert be == [1, 2, 3, 4]


def test_sign_choices_and_literals():
    L = [[f64(1 if i == j else 0) for j in range(10)] for i in range(6)]
    rho = [f64(v) for v in (-4, 2, 9, -6, 1, 1)]
    # approx_1 solves columns 0, 1, 3, 6 -> b = (-4, 2, -6, 0): b0 < 0 flips every sign
    assert P.find_betas_approx(1, L, rho) == [2, -1, 3, 0]
    # approx_2 solves columns 0, 1, 2 -> b = (-4, 2, 9): b0 < 0, b2 > 0 -> beta1 = 0; b1 >= 0 keeps the sign of beta0
    assert P.find_betas_approx(2, L, rho) == [2, 0, 0, 0]
    assert P.find_betas_approx(2, L, [f64(v) for v in (4, -2, 9, 0, 0, 0)]) == [-2, 3, 0, 0]
    # approx_3 solves columns 0 .. 4 -> b = (-4, 2, 9, -6, 1): beta2 = b3 / beta0
    assert P.find_betas_approx(3, L, rho) == [2, 0, -3, 0]
    v = [[f64(1 if k == 3 * i else 0) for k in range(12)] for i in range(4)]
    assert P.compute_L_6x10(v)[0][:3] == [1, -2, 1] and P.compute_L_6x10(v)[3][4] == -2   # 2.0f * dot
    # a reflection: det < 0 flips row 2 of R only
    R = P.svd_uvt3(np.diag([1.0, 1.0, -1.0]))
    assert np.array_equal(R, np.diag([1.0, 1.0, -1.0]))


def test_check_inliers_type_mix():
    cam = P.make_cam(**CAM)
    S = dict(n_corr=2, p3d=np.array([[0.1, 0.2, 4.0], [0.1, 0.2, 0.0]], f32), p2d=np.zeros((2, 2), f32), max_err=np.zeros(2, f32))
    R, t = np.eye(3), [f64(0)] * 3
    Xc, Yc, inv = f32(0.1), f32(0.2), f32(f64(1) / f64(f32(4.0)))
    ue = cam["uc"] + cam["fu"] * f64(Xc) * f64(inv)
    ve = cam["vc"] + cam["fv"] * f64(Yc) * f64(inv)
    S["p2d"][0] = (f32(ue) + f32(1), f32(ve))
    dx, dy = f32(f64(S["p2d"][0][0]) - ue), f32(f64(S["p2d"][0][1]) - ve)
    err = f32(f32(dx * dx) + f32(dy * dy))
    S["max_err"][:] = err                                                        # strict: equal is out
    assert P.check_inliers(S, R, t, cam).tolist() == [0, 0]
    S["max_err"][:] = np.nextafter(err, f32(2))
    assert P.check_inliers(S, R, t, cam).tolist() == [1, 0]                     # zero depth: inf, no inlier, no fault


def test_coplanar_sample_gives_no_inliers():
    ref = reference("planar")
    S = setups("planar")[0]
    cam = P.make_cam(**CAM)
    sc, draws, _, _ = case("planar")
    for it in range(3):
        R, t = P.pose_of(S, P.sample(S["n_corr"], draws[0][it]), cam)
        assert not np.isfinite(np.array(R)).any() and P.check_inliers(S, R, t, cam).sum() == 0
    assert ref[0][0][0][0] == P.NO_MORE and ref[0][0][0][4] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the scenes
def test_scenes_cover_every_status_and_shape():
    seen = set()
    for name in SCENES:
        for call in reference(name):
            seen |= {int(r[0][0]) for r in call}
    assert seen == {P.REFINED, P.BEST, P.NO_MORE, P.TOO_FEW}
    edge = reference("edge")[0]
    assert [int(r[0][0]) for r in edge[:4]] == [P.TOO_FEW, P.TOO_FEW, P.BEST, P.NO_MORE]
    assert [S["n_corr"] for S in setups("edge")] == [0, 7, 10, 10, 40] and [S["limit"] for S in setups("edge")] == [0, 0, 1, 1, 65]
    assert [(S["n_corr"], S["min_inliers"], S["limit"]) for S in setups("plain")] == [(24, 10, 62), (40, 16, 65), (60, 24, 65), (20, 10, 35)]
    # the refinement sets of the "sizes" and "large" scenes
    sizes = [int(r[3]["state"][1]) for r in reference("sizes")[0]]
    assert sizes == [15, 16, 17, 63, 64, 65] and all(int(r[0][0]) == P.REFINED for r in reference("sizes")[0])
    assert reference("large")[0][0][3]["state"][1] == 300 and reference("large")[0][0][0][0] == P.REFINED
    # a resumed solver returns again (the best set's refinement is repeated) and one reaches its limit with BEST / NO_MORE
    assert any(int(r[0][0]) == P.REFINED for r in reference("plain")[1])


def test_refined_poses_recover_the_truth():
    sc = case("plain")[0]
    for r in reference("plain")[0][:3]:
        assert r[0][0] == P.REFINED
        T = r[1].reshape(3, 4)
        assert np.abs(T[:, :3] - sc["R"]).max() < 5e-3 and np.abs(T[:, 3] - sc["t"]).max() < 5e-2


# ---------------------------------------------------------------------------------------------------------------------
# against LAPACK
def _samples(name, count):
    sc, draws, _, _ = case(name)
    cam = P.make_cam(**CAM)
    for c, S in enumerate(setups(name)):
        if S["n_corr"] < 12:
            continue
        for it in range(count):
            idx = P.sample(S["n_corr"], draws[c][it])
            yield S, idx, cam


def _mtm(S, idx, cam):
    pws = [[f64(v) for v in S["p3d"][i]] for i in idx]
    us = [[f64(v) for v in S["p2d"][i]] for i in idx]
    with np.errstate(all="ignore"):
        return P.mtm_of(pws, us, cam)[2]


def test_eigen_solver_against_lapack():
    worst = dict(eigenvalues=0.0, residual=0.0, projector=0.0)
    cases = [(S, idx) + (cam,) for S, idx, cam in _samples("plain", 6)]
    S = setups("plain")[2]
    cases.append((S, list(range(S["n_corr"])), P.make_cam(**CAM)))              # an n-point MtM
    for S, idx, cam in cases:
        A = _mtm(S, idx, cam)
        w, ut = P.jacobi_eig(A)
        wl, vl = np.linalg.eigh(A)
        scale = abs(wl).max()
        worst["eigenvalues"] = max(worst["eigenvalues"], np.abs(w - wl[::-1]).max() / scale)
        worst["residual"] = max(worst["residual"], max(np.linalg.norm(A @ ut[k] - w[k] * ut[k]) for k in range(12)) / scale)
        if len(idx) == 4:
            worst["projector"] = max(worst["projector"], np.abs(ut[8:].T @ ut[8:] - vl[:, :4] @ vl[:, :4].T).max())
        assert np.abs(ut @ ut.T - np.eye(12)).max() < 1e-14
    print("measured", worst)
    for k, v in worst.items():
        assert v <= TOL[k], (k, v)


@contextlib.contextmanager
def lapack():
    """The seqref with numpy.linalg in place of the Jacobi routines."""
    saved = P.jacobi_eig, P.svd_solve, P.svd_pinv3, P.svd_uvt3

    def eig(A):
        w, v = np.linalg.eigh(np.array(A, f64))
        return w[::-1].copy(), v[:, ::-1].T.copy()

    def uvt(A):
        u, _, vt = np.linalg.svd(np.array(A, f64))
        return u @ vt
    P.jacobi_eig = eig
    P.svd_solve = lambda B, b: list(np.linalg.lstsq(np.array(B, f64), np.array(b, f64), rcond=float(P.SVD_CUT))[0])
    P.svd_pinv3 = lambda Cm: np.linalg.pinv(np.array(Cm, f64), rcond=float(P.SVD_CUT))
    P.svd_uvt3 = uvt
    try:
        yield
    finally:
        P.jacobi_eig, P.svd_solve, P.svd_pinv3, P.svd_uvt3 = saved


def test_refined_poses_against_lapack_restatement():
    worst = dict(R=0.0, t=0.0)
    cam = P.make_cam(**CAM)
    count = 0
    for name in ("plain", "sizes", "edge"):
        for call in reference(name):
            for c, r in enumerate(call):
                if r[0][0] != P.REFINED:
                    continue
                S = dict(setups(name)[c], best_inliers=r[3]["best_inliers"])
                ok, mask, cnt, tcw = P.refine(S, cam)
                assert ok and tcw.tobytes() == r[1].tobytes()
                idx = [i for i in range(S["n_corr"]) if S["best_inliers"][i]]
                R, t = P.pose_of(S, idx, cam)
                with lapack():
                    Rl, tl = P.pose_of(S, idx, cam)
                    mask_l = P.check_inliers(S, Rl, tl, cam)
                assert np.array_equal(mask, mask_l), (name, c)                  # a condition on the scenes, checked here
                worst["R"] = max(worst["R"], np.abs(np.array(R) - np.array(Rl)).max())
                worst["t"] = max(worst["t"], np.abs(np.array(t, f64) - np.array(tl, f64)).max())
                count += 1
    print("measured", worst, count)
    assert count >= 8
    for k, v in worst.items():
        assert v <= TOL[k], (k, v)
