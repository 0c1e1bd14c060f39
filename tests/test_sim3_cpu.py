"""Sim3Solver over tables: the sequential reference (tests/seqref/sim3.py) alone, no GPU.

The rules of src/Sim3Solver.cc are pinned by hand-worked cases: every skip reason of the constructor, the truncated
thresholds, the list handling of the sampler, the state machine of iterate (>= for the best, > for the return, "no more"
only after the loop), the iteration limit as a function of N.  A synthetic scene with a known Sim3 checks the whole, and
the fp32 Jacobi route is measured against an fp64 restatement over numpy.linalg.eigh.  The scenes built here are also the
inputs of test_sim3_gpu.py and test_cpp_sim3_gpu.py, with the reference answers computed once per process.
"""
import numpy as np

from orb_slam2_comment_amd import capi
from seqref import sim3 as S

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8
CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], f32)


def rot(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(axis, angle, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(axis, angle), t
    return T


SIM3_A = (1.7, rot([0.3, 1.0, 0.2], 0.4), np.array([0.5, -0.2, 0.3]))
SIM3_B = (0.8, rot([1.0, -0.2, 0.5], -0.3), np.array([-0.4, 0.3, 0.1]))


def inverse_sim3(sim3, X1):
    s, R, t = sim3
    return (R.T @ (np.asarray(X1, f64) - t)) / s


def build(cands, n1, cap, seed, no_point=(), p1_absent=(), p1_unobserved=(), p1_twice=()):
    """Tables for the current key frame (bank row 1) and len(cands) candidates (rows 2 ..; row 0 is a bystander).
    cands[c] = list of (i1, X2 or a Sim3 or None, marks): slot i1 of the current key frame is matched to a new point of the
    candidate whose camera coordinates are X2 (a Sim3: the exact partner of X1; None: a random point); marks is a set of
    'nomatch', 'absent', 'unobserved', 'empty_slot', 'l0' (octave 0 in the current key frame), 'l2' (octave 2 in the
    candidate).  Returns T (tables), cur, kf_index, matched12 in both forms, X1 [n1, 3]."""
    rng = np.random.default_rng(seed)
    C = len(cands)
    rows, cur = C + 2, 1
    Tcw = [pose(rng.uniform(-1, 1, 3), rng.uniform(0, 0.6), rng.uniform(-2, 2, 3)) for _ in range(rows)]
    z = rng.uniform(2.0, 8.0, n1)
    X1 = np.stack([rng.uniform(-0.5, 0.5, n1) * z, rng.uniform(-0.4, 0.4, n1) * z, z], 1)
    world, flags, obs = [], [], []
    slot_point = np.full((rows, cap), -1, i32)
    kps = np.zeros((rows, cap), capi.KP_DTYPE)
    kps["octave"] = rng.integers(0, 8, (rows, cap))
    inv_cur = np.linalg.inv(Tcw[cur])
    for i in range(n1):
        world.append(inv_cur[:3, :3] @ X1[i] + inv_cur[:3, 3])
        flags.append(0 if i in p1_absent else capi.POINT_PRESENT)
        lst = [(0, int(rng.integers(0, cap)))] if i % 3 == 0 else []          # seen by the bystander first
        if i in p1_twice:
            lst += [(cur, (i + 7) % n1), (cur, i)]                            # the first entry that names the row counts
        elif i not in p1_unobserved:
            lst.append((cur, i))
        obs.append(lst)
        if i not in no_point:
            slot_point[cur, i] = i
    m_points, m_slots = np.full((C, cap), -1, i32), np.full((C, cap), -1, i32)
    for c, corr in enumerate(cands):
        kf = c + 2
        inv_kf = np.linalg.inv(Tcw[kf])
        slots = rng.permutation(cap)[:len(corr)]
        for (i1, what, marks), j in zip(corr, slots):
            if what is None:
                zz = rng.uniform(2.0, 8.0)
                X2 = np.array([rng.uniform(-0.5, 0.5) * zz, rng.uniform(-0.4, 0.4) * zz, zz])
            elif isinstance(what, tuple):
                X2 = inverse_sim3(what, X1[i1])
            else:
                X2 = np.asarray(what, f64)
            p2 = len(world)
            world.append(inv_kf[:3, :3] @ X2 + inv_kf[:3, 3])
            flags.append(0 if "absent" in marks else capi.POINT_PRESENT)
            obs.append([(0, 3)] if "unobserved" in marks else [(kf, int(j))])
            if "l0" in marks:
                kps["octave"][cur, i1] = 0
            if "l2" in marks:
                kps["octave"][kf, j] = 2
            if "nomatch" in marks:
                slot_point[kf, j] = p2
            elif "empty_slot" in marks:
                m_slots[c, i1] = j                                            # a slot without a point: no match
            else:
                slot_point[kf, j] = p2
                m_points[c, i1], m_slots[c, i1] = p2, j
    n_pts = len(world)
    obs_start = np.zeros(n_pts + 1, i32)
    obs_start[1:] = np.cumsum([len(o) for o in obs])
    flat = [e for o in obs for e in o]
    n = np.full(rows, cap, i32)
    n[cur] = n1
    T = dict(slot_point=slot_point, n=n, obs_start=obs_start, obs_kf=np.array([e[0] for e in flat], i32),
             obs_idx=np.array([e[1] for e in flat], i32), flags=np.array(flags + [0] * 5, u8),
             world=np.array(world + [[0, 0, 0]] * 5, f64).astype(f32), Tcw=np.stack(Tcw)[:, :3, :].reshape(rows, 12).astype(f32),
             kps=kps)
    return dict(T=T, cur=cur, kf_index=np.arange(2, rows, dtype=i32), m_points=m_points, m_slots=m_slots, X1=X1, cap=cap,
                rows=rows, np=n_pts, pcap=n_pts + 5, C=C)


def cam_dict():
    return S.make_cam(**CAM)


def setups(scene, prob=0.99, min_inliers=20, max_its=300):
    return [S.setup(scene["T"], scene["cur"], int(kf), scene["m_points"][c], S.MATCH_POINTS, cam_dict(), SIGMA2, prob,
                    min_inliers, max_its) for c, kf in enumerate(scene["kf_index"])]


def run_calls(scene, draws, n_iterations, fix_scale, min_inliers=20, max_its=300):
    """The reference's calling pattern: iterate(n_iterations) on every candidate, again and again until every one of
    them has reported "no more" (or too few).  Returns the list of calls, each a list of (report, sim3, inliers, state)."""
    sol = setups(scene, 0.99, min_inliers, max_its)
    calls, done = [], [False] * len(sol)
    while not all(done):
        out = []
        for c, s in enumerate(sol):
            rep, sim3, inl = S.iterate(s, draws[c], n_iterations, min_inliers, fix_scale, cam_dict())
            out.append((rep, sim3, inl, list(s["state"])))
            done[c] = rep[0] in (S.NO_MORE, S.TOO_FEW)
        calls.append(out)
        assert len(calls) <= max_its + 2
    return calls


# ---- the inputs shared with the GPU tests ----------------------------------------------------------------------------
def _seq(first, count, what, marks=()):
    return [(first + k, what, set(marks)) for k in range(count)]


def hand_scene():
    """Candidate 0: every skip reason.  1: 20 exact partners + 5 random ones (exactly min_inliers).  2: 22 + 3 (N = 25,
    limit 7).  3: two models, 30 under A then 24 under B, then 6 random.  4 / 5 / 6: N = 19 / 20 / 21.  7: the truncated
    threshold, as in hand_threshold_scene."""
    skip = ([(0, SIM3_A, {"nomatch"}), (1, SIM3_A, set()), (2, SIM3_A, set()), (3, SIM3_A, set()), (4, SIM3_A, {"absent"}),
             (5, SIM3_A, {"unobserved"}), (6, SIM3_A, {"empty_slot"}), (7, SIM3_A, set())] + _seq(8, 24, SIM3_A))
    def make(thr):
        # slots 1 .. 3 of the current key frame are spoilt for every candidate: the others start at slot 8
        return build([skip, _seq(8, 20, SIM3_A) + _seq(28, 5, None), _seq(8, 22, SIM3_A) + _seq(30, 3, None),
                      _seq(8, 30, SIM3_A) + _seq(38, 24, SIM3_B) + _seq(62, 6, None), _seq(8, 19, SIM3_A), _seq(8, 20, SIM3_A),
                      _seq(8, 21, SIM3_A), thr], 70, 96, 11, no_point={1}, p1_absent={2}, p1_unobserved={3}, p1_twice={7})
    X1 = make(_seq(40, 26, SIM3_A))["X1"][65]          # the camera coordinates do not depend on the partners
    off = X1 + np.array([3.017 * X1[2] / CAM["fx"], 0.0, 0.0])
    return make(_seq(40, 25, SIM3_A) + [(65, inverse_sim3(SIM3_A, off), {"l0", "l2"})])


def hand_threshold_scene():
    """Correspondence 25 of the only candidate misses in image 1 by 3.017 px at octave 0 (threshold 9, not 9.21) and is at
    octave 2 in the candidate (threshold 19), so only the truncation rejects it."""
    probe = build([_seq(0, 26, SIM3_A)], 30, 64, 12)
    X1 = probe["X1"][25]
    off = X1 + np.array([3.017 * X1[2] / CAM["fx"], 0.0, 0.0])
    corr = _seq(0, 25, SIM3_A) + [(25, inverse_sim3(SIM3_A, off), {"l0", "l2"})]
    return build([corr], 30, 64, 12)


def hand_draws(scene, max_its=300):
    """Draws that name correspondences directly: three different positions below N - 2 are still where they started
    when they are drawn, so the replay returns the draws themselves."""
    C = scene["C"]
    d = np.zeros((C, max_its, 3), i32)
    d[:, :, 0], d[:, :, 1], d[:, :, 2] = 0, 1, 2
    rng = np.random.default_rng(3)
    for it in range(max_its):
        d[:, it] = np.sort(rng.choice(15, 3, replace=False))                  # triples inside the first model
    # candidate 2 (22 + 3): six iterations that take a random partner (22 .. 24) with the first draw, whose range is the
    # whole list, the seventh and last clean
    d[2, :6] = [[23, 0, 5], [22, 1, 6], [24, 2, 7], [22, 3, 8], [23, 4, 9], [24, 0, 9]]
    d[2, 6] = [3, 10, 17]
    # candidate 3 (30 A + 24 B + 6): A returns, then B (24 < 30: not returned), then A again; later rows stay inside A
    d[3, 0] = [2, 11, 25]
    d[3, 1] = [31, 40, 52]
    d[3, 2] = [5, 14, 28]
    return d


def scene64():
    """64 matches under a Sim3 with s = 1.7; 19 of them (30 %) have the partner displaced by 0.5 to 1 m at 2 to 8 m depth."""
    rng = np.random.default_rng(21)
    probe = build([_seq(0, 64, SIM3_A)], 64, 80, 20)
    bad = np.sort(rng.choice(64, 19, replace=False))
    corr = []
    for i in range(64):
        if i in bad:
            v = rng.normal(size=3)
            v *= rng.uniform(0.5, 1.0) / np.linalg.norm(v)
            corr.append((i, inverse_sim3(SIM3_A, probe["X1"][i]) + v, set()))
        else:
            corr.append((i, SIM3_A, set()))
    sc = build([corr], 64, 80, 20)
    sc["clean"] = np.array([i for i in range(64) if i not in bad])
    return sc


SIM3_U = (1.0, rot([0.2, -0.4, 1.0], 0.5), np.array([0.3, 0.1, -0.6]))


def unit_scene():
    """40 matches under a Sim3 of scale 1 and 10 random ones: the input on which mbFixScale returns something."""
    return build([_seq(0, 40, SIM3_U) + _seq(40, 10, None)], 50, 64, 41)


BATCH_N = (0, 3, 19, 65, 257)
BATCH_MIN, BATCH_ITS = 3, 70


def batch_scene():
    """Five candidates of N = 0, 3, 19, 65 and 257 correspondences, about 40 % of each under one model; min_inliers = 3."""
    cands = []
    for N in BATCH_N:
        good = (2 * N) // 5 if N > 3 else N
        cands.append(_seq(0, good, SIM3_B) + _seq(good, N - good, None))
    return build(cands, 300, 320, 31)


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def case(name):
    """(scene, draws, min_inliers, max_its) of 'hand', 'scene', 'unit' or 'batch', built once."""
    def make():
        if name == "hand":
            sc = hand_scene()
            return sc, hand_draws(sc), 20, 300
        if name == "scene":
            sc = scene64()
            from orb_slam2_comment_amd import sim3_draws
            return sc, sim3_draws(1, 300, [64], 5), 20, 300
        from orb_slam2_comment_amd import sim3_draws
        if name == "unit":
            return unit_scene(), sim3_draws(1, 300, [50], 7), 20, 300
        sc = batch_scene()
        return sc, sim3_draws(5, BATCH_ITS, BATCH_N, 6), BATCH_MIN, BATCH_ITS
    return cached(("case", name), make)


def reference(name, n_iterations, fix_scale):
    sc, draws, mn, mx = case(name)
    return cached(("ref", name, n_iterations, fix_scale), lambda: run_calls(sc, draws, n_iterations, fix_scale, mn, mx))


# ---- setup -----------------------------------------------------------------------------------------------------------
def test_every_skip_reason_and_the_compaction_order():
    sc = hand_scene()
    s = setups(sc)[0]
    # slots 0 .. 7: no match, no point in the slot, point 1 bad, point 1 unobserved, point 2 bad, point 2 unobserved,
    # (slots form only) a slot without a point, and slot 7 whose point names the row twice
    assert s["slot1"].tolist() == [7] + list(range(8, 32)) and s["n_corr"] == 25 and s["n1"] == 70
    # slots form: the same answer, through slot_point
    s2 = S.setup(sc["T"], sc["cur"], 2, sc["m_slots"][0], S.MATCH_SLOTS, cam_dict(), SIGMA2)
    for k in ("x1", "x2", "p1", "p2", "max_err1", "max_err2", "slot1"):
        assert np.array_equal(s[k], s2[k]), k
    assert sc["m_slots"][0][6] >= 0 and sc["m_points"][0][6] < 0
    # GetIndexInKeyFrame is the FIRST entry naming the row: slot 7's octave comes from key point (7 + 7) % 70
    oct7 = int(sc["T"]["kps"]["octave"][1, 14])
    assert s["max_err1"][0] == int(9.210 * float(SIGMA2[oct7]))


def test_thresholds_are_truncated_integers():
    assert [S.max_error(v) for v in SIGMA2[:4]] == [9, 13, 19, 27]
    assert 9.210 * float(SIGMA2[1]) > 13.2
    sc = hand_threshold_scene()
    s = setups(sc)[0]
    assert s["n_corr"] == 26 and s["max_err1"][25] == 9 and s["max_err2"][25] == 19
    H = S.compute_sim3([s["x1"][i] for i in (1, 8, 19)], [s["x2"][i] for i in (1, 8, 19)], False)
    errs = []
    inl = S.check_inliers(s, H, cam_dict(), errs)
    e1, e2 = errs[25]
    print("err1 %.4f err2 %.4f" % (e1, e2))
    assert 9.0 < e1 < 9.21 and e2 < 19.0
    assert inl == [True] * 25 + [False]                                       # 9.21 would have let it in


def test_camera_coordinates_and_projections_follow_the_conventions():
    sc = hand_scene()
    s = setups(sc)[1]
    T, cur = sc["T"], sc["cur"]
    for k in range(s["n_corr"]):
        W = T["world"][int(s["slot1"][k])].astype(f64)
        M = T["Tcw"][cur].reshape(3, 4).astype(f64)
        X = (M[:, :3] @ W + M[:, 3])
        assert np.abs(X - s["x1"][k]).max() < 1e-5
        assert abs(CAM["fx"] * X[0] / X[2] + CAM["cx"] - s["p1"][k][0]) < 1e-3


# ---- the sampler -----------------------------------------------------------------------------------------------------
def test_draw_replay_by_hand():
    assert S.sample(5, [1, 1, 1]) == [1, 4, 3]        # a repeated randi takes what was moved in
    assert S.sample(5, [4, 0, 0]) == [4, 0, 3]        # randi equal to the last position: nothing moves
    assert S.sample(5, [0, 3, 0]) == [0, 3, 4]        # the third draw lands on the position the first one refilled
    assert S.sample(3, [0, 0, 0]) == [0, 2, 1]
    for N in range(3, 8):                             # always three different correspondences
        for a in range(N):
            for b in range(N - 1):
                for c in range(N - 2):
                    assert len(set(S.sample(N, [a, b, c]))) == 3


# ---- the limit -------------------------------------------------------------------------------------------------------
def test_iteration_limit_table():
    got = [S.iteration_limit(N, 0.99, 20, 300) for N in (20, 21, 25, 30, 40, 60, 80, 81)]
    assert got == [1, 3, 7, 14, 35, 123, 293, 300]
    assert S.iteration_limit(19, 0.99, 20, 300) == 0 and S.iteration_limit(4096, 0.99, 20, 300) == 300
    assert S.iteration_limit(4096, 0.99, 3, 10 ** 9) == 10 ** 9        # clamped before the conversion to int
    assert S.iteration_limit(3, 0.99, 3, 70) == 1


def test_n_19_20_21():
    sc, draws, mn, mx = case("hand")
    first = reference("hand", 5, False)[0]
    assert first[4][0].tolist()[:4] == [S.TOO_FEW, 19, 0, 0] and not first[4][2].any()
    assert first[5][0].tolist()[:4] == [S.NO_MORE, 20, 1, 1] and first[5][0][4] == 20      # one iteration, 20 is not > 20
    assert first[6][0].tolist() == [S.RETURNED, 21, 3, 1, 21, 0, 21, 0]


# ---- the state machine -----------------------------------------------------------------------------------------------
def test_exactly_min_inliers_is_not_returned():
    calls = reference("hand", 5, False)
    reps = [c[1][0].tolist() for c in calls]
    assert reps[0] == [S.CONTINUE, 25, 7, 5, 20, -1, 0, 0]                   # best is 20, nothing returned
    assert reps[1] == [S.NO_MORE, 25, 7, 7, 20, -1, 0, 0]
    assert not calls[0][1][2].any() and calls[0][1][1] is None


def test_return_on_the_last_iteration_then_no_more():
    calls = reference("hand", 5, False)
    reps = [c[2][0].tolist() for c in calls]
    assert reps[0][0] == S.CONTINUE and reps[0][3] == 5 and reps[0][4] < 20
    assert reps[1] == [S.RETURNED, 25, 7, 7, 22, 6, 22, 0]                   # bNoMore stays false on this call
    assert reps[2] == [S.NO_MORE, 25, 7, 7, 22, -1, 0, 0]                    # and the next one runs nothing
    inl = calls[1][2][2]
    assert inl[8:30].all() and inl.sum() == 22


def test_resuming_after_a_return():
    calls = reference("hand", 5, False)
    reps = [c[3][0].tolist() for c in calls]
    assert reps[0] == [S.RETURNED, 60, reps[0][2], 1, 30, 0, 30, 0]
    # the second call passes the 24-inlier model (24 > 20 but < 30) and returns on the next 30
    assert reps[1] == [S.RETURNED, 60, reps[0][2], 3, 30, 2, 30, 0]
    assert calls[0][3][2][8:38].all() and calls[0][3][2].sum() == 30
    # the other order: B first returns 24, then A returns 30
    sc, draws, mn, mx = case("hand")
    s = setups(sc)[3]
    d = draws[3].copy()
    d[0], d[1] = draws[3][1], draws[3][0]
    r0, _, i0 = S.iterate(s, d, 5, 20, False, cam_dict())
    r1, _, i1 = S.iterate(s, d, 5, 20, False, cam_dict())
    assert r0.tolist()[3:7] == [1, 24, 0, 24] and r1.tolist()[3:7] == [2, 30, 1, 30]
    assert i0[38:62].all() and i0.sum() == 24 and i1[8:38].all() and i1.sum() == 30


def test_all_at_once_finds_what_five_at_a_time_finds():
    for name in ("hand", "scene"):
        a, b = reference(name, 5, False), reference(name, case(name)[3], False)
        for c in range(case(name)[0]["C"]):
            ret5 = [x[c][0].tolist() for x in a if x[c][0][0] == S.RETURNED]
            ret_all = [x[c][0].tolist() for x in b if x[c][0][0] == S.RETURNED]
            assert [r[5] for r in ret5] == [r[5] for r in ret_all]           # the same iterations return


# ---- the scene -------------------------------------------------------------------------------------------------------
def test_scene_returns_the_clean_set():
    sc, draws, mn, mx = case("scene")
    s = setups(sc)[0]
    assert s["n_corr"] == 64 and 123 <= s["limit"] <= 293
    first = [c[0] for c in reference("scene", 300, False) if c[0][0][0] == S.RETURNED][0]
    rep, sim3, inl = first[0], first[1], first[2]
    assert np.array_equal(np.nonzero(inl)[0], sc["clean"]) and rep[6] == 45
    s12, R12, t12 = SIM3_A
    assert abs(sim3[12] - s12) < 1e-4 and np.abs(sim3[:9].reshape(3, 3) - R12).max() < 1e-4 and np.abs(sim3[9:12] - t12).max() < 1e-3
    # every all-clean sample marks exactly the clean matches
    n = 0
    for it in range(s["limit"]):
        idx = S.sample(64, draws[0][it])
        if all(i in sc["clean"] for i in idx):
            H = S.compute_sim3([s["x1"][i] for i in idx], [s["x2"][i] for i in idx], False)
            assert np.array_equal(np.nonzero(S.check_inliers(s, H, cam_dict()))[0], sc["clean"])
            n += 1
    assert n > 20


def sim3_fp64(P1, P2):
    """ComputeSim3 restated in fp64 over numpy.linalg.eigh, from the same float inputs."""
    P1, P2 = np.asarray(P1, f64).T, np.asarray(P2, f64).T                    # columns = points
    O1, O2 = P1.mean(1, keepdims=True), P2.mean(1, keepdims=True)
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    q = V[:, 3] / np.linalg.norm(V[:, 3])
    qw, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - qw * z), 2 * (x * z + qw * y)],
                  [2 * (x * y + qw * z), 1 - 2 * (x * x + z * z), 2 * (y * z - qw * x)],
                  [2 * (x * z - qw * y), 2 * (y * z + qw * x), 1 - 2 * (x * x + y * y)]])
    P3 = R @ Pr2
    s = (Pr1 * P3).sum() / (P3 * P3).sum()
    t = O1[:, 0] - s * (R @ O2[:, 0])
    return R, t, s


# Largest |fp32 - fp64| over a seeded sample of 300 all-clean triples of the scene, measured on the CPU (the printed
# figures of test_fp32_route_against_fp64): R 1.46e-5, t 2.86e-5 m, s 1.36e-7 (one ulp of 1.7 is 1.2e-7).  The spread over triples is conditioning
# (nearly collinear samples), not noise, hence the factor 4.
FP32_R, FP32_T, FP32_S = 1.46e-5, 2.86e-5, 1.36e-7


def test_fp32_route_against_fp64():
    sc, _, _, _ = case("scene")
    s = setups(sc)[0]
    rng = np.random.default_rng(77)
    pos = {int(v): k for k, v in enumerate(s["slot1"])}
    dR = dt = ds = 0.0
    sweeps = []
    for _ in range(300):
        idx = [pos[int(i)] for i in rng.choice(sc["clean"], 3, replace=False)]
        P1, P2 = [s["x1"][i] for i in idx], [s["x2"][i] for i in idx]
        info = {}
        H = S.compute_sim3(P1, P2, False, info)
        R, t, sc64 = sim3_fp64(P1, P2)
        dR = max(dR, np.abs(np.array(H["R"], f64) - R).max())
        dt = max(dt, np.abs(np.array(H["t"], f64) - t).max())
        ds = max(ds, abs(float(H["s"]) - sc64))
        sweeps.append(info["sweeps"])
    print("fp32 vs fp64 over 300 clean triples: R %.3g t %.3g s %.3g; sweeps %s" % (dR, dt, ds, np.bincount(sweeps)))
    assert dR <= 4 * FP32_R and dt <= 4 * FP32_T and ds <= 4 * FP32_S
    assert max(sweeps) < S.JACOBI_SWEEPS                                      # the cap never decides


def test_fixed_scale():
    sc, draws, mn, mx = case("unit")
    fixed, free = reference("unit", mx, True), reference("unit", mx, False)
    r = [c[0] for c in fixed if c[0][0][0] == S.RETURNED]
    assert r and r[0][1][12] == 1.0 and r[0][0][6] == 40 and r[0][2][:40].all()
    r2 = [c[0] for c in free if c[0][0][0] == S.RETURNED]
    assert r2 and r2[0][1][12] != 1.0 and abs(r2[0][1][12] - 1.0) < 1e-4
    assert not any(c[0][0][0] == S.RETURNED for c in reference("scene", 300, True))      # s = 1.7 does not fit s = 1


def test_identity_and_degenerate_samples():
    P = [[f32(0.1), f32(0.2), f32(3.0)], [f32(-0.4), f32(0.3), f32(4.0)], [f32(0.5), f32(-0.6), f32(5.0)]]
    H = S.compute_sim3(P, P, False)                                           # the text's angle-axis route gives NaN here
    assert np.array_equal(np.array(H["R"], f32), np.eye(3, dtype=f32)) and H["s"] == 1 and not np.any(H["t"])
    Q = [P[0], P[0], P[0]]                                                    # den = 0: NaN propagates, no inliers
    H = S.compute_sim3(Q, Q, False)
    assert np.isnan(H["s"])
    sc, _, _, _ = case("hand")
    s = setups(sc)[1]
    assert not any(S.check_inliers(s, H, cam_dict()))


def test_python_mirror_declares_the_constants():
    assert (capi.SIM3_RETURNED, capi.SIM3_CONTINUE, capi.SIM3_NO_MORE, capi.SIM3_TOO_FEW) == (S.RETURNED, S.CONTINUE, S.NO_MORE,
                                                                                            S.TOO_FEW)
    assert (capi.SIM3_MATCH_POINTS, capi.SIM3_MATCH_SLOTS) == (S.MATCH_POINTS, S.MATCH_SLOTS)
    from orb_slam2_comment_amd import sim3_draws
    d = sim3_draws(3, 50, [5, 2, 64], 1)
    assert d.shape == (3, 50, 3) and d.dtype == i32 and not d[1].any()
    for k in range(3):
        assert d[0, :, k].min() >= 0 and d[0, :, k].max() <= 4 - k and d[2, :, k].max() <= 63 - k
    assert len(np.unique(d[2, :, 0])) > 20
