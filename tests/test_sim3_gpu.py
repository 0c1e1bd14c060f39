"""Sim3 RANSAC on the device against the sequential reference (tests/seqref/sim3.py), byte for byte.

Inputs (built in test_sim3_cpu.py, the reference answers are computed once per process): the hand-worked cases, the
64-match scene with a known Sim3, a scene of scale 1 for mbFixScale, and one batch of five candidates with N = 0, 3, 19,
65 and 257 correspondences (min_inliers = 3), which are the boundaries between 16-lane teams and wavefronts and between
one and several rounds of a team.  Each runs five iterations at a time until every candidate is done and with all iterations in one call, with the
scale free and fixed and with both forms of matched12; entries behind the counts must keep the fill pattern.  The host
form must agree with the device form."""
import numpy as np
import pytest

import test_sim3_cpu as K
from seqref import sim3 as S

pytestmark = pytest.mark.gpu
FILL = 0x5A
f32, i32, u8 = np.float32, np.int32, np.uint8


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(K.CAM["fx"], K.CAM["fy"], K.CAM["cx"], K.CAM["cy"], (0.0, 0.0, 640.0, 480.0), [1.2 ** l for l in range(8)])
    yield dict(pkg=pkg, m=m, cam=cam)
    m.close()


def check_setup(host, refs, cap):
    for c, r in enumerate(refs):
        N = r["n_corr"]
        assert host["n_corr"][c] == N and host["n1"][c] == r["n1"] and host["limit"][c] == r["limit"], c
        assert host["state"][c].tolist() == [0, 0]
        for k in ("x1", "x2", "p1", "p2", "max_err1", "max_err2", "slot1"):
            a = host[k][c]
            assert a[:N].tobytes() == r[k].tobytes(), (c, k)
            assert (a[N:].view(u8) == FILL).all(), (c, k)


def check_call(out, ref_call, n1s, solver_state, what):
    rep, sim3, inl = out
    for c, (r_rep, r_sim3, r_inl, r_state) in enumerate(ref_call):
        assert rep[c].tolist() == r_rep.tolist(), (what, c)
        if r_sim3 is None:
            assert (sim3[c].view(u8) == FILL).all(), (what, c)
        else:
            assert sim3[c].tobytes() == r_sim3.tobytes(), (what, c)
        n1 = n1s[c]
        assert np.array_equal(inl[c][:n1], r_inl) and (inl[c][n1:] == FILL).all(), (what, c)
        if r_rep[0] != S.TOO_FEW:
            assert solver_state[c].tolist() == r_state, (what, c)


def modes(name):
    mx = K.case(name)[3]
    if name == "unit":
        return [(5, True, S.MATCH_POINTS), (mx, True, S.MATCH_POINTS), (mx, False, S.MATCH_POINTS), (mx, True, S.MATCH_SLOTS)]
    return [(5, False, S.MATCH_POINTS), (mx, False, S.MATCH_POINTS), (mx, True, S.MATCH_POINTS), (mx, False, S.MATCH_SLOTS)]


@pytest.mark.parametrize("name,mode", [(n, k) for n in ("hand", "scene", "unit", "batch") for k in range(4)])
def test_device_equals_seqref(env, name, mode):
    sc, draws, mn, mx = K.case(name)
    n_iterations, fix_scale, form = modes(name)[mode]
    ref = K.reference(name, n_iterations, fix_scale)
    refs = K.setups(sc, 0.99, mn, mx)
    m = env["m"]
    matched = sc["m_points"] if form == S.MATCH_POINTS else sc["m_slots"]
    solver = m.Sim3Setup(sc["T"], sc["cur"], sc["kf_index"], env["cam"], matched, form, K.SIGMA2, 0.99, mn, mx, fill=FILL)
    check_setup(solver["host"], refs, sc["cap"])
    n1s = [r["n1"] for r in refs]
    returned = 0
    for t, ref_call in enumerate(ref):
        out = m.Sim3Iterate(solver, draws, n_iterations, fix_scale, fill=FILL)
        check_call(out, ref_call, n1s, solver["host"]["state"], (name, mode, t))
        returned += int((out[0][:, 0] == S.RETURNED).sum())
    assert all(r[0][0] in (S.NO_MORE, S.TOO_FEW) for r in ref[-1])
    assert returned > 0 or (fix_scale and name != "unit")                     # a fixed scale of 1 fits only the unit scene


def test_batch_covers_the_boundaries(env):
    sc, draws, mn, mx = K.case("batch")
    refs = K.setups(sc, 0.99, mn, mx)
    assert [r["n_corr"] for r in refs] == list(K.BATCH_N) and [r["limit"] for r in refs] == [0, 1, 70, 70, 70]
    first = K.reference("batch", mx, False)[0]
    assert first[0][0][0] == S.TOO_FEW and first[1][0][0] == S.NO_MORE        # 3 inliers are not > 3


def test_host_form_equals_device_form(env):
    m = env["m"]
    for name in ("hand", "batch"):
        sc, draws, mn, mx = K.case(name)
        ref = K.reference(name, mx, False)
        r = m.Sim3Ransac(sc["T"], sc["cur"], sc["kf_index"], env["cam"], sc["m_slots"], S.MATCH_SLOTS, K.SIGMA2, draws, False,
                         0.99, mn, mx, fill=FILL)
        n1s = [int(sc["T"]["n"][sc["cur"]])] * sc["C"]
        check_call((r["report"], r["sim3"], r["inliers"]), ref[0], n1s, r["state"], (name, "host"))
    # five at a time, resumed through the state
    sc, draws, mn, mx = K.case("hand")
    ref = K.reference("hand", 5, False)
    state = None
    for t in range(4):
        r = m.Sim3Ransac(sc["T"], sc["cur"], sc["kf_index"], env["cam"], sc["m_points"], S.MATCH_POINTS, K.SIGMA2, draws, False,
                         0.99, mn, mx, n_iterations=5, state=state, fill=FILL)
        check_call((r["report"], r["sim3"], r["inliers"]), ref[t], [70] * sc["C"], r["state"], ("hand", "host", t))
        state = r["state"]


def test_host_form_refuses_what_it_checks(env):
    m, capi = env["m"], env["pkg"].capi
    sc, draws, mn, mx = K.case("hand")
    args = (sc["T"], sc["cur"], sc["kf_index"], env["cam"], sc["m_points"], S.MATCH_POINTS, K.SIGMA2)

    def code(*a, **k):
        with pytest.raises(env["pkg"].OrbHipError) as e:
            m.Sim3Ransac(*a, **k)
        return e.value.code
    bad = draws.copy()
    bad[1, 0, 2] = 23                                                         # N = 25: the third draw ends at 22
    assert code(*args, bad) == capi.E_ARG
    bad = draws.copy()
    bad[1, 0, 0] = -1
    assert code(*args, bad) == capi.E_ARG
    bad[1, 0, 0] = 0
    bad[1, 7, 0] = 99                                                         # behind the limit of 7: never read
    m.Sim3Ransac(*args, bad)
    assert code(*args, draws, min_inliers=2) == capi.E_ARG
    assert code(*args, draws, prob=1.0) == capi.E_ARG
    T = dict(sc["T"], obs_kf=np.where(np.arange(len(sc["T"]["obs_kf"])) == 5, 99, sc["T"]["obs_kf"]).astype(i32))
    assert code(T, *args[1:], draws) == capi.E_ARG
    assert code(sc["T"], sc["cur"], sc["kf_index"] + 100, *args[3:], draws) == capi.E_ARG
    # capacity and an empty batch
    big = dict(sc["T"], slot_point=np.full((sc["rows"], 4097), -1, i32), kps=np.zeros((sc["rows"], 4097), capi.KP_DTYPE))
    assert code(big, sc["cur"], sc["kf_index"], env["cam"], np.full((sc["C"], 4097), -1, i32), S.MATCH_POINTS, K.SIGMA2,
                draws) == capi.E_CAPACITY
    r = m.Sim3Ransac(sc["T"], sc["cur"], np.zeros(0, i32), env["cam"], np.zeros((0, sc["cap"]), i32), S.MATCH_POINTS, K.SIGMA2,
                     np.zeros((0, 300, 3), i32))
    assert r["report"].shape == (0, 8)
