"""Sim3 optimisation on the device against the sequential reference (tests/seqref/sim3opt.py), byte for byte.

Inputs (built in test_sim3opt_cpu.py, the reference answers are computed once per process): two batches of three candidates
at cap 512 with 0, 9 and 12 pairs and with 64, 65 (the second wavefront holds one pair) and 257 pairs (lane 0 holds two).
Device form and host form, both forms of matched12, the scale free and fixed, d_select skipping the middle candidate, d_Scw
NULL, a candidate alone against its row of the batch.  Every output, the in/out matches and the report must equal the
reference; what a call must not write keeps the sentinel."""
import numpy as np
import pytest

import test_sim3opt_cpu as K
from seqref import sim3 as S3
from seqref import sim3opt as Q

pytestmark = pytest.mark.gpu
FILL = K.SENTINEL
f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(K.CAM[0], K.CAM[1], K.CAM[2], K.CAM[3], (0.0, 0.0, 640.0, 480.0), [1.2 ** l for l in range(8)])
    yield dict(pkg=pkg, m=m, cam=cam)
    m.close()


def device_form(env, sc, sim3, form, fix_scale, select=None, want_scw=True):
    """OptimizeSim3Device over torch tensors: dict(matched12, S12, Scw, report) read back."""
    import torch
    m = env["m"]
    T, rows, cap, n_pts, pcap = m._sim3_tables(sc["T"])
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).to(dev)  # noqa: E731
    dT = {k: up(v) for k, v in T.items()}
    Cn = sc["C"]
    matched = sc["m_points"] if form == S3.MATCH_POINTS else sc["m_slots"]
    d_kf, d_m, d_sim3 = up(sc["kf_index"]), up(matched.astype(i32)), up(sim3.astype(f32))
    d_sel = None if select is None else up(np.array(select, u8))
    d_S12 = torch.full((Cn * 64,), FILL, dtype=torch.uint8, device=dev)
    d_Scw = torch.full((Cn * 48,), FILL, dtype=torch.uint8, device=dev)
    d_rep = torch.full((Cn * 32,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    m.OptimizeSim3Device(Cn, sc["cur"], d_kf, env["cam"], rows, cap, n_pts, pcap, dT, form, K.INV_SIGMA2, d_m, d_sim3, d_S12,
                         d_Scw if want_scw else None, d_rep, K.TH2, fix_scale, d_sel)
    m.sync()
    return dict(matched12=d_m.cpu().numpy().view(i32).reshape(Cn, cap), S12=d_S12.cpu().numpy().view(f64).reshape(Cn, 8),
                Scw=d_Scw.cpu().numpy().view(f32).reshape(Cn, 12), report=d_rep.cpu().numpy().view(i32).reshape(Cn, 8))


def host_form(env, sc, sim3, form, fix_scale, select=None, want_scw=True):
    matched = sc["m_points"] if form == S3.MATCH_POINTS else sc["m_slots"]
    r = env["m"].OptimizeSim3(sc["T"], sc["cur"], sc["kf_index"], env["cam"], matched, form, K.INV_SIGMA2, sim3, K.TH2, fix_scale,
                              select, want_scw, fill=FILL)
    if r["Scw"] is None:
        r["Scw"] = np.full(sc["C"] * 48, FILL, u8).view(f32).reshape(sc["C"], 12)
    return r


MODES = [(S3.MATCH_POINTS, False), (S3.MATCH_SLOTS, False), (S3.MATCH_POINTS, True), (S3.MATCH_SLOTS, True)]


@pytest.mark.parametrize("name,mode", [(n, k) for n in ("A", "B") for k in range(4)])
def test_device_equals_seqref(env, name, mode):
    sc, sim3 = K.case(name)
    form, fix = MODES[mode]
    K.assert_same(device_form(env, sc, sim3, form, fix), K.reference(name, form, fix), (name, mode))


@pytest.mark.parametrize("name,mode", [("A", 1), ("B", 0), ("B", 3)])
def test_host_form_equals_seqref(env, name, mode):
    sc, sim3 = K.case(name)
    form, fix = MODES[mode]
    K.assert_same(host_form(env, sc, sim3, form, fix), K.reference(name, form, fix), (name, mode))


def test_select_skips_the_middle_candidate(env):
    sc, sim3 = K.case("B")
    want = K.reference("B", S3.MATCH_POINTS, False, (1, 0, 1))
    assert want["report"][1][0] == Q.SKIPPED and (want["S12"][1].view(u8) == FILL).all()
    K.assert_same(device_form(env, sc, sim3, S3.MATCH_POINTS, False, (1, 0, 1)), want, "device")
    K.assert_same(host_form(env, sc, sim3, S3.MATCH_POINTS, False, (1, 0, 1)), want, "host")


def test_scw_null(env):
    sc, sim3 = K.case("A")
    want = dict(K.reference("A"))
    want["Scw"] = np.full(3 * 48, FILL, u8).view(f32).reshape(3, 12)
    K.assert_same(device_form(env, sc, sim3, S3.MATCH_POINTS, False, want_scw=False), want, "device")
    K.assert_same(host_form(env, sc, sim3, S3.MATCH_POINTS, False, want_scw=False), want, "host")


def test_candidate_alone_equals_its_row_of_the_batch(env):
    sc, sim3 = K.case("A_alone")
    alone = device_form(env, sc, sim3, S3.MATCH_POINTS, False)
    batch = K.reference("A")
    for k in ("matched12", "S12", "Scw", "report"):
        assert alone[k][0].tobytes() == batch[k][2].tobytes(), k


def test_refusals_with_a_live_handle(env):
    m, capi = env["m"], env["pkg"].capi
    sc, sim3 = K.case("A")
    args = (sc["T"], sc["cur"], sc["kf_index"], env["cam"], sc["m_points"], S3.MATCH_POINTS, K.INV_SIGMA2, sim3)

    def code(*a, **k):
        with pytest.raises(env["pkg"].OrbHipError) as e:
            m.OptimizeSim3(*a, **k)
        return e.value.code
    assert code(*args, th2=0.0) == capi.E_ARG
    assert code(*args, th2=float("nan")) == capi.E_ARG
    assert code(*args[:5], 2, *args[6:]) == capi.E_ARG                           # match_form
    assert code(sc["T"], sc["rows"], *args[2:]) == capi.E_ARG                    # cur outside the bank
    assert code(sc["T"], sc["cur"], sc["kf_index"] + 100, *args[3:]) == capi.E_ARG
    bad = sc["m_points"].copy()
    bad[2, 0] = sc["np"]
    assert code(*args[:4], bad, *args[5:]) == capi.E_ARG
    T = dict(sc["T"], obs_kf=np.where(np.arange(len(sc["T"]["obs_kf"])) == 5, 99, sc["T"]["obs_kf"]).astype(i32))
    assert code(T, *args[1:]) == capi.E_ARG
    kps = sc["T"]["kps"].copy()
    kps["octave"][sc["cur"], 0] = 8
    assert code(dict(sc["T"], kps=kps), *args[1:]) == capi.E_ARG
    big = dict(sc["T"], slot_point=np.full((sc["rows"], 4097), -1, i32), kps=np.zeros((sc["rows"], 4097), capi.KP_DTYPE))
    assert code(big, sc["cur"], sc["kf_index"], env["cam"], np.full((3, 4097), -1, i32), *args[5:]) == capi.E_CAPACITY
    # the device form refuses before any device work: null pointers never reach a kernel
    with pytest.raises(env["pkg"].OrbHipError) as e:
        m.OptimizeSim3Device(3, sc["cur"], 0, env["cam"], sc["rows"], sc["cap"], sc["np"], sc["pcap"],
                             {k: 16 for k in m.SIM3_TABLES}, S3.MATCH_POINTS, K.INV_SIGMA2, 0, 0, 0, None, 0)
    assert e.value.code == capi.E_ARG
    # an empty batch: success, nothing written
    r = m.OptimizeSim3(sc["T"], sc["cur"], np.zeros(0, i32), env["cam"], np.zeros((0, sc["cap"]), i32), S3.MATCH_POINTS,
                       K.INV_SIGMA2, np.zeros((0, 16), f32))
    assert r["report"].shape == (0, 8) and r["S12"].shape == (0, 8)
    # the handle still works
    K.assert_same(host_form(env, *K.case("A_alone"), S3.MATCH_POINTS, False), K.reference("A_alone"), "after")
