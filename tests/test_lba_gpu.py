"""Local bundle adjustment on the device against the sequential reference (tests/seqref/lba.py), byte for byte.

The cases are built in test_lba_cpu.py and their reference answers are computed once per process: the hand-worked lists,
scene S (mixed and monocular only), scene M (a pose with 65 edges, a point with one observation, a point with 18, outliers, a
point and a pose that leave the system of round 2), the rule-4 scene, a point at zero depth, max_edges and max_points exceeded
by one, the stop byte set and clear, and a window without a point.  The lists, the erase rows, Tcw, world and the report must
equal the reference through the device form and through the host form; what a call must not write keeps the sentinel the
test put there."""
import numpy as np
import pytest

import test_lba_cpu as K

pytestmark = pytest.mark.gpu
f32, i32, u8 = np.float32, np.int32, np.uint8
TABLE_KEYS = ("slot_point", "n", "kf_bad", "obs_start", "obs_kf", "obs_idx", "flags", "kps", "u_right", "ord_kf", "n_ord", "Tcw", "world")


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(*K.CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=K.CAM[4])
    yield dict(pkg=pkg, m=m, cam=cam)
    m.close()


def run_device(env, b, tables=None):
    import torch
    dev = torch.device("cuda")
    t = b["tables"] if tables is None else tables
    o = K.prefilled(b)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_t = {k: up(t[k]) for k in TABLE_KEYS}
    d_o = {k: up(o[k]) for k in o}
    d_stop = None if b["stop"] is None else up(np.array([b["stop"]], u8))
    torch.cuda.synchronize()
    env["m"].LocalBundleAdjustmentDevice(b["cur"], b["id0_row"], env["cam"], b["rows"], b["cap"], b["np"], b["pcap"], d_t, K.INV_SIGMA2,
                                         b["max_points"], b["max_edges"], d_o, d_stop=d_stop)
    env["m"].sync()
    got = {k: d_o[k].cpu().numpy().view(o[k].dtype).reshape(o[k].shape) for k in o}
    got["Tcw"] = d_t["Tcw"].cpu().numpy().view(f32).reshape(-1, 12)
    got["world"] = d_t["world"].cpu().numpy().view(f32).reshape(-1, 3)
    return got


def run_host(env, b, tables=None):
    t = b["tables"] if tables is None else tables
    got = env["m"].LocalBundleAdjustment(t, b["cur"], b["id0_row"], env["cam"], K.INV_SIGMA2, b["max_points"], b["max_edges"],
                                         stop=b["stop"], fill=K.SENTINEL)
    return got


@pytest.mark.parametrize("name", K.CASES)
def test_device_equals_seqref(env, name):
    K.assert_same(run_device(env, K.case(name)), K.reference(name), name)


@pytest.mark.parametrize("name", K.CASES)
def test_host_form_equals_seqref(env, name):
    K.assert_same(run_host(env, K.case(name)), K.reference(name), name)


def test_second_call_on_the_outputs_of_the_first(env):
    b = K.case("S")
    first = K.reference("S")
    t2 = dict(b["tables"], Tcw=first["Tcw"], world=first["world"])
    want = K.as_arrays(b, K.run_seqref(dict(b, tables=t2)))
    got1 = run_device(env, b)
    got2 = run_device(env, b, tables=dict(b["tables"], Tcw=got1["Tcw"], world=got1["world"]))
    K.assert_same(got2, want, "S twice")


def test_refusals_with_a_live_handle(env):
    from orb_slam2_comment_amd import capi
    b = K.case("S")
    for bad in (dict(cur=b["rows"]), dict(id0_row=-2), dict(max_points=0), dict(max_edges=0)):
        with pytest.raises(capi.OrbHipError) as ei:
            run_host(env, dict(b, **bad))
        assert ei.value.code == capi.E_ARG
    t = dict(b["tables"], obs_kf=b["tables"]["obs_kf"].copy())
    t["obs_kf"][0] = b["rows"]
    with pytest.raises(capi.OrbHipError) as ei:
        run_host(env, b, tables=t)
    assert ei.value.code == capi.E_ARG
    t = dict(b["tables"], slot_point=np.full((5000, 1), -1, i32), n=np.zeros(5000, i32), kf_bad=None, kps=np.zeros((5000, 1), K.KP_DTYPE),
             u_right=None, ord_kf=np.zeros((1, 1), i32), n_ord=np.zeros(5000, i32), Tcw=np.zeros((5000, 12), f32))
    with pytest.raises(capi.OrbHipError) as ei:                                 # rows above 4096, refused before the tables are read
        run_host(env, b, tables=t)
    assert ei.value.code == capi.E_CAPACITY
