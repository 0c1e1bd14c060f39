"""Global bundle adjustment and its map update on the device against the sequential reference (tests/seqref/gba.py), byte for
byte.

The cases are built in test_gba_cpu.py and their reference answers are computed once per process: the hand-worked rules (a bad
listed row, a bad point, a point with bad observers only, a row newer than maxKFid, a null vertex, monocular / stereo / mixed
scenes, Huber on and off, both modes, the stop byte set and clear, no id-0 row, max_points / max_edges exceeded by one, 513 good
rows, a point list, no point at all), 3 / 4 / 5 and 8 / 9 free poses around the panel of 4 poses and its double, 37 free poses
(ten panels, the last one short), and a scene with a pose of 70 edges and a point of 18.  Every output must equal the reference
through the device form and through the host form; what a call must not write keeps the sentinel the test put there."""
import numpy as np
import pytest

import test_gba_cpu as K
from seqref import gba as G

pytestmark = pytest.mark.gpu
f32, i32, u8 = np.float32, np.int32, np.uint8


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(*K.CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=K.CAM[4])
    yield dict(pkg=pkg, m=m, cam=cam)
    m.close()


def up(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).to(torch.device("cuda"))


def down(d, like):
    return d.cpu().numpy().view(like.dtype).reshape(like.shape)


def run_device(env, b, tables=None, keep=None):
    """The device form; returns the outputs and (in `keep`) the device arrays themselves."""
    import torch
    t = b["tables"] if tables is None else tables
    o = K.prefilled(b)
    d_t = {k: up(t[k]) for k in K.TABLE_KEYS}
    d_o = {k: up(o[k]) for k in o}
    d_kl = None if b["kf_list"] is None else up(np.array(list(b["kf_list"]) + [0], i32))
    d_pl = None if b["pt_list"] is None else up(np.array(list(b["pt_list"]) + [0], i32))
    d_stop = None if b["stop"] is None else up(np.array([b["stop"]], u8))
    torch.cuda.synchronize()
    env["m"].GlobalBundleAdjustmentDevice(env["cam"], b["rows"], b["cap"], b["np"], b["pcap"], d_t, K.INV_SIGMA2, b["iterations"],
                                          b["robust"], b["mode"], b["max_points"], b["max_edges"], d_o, d_kf_list=d_kl,
                                          nkf=0 if b["kf_list"] is None else len(b["kf_list"]), d_pt_list=d_pl,
                                          npt=0 if b["pt_list"] is None else len(b["pt_list"]), d_stop=d_stop)
    got = {k: down(d_o[k], o[k]) for k in o}
    got["Tcw"], got["world"] = down(d_t["Tcw"], t["Tcw"]), down(d_t["world"], t["world"])
    for k in K.TABLE_KEYS:                                                      # the inputs are inputs
        if k not in ("Tcw", "world") and t[k] is not None:
            assert down(d_t[k], t[k]).tobytes() == np.ascontiguousarray(t[k]).tobytes(), k
    if keep is not None:
        keep.update(tables=d_t, out=d_o)
    return got


def run_host(env, b, tables=None):
    t = b["tables"] if tables is None else tables
    return env["m"].GlobalBundleAdjustment(t, env["cam"], K.INV_SIGMA2, b["iterations"], b["robust"], b["mode"], b["max_points"],
                                           b["max_edges"], kf_list=b["kf_list"], pt_list=b["pt_list"], stop=b["stop"],
                                           out=K.prefilled(b), fill=K.SENTINEL)


@pytest.mark.parametrize("name", K.CASES)
def test_device_equals_seqref(env, name):
    K.assert_same(run_device(env, K.case(name)), K.reference(name), name)
    syncs, launches = env["m"].GlobalBACounters()
    trials = int(K.reference(name)["report"][10])
    assert syncs == 1 + trials + 1 and launches >= 4, (syncs, trials, launches)


@pytest.mark.parametrize("name", [n for n in K.CASES if n != "null_vertex"])
def test_host_form_equals_seqref(env, name):
    K.assert_same(run_host(env, K.case(name)), K.reference(name), name)


def test_host_form_refuses_a_null_vertex(env):
    from orb_slam2_comment_amd import capi
    with pytest.raises(capi.OrbHipError) as ei:
        run_host(env, K.case("null_vertex"))
    assert ei.value.code == capi.E_ARG


def test_second_call_on_the_first_calls_outputs(env):
    b = K.case("in_place")
    first = K.reference("in_place")
    want = K.run_seqref(dict(b, tables=dict(b["tables"], Tcw=first["Tcw"], world=first["world"])))
    got1 = run_device(env, b)
    got2 = run_device(env, b, tables=dict(b["tables"], Tcw=got1["Tcw"], world=got1["world"]))
    K.assert_same(got2, want, "in_place twice")


def test_apply_device_and_host_equal_seqref(env):
    import torch
    for name in ("tree", "no_bad"):
        a, ref = K.apply_case(name), K.apply_reference(name)
        o = K.apply_prefilled(a)
        d = {k: up(v) for k, v in dict(a, **o).items()}
        torch.cuda.synchronize()
        env["m"].ApplyGlobalBADevice(len(a["origins"]), len(a["parent"]), len(a["flags"]), d)
        env["m"].sync()
        full = dict(a, **o)
        got = {k: down(d[k], np.ascontiguousarray(full[k])) for k in K.APPLY_KEYS}
        K.assert_same_apply(got, ref, name + " device")
        for k in ("origins", "parent", "pt_mark", "posGBA", "flags", "ref_kf"):
            assert down(d[k], a[k]).tobytes() == np.ascontiguousarray(a[k]).tobytes(), k
        K.assert_same_apply(env["m"].ApplyGlobalBA(a, fill=K.SENTINEL), ref, name + " host")


def test_full_chain_on_device_arrays(env):
    """GlobalBundleAdjustment STAGED -> ApplyGlobalBA -> UpdateMapPoints(NORMAL_DEPTH), never leaving the device, against the
    same chain of sequential references.  Row 4 is left out of the adjustment (its kf_id is the newest) and is corrected through
    its parent; a point seen by row 4 alone moves through its reference row."""
    import torch
    import test_seqref_projection_cpu as PC
    from seqref import mappoint as MP
    sc = K.make_scene(36, 5, 14, 16, pcap=16)
    p_only4 = sc.point([1.0, 0.3, 9.0])
    sc.observe(p_only4, 4)
    b = K._case(sc, kf_list=[0, 1, 2, 3])
    t = b["tables"]
    rows, pcap, npts = b["rows"], b["pcap"], b["np"]
    parent = np.array([-1, 0, 1, 2, 3], i32)
    ref_kf = np.array([int(t["obs_kf"][t["obs_start"][p]]) if p < npts else -1 for p in range(pcap)], i32)
    # the references
    r1 = K.run_seqref(b)
    assert r1["kf_mark"].tolist() == [1, 1, 1, 1, 0] and r1["pt_mark"][p_only4] == 0 and r1["report"][7] >= 1
    arrays = dict(origins=np.array([0], i32), parent=parent, kf_bad=t["kf_bad"], kf_mark=r1["kf_mark"], TcwGBA=r1["TcwGBA"], Tcw=t["Tcw"],
                  pt_mark=r1["pt_mark"], posGBA=r1["posGBA"], flags=t["flags"], ref_kf=ref_kf, world=t["world"])
    r2 = G.apply_global_ba(dict(arrays, TcwBefGBA=K.apply_prefilled(arrays)["TcwBefGBA"]))
    assert r2["report"][:5] == [5, 1, 14, 1, 0]
    cam_c, cam_s = PC.make_cam()
    keys = [t["kps"][r] for r in range(rows)]
    sent = lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, K.SENTINEL, u8).view(dt).reshape(shape)  # noqa: E731
    pd0, n0, mx0, mn0 = sent((pcap, 32), u8), sent((pcap, 3), f32), sent(pcap, f32), sent(pcap, f32)
    ref_obs = np.zeros(pcap, i32)
    total = int(t["obs_start"][-1])
    r3 = MP.update_map_points(cam_s, MP.UPDATE_NORMAL_DEPTH, [T.reshape(3, 4) for T in r2["Tcw"]], keys, None, t["kf_bad"], t["obs_start"],
                              t["obs_kf"][:total], t["obs_idx"][:total], ref_obs, r2["world"], t["flags"], pd0, n0, mx0, mn0)
    # the device chain
    keep = {}
    got1 = run_device(env, b, keep=keep)
    K.assert_same(got1, r1, "chain: adjustment")
    o = K.apply_prefilled(arrays)
    d = dict(origins=up(arrays["origins"]), parent=up(parent), kf_bad=keep["tables"]["kf_bad"], kf_mark=keep["out"]["kf_mark"],
             TcwGBA=keep["out"]["TcwGBA"], Tcw=keep["tables"]["Tcw"], pt_mark=keep["out"]["pt_mark"], posGBA=keep["out"]["posGBA"],
             flags=keep["tables"]["flags"], ref_kf=up(ref_kf), world=keep["tables"]["world"], TcwBefGBA=up(o["TcwBefGBA"]),
             report=up(o["report"]))
    env["m"].ApplyGlobalBADevice(1, rows, pcap, d)
    d_desc = torch.zeros(rows * b["cap"] * 32, dtype=torch.uint8, device="cuda")
    d_n = up(np.full(rows, b["cap"], i32))
    outs = [up(a) for a in (pd0, n0, mx0, mn0)]
    d_status = torch.full((pcap,), 0x77, dtype=torch.uint8, device="cuda")
    d_ref = up(ref_obs)
    env["m"].UpdateMapPointsDevice(cam_c, MP.UPDATE_NORMAL_DEPTH, d["Tcw"].data_ptr(), keep["tables"]["kps"].data_ptr(), d_desc.data_ptr(),
                                   d_n.data_ptr(), b["cap"], npts, pcap, keep["tables"]["obs_start"].data_ptr(),
                                   keep["tables"]["obs_kf"].data_ptr(), keep["tables"]["obs_idx"].data_ptr(), d_ref.data_ptr(),
                                   d["world"].data_ptr(), d["flags"].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                   outs[2].data_ptr(), outs[3].data_ptr(), d_status.data_ptr(), d_kf_bad=d["kf_bad"].data_ptr())
    env["m"].sync()
    full = dict(arrays, **o)
    K.assert_same_apply({k: down(d[k], np.ascontiguousarray(full[k])) for k in K.APPLY_KEYS},
                        dict(r2, report=np.array(r2["report"], i32)), "chain: apply")
    for got, want, nm in zip(outs[1:], r3[1:4], ("normal", "max_dist", "min_dist")):
        assert down(got, want)[:npts].tobytes() == np.ascontiguousarray(want)[:npts].tobytes(), nm
    assert d_status.cpu().numpy()[:npts].tolist() == r3[5].tolist()


def test_refusals_with_a_live_handle(env):
    from orb_slam2_comment_amd import capi
    b = K.case("base")
    for bad in (dict(iterations=0), dict(mode=2), dict(max_points=0), dict(max_edges=0), dict(kf_list=[0, 1, 1]), dict(kf_list=[0, 9]),
                dict(pt_list=[0, 99]), dict(kf_list=[0, 1, 2, 3, 4, 0])):
        with pytest.raises(capi.OrbHipError) as ei:
            run_host(env, dict(b, **bad))
        assert ei.value.code == capi.E_ARG, bad
    t = dict(b["tables"], obs_kf=b["tables"]["obs_kf"].copy())
    t["obs_kf"][0] = b["rows"]
    with pytest.raises(capi.OrbHipError) as ei:
        run_host(env, b, tables=t)
    assert ei.value.code == capi.E_ARG
    t = dict(b["tables"], kf_bad=None, kf_id=np.zeros(5000, i32), kps=np.zeros((5000, 1), K.K.KP_DTYPE), u_right=None,
             Tcw=np.zeros((5000, 12), f32))
    with pytest.raises(capi.OrbHipError) as ei:                                 # rows above 4096, refused before the tables are read
        run_host(env, b, tables=t)
    assert ei.value.code == capi.E_CAPACITY
    a = K.apply_case()
    with pytest.raises(capi.OrbHipError) as ei:
        env["m"].ApplyGlobalBA(dict(a, origins=np.array([2], i32)))
    assert ei.value.code == capi.E_ARG
    with pytest.raises(capi.OrbHipError) as ei:
        env["m"].ApplyGlobalBA(dict(a, parent=np.array([-1, 0, 0, 2, 0, 4, -1, 6, 9], i32)))
    assert ei.value.code == capi.E_ARG
