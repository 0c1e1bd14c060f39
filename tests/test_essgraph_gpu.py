"""Essential-graph optimisation on the device against the sequential reference (tests/seqref/essgraph.py), byte for byte.

The cases are built in test_essgraph_cpu.py and their reference answers are computed once per process: the hand-built graph, 6
rows with one loop connection and its fix_scale twin, 3 / 4 / 5 free vertices around a panel of 4 poses and 7 / 8 / 9 around two
(9 spans three panels and is no multiple), 37 rows (nine panels), a bad row, the point scene, null vertices (device form only: the host form refuses them), max_edges exceeded
by one and 513 rows that are not bad (ORBHIP_EG_CAPACITY: only the report is written).  Tcw, world, the point list, Scw, Swc
and the report must equal the reference through the device form and through the host form; what a call must not write keeps the
sentinel the test put there."""
import numpy as np
import pytest

import test_essgraph_cpu as K

pytestmark = pytest.mark.gpu
f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    m = pkg.ORBmatcher(0.6, True)
    yield dict(pkg=pkg, m=m)
    m.close()


def run_device(env, b, tables=None):
    import torch
    dev = torch.device("cuda")
    t = b["tables"] if tables is None else tables
    o = K.prefilled(b)
    up = lambda a: None if a is None or a.size == 0 else torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_t = {k: up(t[k]) for k in K.TABLE_KEYS}
    d_o = {k: up(o[k]) for k in o}
    torch.cuda.synchronize()
    env["m"].OptimizeEssentialGraphDevice(b["cur"], b["loop_row"], b["rows"], b["pcap"], d_t, b["fix_scale"], b["max_edges"], d_o)
    got = {k: (o[k] if d_o[k] is None else d_o[k].cpu().numpy().view(o[k].dtype).reshape(o[k].shape)) for k in o}
    got["Tcw"] = d_t["Tcw"].cpu().numpy().view(f32).reshape(-1, 12)
    got["world"] = t["world"] if d_t["world"] is None else d_t["world"].cpu().numpy().view(f32).reshape(-1, 3)
    return got


def run_host(env, b, tables=None):
    t = b["tables"] if tables is None else tables
    return env["m"].OptimizeEssentialGraph(t, b["cur"], b["loop_row"], b["fix_scale"], b["max_edges"], fill=K.SENTINEL)


@pytest.mark.parametrize("name", K.CASES)
def test_device_equals_seqref(env, name):
    K.assert_same(run_device(env, K.case(name)), K.reference(name), name)


@pytest.mark.parametrize("name", K.HOST_FORM_CASES)
def test_host_form_equals_seqref(env, name):
    K.assert_same(run_host(env, K.case(name)), K.reference(name), name)


def test_the_call_synchronises_once_per_trial(env):
    b = K.case("p9")
    run_device(env, b)
    syncs, launches = env["m"].EssentialGraphCounters()
    rep = K.reference("p9")["raw"]["report"]
    assert syncs == 1 + rep[9] + 1 and launches > syncs                        # the setup, every trial, the epilogue


def test_refusals_with_a_live_handle(env):
    from orb_slam2_comment_amd import capi
    b = K.case("r6")
    for bad in (dict(cur=b["rows"]), dict(loop_row=-1), dict(max_edges=0)):
        with pytest.raises(capi.OrbHipError) as ei:
            run_host(env, dict(b, **bad))
        assert ei.value.code == capi.E_ARG
    nb = K.case("nullv")                                                       # a bad parent, a bad loop_kf entry, a bad lc_kf entry
    with pytest.raises(capi.OrbHipError) as ei:
        run_host(env, nb)
    assert ei.value.code == capi.E_ARG
    ok = K.case("bad9")["tables"]
    for keys in (("parent",), ("loop_start", "loop_kf"), ("lc_start", "lc_kf")):
        with pytest.raises(capi.OrbHipError) as ei:
            run_host(env, nb, tables=dict(ok, **{k: nb["tables"][k] for k in keys}))
        assert ei.value.code == capi.E_ARG, keys
    rows = 5000
    z = np.zeros(rows, i32)
    t = dict(b["tables"], kf_bad=None, kf_id=z, parent=z - 1, conn_w=np.zeros((1, 1), i32), ord_kf=np.zeros((1, 1), i32),
             ord_w=np.zeros((1, 1), i32), n_ord=z, loop_start=np.zeros(rows + 1, i32), lc_start=np.zeros(rows + 1, i32),
             corrected=np.zeros((1, 8)), non_corrected=np.zeros((1, 8)), in_corrected=z.astype(u8), in_non_corrected=z.astype(u8),
             Tcw=np.zeros((rows, 12), f32))
    with pytest.raises(capi.OrbHipError) as ei:                                 # rows above 4096, refused before the tables are read
        run_host(env, b, tables=t)
    assert ei.value.code == capi.E_CAPACITY
