"""orbhip_update_connections_device / orbhip_update_connections (KeyFrame::UpdateConnections over tables),
orbhip_covisible_targets* and orbhip_children_from_parents_device against tests/seqref/covisibility.py, byte for byte: the
scenes of test_covisibility_cpu.py (bank sizes around a wavefront and around a 256-thread pass, a list of rows - 1 entries,
observation lists of 17 and 33 entries), update lists of 0, 1 and 3 entries with a repeat, two calls on one handle, the host
entries against the device entries, and the two chains: into the local map and into the batched fuse."""
import numpy as np
import pytest

import test_covisibility_cpu as CC
from seqref import covisibility as CV

pytestmark = pytest.mark.gpu

f32, i32, u8 = np.float32, np.int32, np.uint8
SENTINEL = CC.SENTINEL


@pytest.fixture(scope="module")
def env():
    import torch
    import orb_slam2_comment_amd as pkg
    E = dict(pkg=pkg, torch=torch, dev=torch.device("cuda:0"), m=pkg.ORBmatcher(0.6, True))
    yield E
    E["m"].close()


def up(E, a):
    a = np.array(a, order="C")                                    # a copy: the shared scenes are read-only
    if a.size == 0:
        a = np.zeros(16, u8)                                      # an empty list still needs an address
    return E["torch"].from_numpy(a).to(E["dev"])


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(u8)


class Call:
    """The tables and the graph state of a scene on the device, with a sentinel-filled report."""

    def __init__(self, E, T, state, upd, id0):
        self.E, self.T, self.id0 = E, T, id0
        self.upd = np.array(upd, i32)
        self.tab = {k: up(E, T[k]) for k in CC.TABLE_KEYS}
        self.state = {k: up(E, state[k]) for k in CC.STATE_KEYS}
        self.d_upd = up(E, self.upd)
        self.d_rep = up(E, np.full((max(len(self.upd), 1), 8), SENTINEL, i32))
        E["torch"].cuda.synchronize()

    def update(self):
        T = self.T
        self.E["m"].UpdateConnectionsDevice(T["rows"], T["cap"], T["np"], T["pcap"], self.tab, self.state, self.id0, len(self.upd),
                                            self.d_upd.data_ptr(), self.d_rep.data_ptr())
        return self

    def results(self):
        self.E["m"].sync()
        got = {k: a.cpu().numpy() for k, a in self.state.items()}
        got["report"] = self.d_rep.cpu().numpy()
        return got


def assert_state_equal(got, out, report, where):
    """All seven arrays whole, as bytes: the rewritten rows are seqref's, and list entries past n_ord, covis of rows whose list
    was not rewritten and every other row hold what the caller passed in."""
    U = len(report)
    assert np.array_equal(got["report"][:U], report), (where, got["report"][:U].tolist(), np.array(report).tolist())
    assert (got["report"][U:] == SENTINEL).all(), where
    for k in ("n_ord", "first_conn", "parent", "conn_w", "ord_kf", "ord_w", "covis"):
        a, b = np.asarray(got[k]).reshape(np.asarray(out[k]).shape), np.asarray(out[k])
        assert np.array_equal(bits(a), bits(b)), (where, k, np.argwhere(a != b)[:6].tolist())


SCENES = [("random", r) for r in (1, 2, 63, 64, 65, 257)] + [("strides", 40)]


@pytest.mark.parametrize("name", SCENES, ids=lambda n: "%s-%d" % n)
def test_update_connections_device_equals_seqref(env, name):
    S = CC.scene_and_reference(name)
    got = Call(env, S["T"], S["state"], S["upd"], S["id0"]).update().results()
    assert_state_equal(got, S["out"], S["report"], name)


@pytest.mark.parametrize("rows", [2, 65])
@pytest.mark.parametrize("upd", [[], [3], [2, 6, 2]], ids=["U0", "U1", "U3"])
def test_update_list_lengths(env, rows, upd):
    S = CC.scene_and_reference(("random", rows))
    upd = [r % rows for r in upd]
    out, rep, touched = CC.run_reference(S["T"], S["state"], upd, S["id0"])
    got = Call(env, S["T"], S["state"], upd, S["id0"]).update().results()
    assert_state_equal(got, out, rep, (rows, upd))
    if not upd:
        assert all(np.array_equal(bits(got[k]), bits(S["state"][k])) for k in CC.STATE_KEYS)      # nothing written


def test_two_calls_on_one_handle(env):
    """A second call continues from the state the first one left (the same as one call with both lists), and a call on
    another scene in between does not leak through the workspace."""
    S, S2 = CC.scene_and_reference(("random", 64)), CC.scene_and_reference(("strides", 40))
    a, b = S["upd"][:3], S["upd"][3:]
    c = Call(env, S["T"], S["state"], a, S["id0"]).update()
    other = Call(env, S2["T"], S2["state"], S2["upd"], S2["id0"]).update()
    first = c.results()
    out1, rep1, _ = CC.run_reference(S["T"], S["state"], a, S["id0"])
    assert_state_equal(first, out1, rep1, "first")
    assert_state_equal(other.results(), S2["out"], S2["report"], "other")
    c2 = Call(env, S["T"], {k: first[k] for k in CC.STATE_KEYS}, b, S["id0"]).update()
    second = c2.results()
    assert_state_equal(second, S["out"], S["report"][3:], "second")


@pytest.mark.parametrize("name", [("random", 65), ("strides", 40), ("random", 1)], ids=lambda n: "%s-%d" % n)
def test_host_entry_equals_the_device_entry(env, name):
    S = CC.scene_and_reference(name)
    state, report = env["m"].UpdateConnections(S["T"], S["state"], S["upd"], S["id0"])
    dev = Call(env, S["T"], S["state"], S["upd"], S["id0"]).update().results()
    host = dict(state, report=report)
    assert_state_equal(host, S["out"], S["report"], "host")
    for k in CC.STATE_KEYS + ("report",):
        assert np.array_equal(bits(host[k]), bits(dev[k])), k
    state, report = env["m"].UpdateConnections(S["T"], S["state"], [], S["id0"])               # U == 0: nothing written
    assert report.shape == (0, 8) and all(np.array_equal(bits(state[k]), bits(S["state"][k])) for k in CC.STATE_KEYS)


def test_host_entry_range_checks_with_a_live_handle(env):
    from orb_slam2_comment_amd import capi
    S = CC.scene_and_reference(("random", 63))
    T, rows = S["T"], 63

    def changed(A, key, index, value):
        B = dict(A)
        B[key] = np.array(A[key]).copy()
        B[key][index] = value
        return B
    r0 = int(S["upd"][0])
    cases = [(changed(T, "obs_kf", 0, rows), S["state"], S["upd"]), (changed(T, "obs_kf", 3, -1), S["state"], S["upd"]),
             (changed(T, "slot_point", (r0, 0), T["np"]), S["state"], S["upd"]), (changed(T, "n", 5, T["cap"] + 1), S["state"], S["upd"]),
             (changed(T, "obs_start", 4, int(T["obs_start"][5]) + 1), S["state"], S["upd"]),
             (T, changed(S["state"], "n_ord", 2, rows + 1), S["upd"]), (T, S["state"], [0, rows]), (T, S["state"], [-1])]
    for Tc, Sc, upd in cases:
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            env["m"].UpdateConnections(Tc, Sc, upd, S["id0"])
        assert ei.value.code == capi.E_ARG
    for dims, code in (((4097, 64), capi.E_CAPACITY), ((63, 4097), capi.E_CAPACITY), ((-1, 64), capi.E_ARG)):
        c = Call(env, T, S["state"], S["upd"], S["id0"])
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            env["m"].UpdateConnectionsDevice(dims[0], dims[1], T["np"], T["pcap"], c.tab, c.state, -1, 1, c.d_upd.data_ptr(),
                                             c.d_rep.data_ptr())
        assert ei.value.code == code
    state, report = env["m"].UpdateConnections(T, S["state"], S["upd"], S["id0"])              # the handle still works
    assert np.array_equal(report, S["report"])


# ---- readers --------------------------------------------------------------------------------------------------------------------
def _updated_graph(name):
    S = CC.scene_and_reference(name)
    rows = S["T"]["rows"]
    bad = np.zeros(rows, u8)
    bad[[r for r in (3, 9) if r < rows]] = 1
    return S, CV.Graph.from_dense(S["out"]), bad


@pytest.mark.parametrize("name", [("random", 2), ("random", 64), ("random", 257), ("strides", 40)], ids=lambda n: "%s-%d" % n)
@pytest.mark.parametrize("nn,nn2", [(10, 0), (3, 0), (10, 5), (20, 5), (12, 70)])
def test_covisible_targets_equal_seqref(env, name, nn, nn2):
    S, G, bad = _updated_graph(name)
    rows = S["T"]["rows"]
    cur = np.array(list(range(min(rows, 24))) + [rows - 1, 0], i32)
    ref = CV.covisible_targets(G, cur, nn, nn2, bad)
    Q, width = len(cur), nn * (1 + nn2)
    d_t, d_c = up(env, np.full((Q + 1, width), SENTINEL, i32)), up(env, np.full(Q + 1, SENTINEL, i32))
    d_ok, d_no, d_bad, d_cur = up(env, S["out"]["ord_kf"]), up(env, S["out"]["n_ord"]), up(env, bad), up(env, cur)
    env["torch"].cuda.synchronize()
    env["m"].CovisibleTargetsDevice(rows, d_ok.data_ptr(), d_no.data_ptr(), d_bad.data_ptr(), Q, d_cur.data_ptr(), nn, nn2,
                                    d_t.data_ptr(), d_c.data_ptr())
    env["m"].sync()
    t, c = d_t.cpu().numpy(), d_c.cpu().numpy()
    assert c[:Q].tolist() == [len(l) for l in ref] and c[Q] == SENTINEL and (t[Q] == SENTINEL).all()
    for q in range(Q):
        assert t[q, :c[q]].tolist() == ref[q] and (t[q, c[q]:] == -1).all(), q
    host = env["m"].CovisibleTargets(S["out"]["ord_kf"], S["out"]["n_ord"], cur, nn, nn2, bad)
    assert [h.tolist() for h in host] == ref
    if nn2 == 0:                                                    # verbatim: without kf_bad the same lists
        assert [h.tolist() for h in env["m"].CovisibleTargets(S["out"]["ord_kf"], S["out"]["n_ord"], cur, nn, 0)] == ref


def test_covisible_targets_edges(env):
    from orb_slam2_comment_amd import capi
    S, G, bad = _updated_graph(("random", 64))
    m = env["m"]
    assert m.CovisibleTargets(S["out"]["ord_kf"], S["out"]["n_ord"], [], 10, 5, bad) == []
    for kw in (dict(cur=[64]), dict(cur=[0], nn=0), dict(cur=[0], nn2=-1)):
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            m.CovisibleTargets(S["out"]["ord_kf"], S["out"]["n_ord"], kw["cur"], kw.get("nn", 10), kw.get("nn2", 5), bad)
        assert ei.value.code == capi.E_ARG


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 257, 600])
def test_children_from_parents(env, rows):
    rng = np.random.default_rng(rows)
    parent = np.where(rng.random(rows) < 0.85, rng.integers(0, max(rows // 3, 1), rows), -1).astype(i32)
    bad = (rng.random(rows) < 0.2).astype(u8)
    for kf_bad in (bad, None):
        start, child = CV.children_from_parents(parent, kf_bad)
        d_s, d_c = up(env, np.full(rows + 2, SENTINEL, i32)), up(env, np.full(rows + 1, SENTINEL, i32))
        d_p, d_b = up(env, parent), up(env, bad)
        env["torch"].cuda.synchronize()
        env["m"].ChildrenFromParentsDevice(rows, d_p.data_ptr(), d_b.data_ptr() if kf_bad is not None else 0, d_s.data_ptr(),
                                           d_c.data_ptr())
        env["m"].sync()
        s, c = d_s.cpu().numpy(), d_c.cpu().numpy()
        assert np.array_equal(s[:rows + 1], start) and s[rows + 1] == SENTINEL
        assert np.array_equal(c[:len(child)], child) and (c[len(child):] == SENTINEL).all()


# ---- chains ---------------------------------------------------------------------------------------------------------------------
def test_chain_into_the_local_map(env):
    """UpdateConnectionsDevice for every row of the local map's scene A, ChildrenFromParentsDevice, then UpdateLocalMapDevice
    reading the covis / parent / child arrays the first two wrote, against seqref.covisibility chained into seqref.localmap."""
    import test_localmap_cpu as LC
    import test_localmap_gpu as LG
    from seqref import localmap as LM
    S, _ = LC.scene_and_reference("A")
    rows, cap, n_pts, pcap = S["rows"], S["cap"], S["np"], S["pcap"]
    upd = list(range(rows))
    T = {k: S[k] for k in CC.TABLE_KEYS}
    T.update(rows=rows, cap=cap, np=n_pts, pcap=pcap)
    state0 = CV.Graph(rows).dense()
    out, rep, touched = CC.run_reference(T, state0, upd, 0)
    start, child = CV.children_from_parents(out["parent"], S["kf_bad"])
    assert (out["n_ord"] >= 5).all() and (out["parent"][1:] >= 0).all() and out["parent"][0] == -1 and len(child) < rows - 1
    S2 = dict(S)
    S2.update(covis=out["covis"], parent=out["parent"], child_start=start, child=child)
    R2 = LM.update_local_map(S2, S["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"], pcap=pcap)
    c = Call(env, T, state0, upd, 0).update()
    d_start, d_child = up(env, np.full(rows + 1, SENTINEL, i32)), up(env, np.full(rows, SENTINEL, i32))
    lm = LG.Call(env, S)
    env["m"].ChildrenFromParentsDevice(rows, c.state["parent"].data_ptr(), lm.tab["kf_bad"].data_ptr(), d_start.data_ptr(),
                                       d_child.data_ptr())
    lm.tab.update(covis=c.state["covis"], parent=c.state["parent"], child_start=d_start, child=d_child)
    got = lm.update().results()
    assert_state_equal(c.results(), out, rep, "chain")
    LG.assert_equal_to_reference(got, S2, R2, LG.DEVICE_TAILS, "chain")
    _, R = LC.scene_and_reference("A")
    assert any(not np.array_equal(R["local_kf"][f], R2["local_kf"][f]) for f in range(S["frames"]))      # the graph is read


def test_chain_into_the_batched_fuse(env):
    """CovisibleTargetsDevice, then FuseDevice with the produced d_targets as d_kf_index: rows equal to FuseDevice called
    with seqref's list."""
    from helpers import synth_frame
    from orb_slam2_comment_amd.matcher import make_camera
    from test_projection_gpu import KITTI_BF, KITTI_CX, KITTI_CY, KITTI_FX, KITTI_FY, _pose, _synthetic_map_for
    t, dev, pkg, m = env["torch"], env["dev"], env["pkg"], env["m"]
    W, H, B = 320, 240, 6
    ext = pkg.ORBextractor(300, 1.2, 8, 20, 7)
    cap = ext.capacity(H, W)
    d_img = t.from_numpy(np.stack([synth_frame(40 + f, W, H) for f in range(B)])).to(dev)
    d_k = t.zeros((B, cap, 7), dtype=t.int32, device=dev)
    d_d = t.zeros((B, cap, 32), dtype=t.uint8, device=dev)
    d_n = t.zeros(B, dtype=t.int32, device=dev)
    t.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    ext.sync()
    n = d_n.cpu().numpy()
    hk = d_k.cpu().numpy().view(u8).reshape(B, cap, 28).view(pkg.KP_DTYPE).reshape(B, cap)
    hd = d_d.cpu().numpy()
    assert (n > 100).all()
    rng = np.random.default_rng(3)
    sf = np.asarray(ext.GetScaleFactors(), f32)
    cam = make_camera(KITTI_FX, KITTI_FY, KITTI_CX, KITTI_CY, (0.0, 0.0, float(W), float(H)), sf, mbf=KITTI_BF, mb=KITTI_BF / KITTI_FX)
    poses = [_pose(rng) for _ in range(B)]
    parts, descs = [], []
    for f in range(B):
        sel = np.sort(rng.choice(int(n[f]), 60, replace=False))
        parts.append(_synthetic_map_for(hk[f, sel], cam, poses[f], rng))
        descs.append(hd[f, sel])
    X, nrm, mx, mn = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    pdesc = np.ascontiguousarray(np.concatenate(descs))
    n_pts = len(X)
    # the graph: row 0 is current; first neighbours 2, 1 (bad), 4; seconds of 2: 4, 0 (current), 5; of 4: 2 (stamped), 5, 3
    G = CC._graph_with_lists(B, {0: [2, 1, 4], 2: [4, 0, 5], 4: [2, 5, 3], 1: [3]})
    bad = np.array([0, 1, 0, 0, 0, 0], u8)
    ref = CV.covisible_targets(G, [0], 10, 5, bad)[0]
    assert ref == [2, 4, 5, 4, 5, 3]
    A = G.dense()
    width = 10 * 6
    d_t, d_c = up(env, np.full((1, width), SENTINEL, i32)), up(env, np.full(1, SENTINEL, i32))
    d_ok, d_no, d_bad, d_cur = up(env, A["ord_kf"]), up(env, A["n_ord"]), up(env, bad), up(env, np.array([0], i32))
    t.cuda.synchronize()
    m.CovisibleTargetsDevice(B, d_ok.data_ptr(), d_no.data_ptr(), d_bad.data_ptr(), 1, d_cur.data_ptr(), 10, 5, d_t.data_ptr(),
                             d_c.data_ptr())
    m.sync()
    K = int(d_c.cpu().numpy()[0])                                   # K is a host integer: four bytes per query come back
    assert K == len(ref)
    d_T = t.from_numpy(np.stack([np.ascontiguousarray(T[:3, :4]).reshape(12) for T in poses])).to(dev)
    pts = [up(env, a) for a in (X, nrm, mx, mn, pdesc)]
    d_fl = up(env, np.ones((K, n_pts), u8))
    inv_sigma2 = (1.0 / (sf * sf)).astype(f32)

    def fuse(d_idx):
        d_Tk = d_T[d_idx[:K].to(t.int64)].contiguous()
        d_bi = t.full((K, n_pts), SENTINEL, dtype=t.int32, device=dev)
        d_bd = t.full((K, n_pts), SENTINEL, dtype=t.int32, device=dev)
        t.cuda.synchronize()
        m.FuseDevice(K, d_idx.data_ptr(), cam, d_Tk.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, n_pts, n_pts,
                     pts[0].data_ptr(), pts[1].data_ptr(), pts[2].data_ptr(), pts[3].data_ptr(), pts[4].data_ptr(), d_fl.data_ptr(),
                     3.0, inv_sigma2, d_bi.data_ptr(), d_bd.data_ptr())
        m.sync()
        return d_bi.cpu().numpy(), d_bd.cpu().numpy()
    bi, bd = fuse(d_t[0])
    bi_ref, bd_ref = fuse(t.tensor(ref, dtype=t.int32, device=dev))
    assert np.array_equal(bi, bi_ref) and np.array_equal(bd, bd_ref)
    assert np.array_equal(bi[1], bi[3]) and not np.array_equal(bi[0], bi[1])     # the repeated target gives the same row twice
    assert ((bd <= 50).sum(1) >= 30).all()
    ext.close()
