"""orbhip_cull_map_points* and orbhip_cull_key_frames* against tests/seqref/culling.py, byte for byte: every in/out and
output array is compared whole, entries behind a count against what the caller passed in.  The scenes of
test_culling_cpu.py (2, 12, 65 and 257 bank rows; a point seen by 70 rows; a culled row with more than 64 connections and
children), candidate lists of 0 and 1 entries, with gaps and with a row twice, recent lists around a wavefront and of 1000
entries with a point twice, two calls on one handle, the host entries, monocular and stereo, and the chains."""
import numpy as np
import pytest

import test_culling_cpu as KC
from seqref import covisibility as CV
from seqref import culling as CU

pytestmark = pytest.mark.gpu

f32, i32, u8 = np.float32, np.int32, np.uint8
SENTINEL = KC.SENTINEL
KF_OUT = ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child", "obs_start_out", "obs_kf_out", "obs_idx_out",
          "ref_obs_out", "conn_w", "ord_kf", "ord_w", "n_ord", "covis", "first_conn", "parent", "report")
MP_OUT = ("slot_point", "flags", "obs_start_out", "obs_kf_out", "obs_idx_out", "ref_obs_out", "recent_out", "n_recent_out", "status")


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
    t = E["torch"]
    if a.dtype.fields is not None:
        a = a.view(u8).reshape(a.shape + (a.dtype.itemsize,))
    return t.from_numpy(a).to(E["dev"])


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(u8)


class Scene:
    """The tables of a scene on the device: fresh in/out copies and sentinel-filled outputs for one call."""

    def __init__(self, E, T, state):
        self.E, self.T = E, T
        host = dict(T, kps=KC.kp_array(T["octave"]))
        self.tab = {k: up(E, host[k]) for k in KC.TABLE_KEYS if host.get(k) is not None}
        self.io = {k: up(E, T[k]) for k in ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child")}
        oc = T["obs_cap"]
        self.io.update(obs_start_out=up(E, np.full(T["np"] + 1, SENTINEL, i32)), obs_kf_out=up(E, np.full(oc, SENTINEL, i32)),
                       obs_idx_out=up(E, np.full(oc, SENTINEL, i32)), ref_obs_out=up(E, np.full(T["np"], SENTINEL, i32)))
        self.state = {k: up(E, state[k]) for k in KC.STATE_KEYS}
        self.extra = {}
        E["torch"].cuda.synchronize()

    def dims(self):
        T = self.T
        return T["rows"], T["cap"], T["np"], T["pcap"], T["obs_cap"]

    def key_frames(self, cand, id0, mono, d_cand=None):
        E, U = self.E, len(cand)
        self.d_cand = up(E, np.array(cand, i32)) if d_cand is None else d_cand
        self.extra["report"] = up(E, np.full((U + 1, 8), SENTINEL, i32))
        E["torch"].cuda.synchronize()
        E["m"].CullKeyFramesDevice(*self.dims(), self.tab, self.io, self.state, id0, U, self.d_cand.data_ptr(), mono, KC.TH_DEPTH,
                                   self.extra["report"].data_ptr())
        return self

    def map_points(self, recent, th_obs, cur_kf_id=100):
        E, T, R = self.E, self.T, len(recent)
        self.d_in = [up(E, a) for a in (np.array(recent, i32), T["found"], T["visible"], T["first_kf_id"])]
        self.extra.update(recent_out=up(E, np.full(R + 1, SENTINEL, i32)), n_recent_out=up(E, np.full(2, SENTINEL, i32)),
                          status=up(E, np.full(R + 1, 77, u8)))
        E["torch"].cuda.synchronize()
        E["m"].CullMapPointsDevice(*self.dims(), self.tab, self.io, R, *[a.data_ptr() for a in self.d_in], cur_kf_id, th_obs,
                                   self.extra["recent_out"].data_ptr(), self.extra["n_recent_out"].data_ptr(),
                                   self.extra["status"].data_ptr())
        return self

    def results(self):
        self.E["m"].sync()
        got = {k: a.cpu().numpy() for d in (self.io, self.state, self.extra) for k, a in d.items()}
        return got


def assert_equal(got, ref, keys, where, tails=True):
    """Whole arrays as bytes.  tails: the device outputs carry one sentinel entry more than the reference's arrays."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if tails and k in ("report", "recent_out", "status", "n_recent_out"):
            fill = 77 if k == "status" else SENTINEL
            assert (a[len(b):] == fill).all(), (where, k)
            a = a[:len(b)]
        a = a.reshape(b.shape)
        assert np.array_equal(bits(a), bits(b.astype(a.dtype))), (where, k, np.argwhere(a != b)[:6].tolist(), a[a != b][:6].tolist(),
                                                                 b[a != b][:6].tolist())


def kf_reference(S, cand, T=None, state=None):
    ref = KC.reference_key_frames(T or S["T"], state or S["state"], cand, S["id0"], S["mono"], KC.TH_DEPTH)
    ref["first_conn"] = (state or S["state"])["first_conn"]
    return ref


@pytest.mark.parametrize("name", list(KC.GPU_SCENES))
def test_cull_key_frames_device_equals_seqref(env, name):
    S = KC.scene_and_reference(name)
    got = Scene(env, S["T"], S["state"]).key_frames(S["cand"], S["id0"], S["mono"]).results()
    assert_equal(got, dict(S["kf"], first_conn=S["state"]["first_conn"]), KF_OUT, name)


@pytest.mark.parametrize("name", ["r2", "r65"])
@pytest.mark.parametrize("cand", [[], [6], [-1, -1]], ids=["U0", "U1", "gaps"])
def test_candidate_list_lengths(env, name, cand):
    S = KC.scene_and_reference(name)
    cand = [r % S["T"]["rows"] if r >= 0 else r for r in cand]
    got = Scene(env, S["T"], S["state"]).key_frames(cand, S["id0"], S["mono"]).results()
    assert_equal(got, kf_reference(S, cand), KF_OUT, (name, cand))


@pytest.mark.parametrize("name", list(KC.GPU_SCENES))
@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 1000])
def test_cull_map_points_device_equals_seqref(env, name, R):
    S = KC.scene_and_reference(name)
    m = S["mp"][R]
    got = Scene(env, S["T"], S["state"]).map_points(m["recent"], S["th_obs"]).results()
    assert_equal(got, m["out"], MP_OUT, (name, R))
    for k in ("kf_bad", "child", "conn_w", "parent"):               # not this call's business
        assert np.array_equal(bits(got[k]), bits(np.asarray(S["T"].get(k, S["state"].get(k))))), k


def test_two_calls_on_one_handle(env):
    """The second call continues from what the first one left, with the table out swapped in, and equals one call with both
    lists; a call on another scene in between does not leak through the workspace."""
    S, S2 = KC.scene_and_reference("r65"), KC.scene_and_reference("r12")
    a, b = S["cand"][:4], S["cand"][4:]
    c = Scene(env, S["T"], S["state"]).key_frames(a, S["id0"], S["mono"])
    other = Scene(env, S2["T"], S2["state"]).map_points(S2["mp"][65]["recent"], S2["th_obs"])
    first = c.results()
    assert_equal(first, kf_reference(S, a), KF_OUT, "first")
    assert_equal(other.results(), S2["mp"][65]["out"], MP_OUT, "other")
    T1 = dict(S["T"])
    total = int(first["obs_start_out"][-1])
    T1.update({k: first[k] for k in ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child")},
              obs_start=first["obs_start_out"], obs_kf=first["obs_kf_out"], obs_idx=first["obs_idx_out"], ref_obs=first["ref_obs_out"])
    T1["obs_kf"], T1["obs_idx"] = T1["obs_kf"].copy(), T1["obs_idx"].copy()
    T1["obs_kf"][total:], T1["obs_idx"][total:] = 0, 0
    state1 = {k: first[k] for k in KC.STATE_KEYS}
    second = Scene(env, T1, state1).key_frames(b, S["id0"], S["mono"]).results()
    whole = dict(S["kf"], first_conn=S["state"]["first_conn"])
    for k in ("obs_kf_out", "obs_idx_out"):                         # behind the count: this call's sentinels
        n2 = int(whole["obs_start_out"][-1])
        assert np.array_equal(second[k][:n2], whole[k][:n2]) and (second[k][n2:] == SENTINEL).all()
    nc = int(whole["child_start"][-1])                              # behind the count: what the first call left there
    assert np.array_equal(second["child"][:nc], whole["child"][:nc]) and np.array_equal(second["child"][nc:], first["child"][nc:])
    assert_equal(second, dict(whole, report=S["kf"]["report"][4:]), [k for k in KF_OUT if k not in ("obs_kf_out", "obs_idx_out", "child")],
                 "second")


@pytest.mark.parametrize("name", ["r12", "r65"])
def test_host_entries_equal_the_device_entries(env, name):
    S = KC.scene_and_reference(name)
    T = dict(S["T"], kps=KC.kp_array(S["T"]["octave"]))
    cand = list(dict.fromkeys(S["cand"].tolist()))                  # the host form wants a row at most once; one gap stays
    io, state, report = env["m"].CullKeyFrames(T, T, S["state"], cand, S["id0"], S["mono"], KC.TH_DEPTH, fill=SENTINEL)
    ref = kf_reference(S, cand)
    assert_equal(dict(io, **state, report=report), ref, KF_OUT, "host", tails=False)
    dev = Scene(env, S["T"], S["state"]).key_frames(cand, S["id0"], S["mono"]).results()
    assert_equal(dev, ref, KF_OUT, "device")
    m = S["mp"][1000]
    io, kept, status = env["m"].CullMapPoints(T, T, m["recent"], T["found"], T["visible"], T["first_kf_id"], 100, S["th_obs"],
                                              fill=SENTINEL)
    out = m["out"]
    assert_equal(io, out, MP_OUT[:6], "host map points", tails=False)
    assert np.array_equal(status, out["status"]) and np.array_equal(kept, out["recent_out"][:int(out["n_recent_out"][0])])
    io, kept, status = env["m"].CullMapPoints(T, T, [], T["found"], T["visible"], T["first_kf_id"], 100, S["th_obs"], fill=SENTINEL)
    assert_equal(io, S["mp"][0]["out"], MP_OUT[:6], "host R == 0", tails=False)      # the table is still copied through
    assert len(kept) == 0 and len(status) == 0


def test_host_entry_range_checks_with_a_live_handle(env):
    from orb_slam2_comment_amd import capi
    S = KC.scene_and_reference("r12")
    T = dict(S["T"], kps=KC.kp_array(S["T"]["octave"]))
    rows = T["rows"]

    def changed(A, key, index, value):
        B = dict(A)
        B[key] = np.array(A[key]).copy()
        B[key][index] = value
        return B
    o1 = int(T["obs_start"][1])
    assert o1 >= 2
    cases = [(changed(T, "obs_kf", 0, rows), S["state"], [3]), (changed(T, "obs_idx", 1, T["cap"]), S["state"], [3]),
             (changed(T, "obs_kf", 1, int(T["obs_kf"][0])), S["state"], [3]),                  # a row twice in a list
             (changed(T, "slot_point", (3, 0), T["np"]), S["state"], [3]), (changed(T, "n", 5, T["cap"] + 1), S["state"], [3]),
             (T, changed(S["state"], "n_ord", 2, rows + 1), [3]), (T, changed(S["state"], "parent", 2, rows), [3]),
             (T, S["state"], [0, rows]), (T, S["state"], [-2]), (T, S["state"], [3, 4, 3])]
    for Tc, Sc, cand in cases:
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            env["m"].CullKeyFrames(Tc, Tc, Sc, cand, S["id0"], S["mono"], KC.TH_DEPTH)
        assert ei.value.code == capi.E_ARG
    for rec in ([T["np"]], [-1]):
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            env["m"].CullMapPoints(T, T, rec, T["found"], T["visible"], T["first_kf_id"], 100, 3)
        assert ei.value.code == capi.E_ARG
    c = Scene(env, S["T"], S["state"])
    d = up(env, np.zeros(16, i32))
    for dims, code in (((4097, 64), capi.E_CAPACITY), ((12, 4097), capi.E_CAPACITY), ((-1, 64), capi.E_ARG)):
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            env["m"].CullKeyFramesDevice(dims[0], dims[1], T["np"], T["pcap"], T["obs_cap"], c.tab, c.io, c.state, -1, 1, d.data_ptr(),
                                         False, KC.TH_DEPTH, d.data_ptr())
        assert ei.value.code == code
    with pytest.raises(env["pkg"].OrbHipError) as ei:                # the table out must not be the table in
        env["m"].CullKeyFramesDevice(*c.dims(), c.tab, dict(c.io, obs_kf_out=c.tab["obs_kf"]), c.state, -1, 1, d.data_ptr(), False,
                                     KC.TH_DEPTH, d.data_ptr())
    assert ei.value.code == capi.E_ARG
    io, state, report = env["m"].CullKeyFrames(T, T, S["state"], [3], S["id0"], S["mono"], KC.TH_DEPTH)      # the handle still works
    assert np.array_equal(report, kf_reference(S, [3])["report"])


def test_monocular_and_stereo_differ(env):
    """The same scene with and without u_right / depth: different counts, different verdicts, both equal to seqref."""
    S = KC.scene_and_reference("r65")                               # the monocular scene
    assert S["mono"] and S["T"]["u_right"] is None
    T2, state2 = KC.cull_scene(65, 5, True)
    ref2 = KC.reference_key_frames(T2, state2, S["cand"], S["id0"], False, KC.TH_DEPTH)
    ref2["first_conn"] = state2["first_conn"]
    got2 = Scene(env, T2, state2).key_frames(S["cand"], S["id0"], False).results()
    assert_equal(got2, ref2, KF_OUT, "stereo")
    assert not np.array_equal(ref2["report"], S["kf"]["report"])


# ---- chains ---------------------------------------------------------------------------------------------------------------------
def test_chain_from_covisible_targets(env):
    """CovisibleTargetsDevice(nn, 0) of the current row, its output passed straight in as d_cand with U = nn: the -1 entries
    behind the count are skipped, and the list is read before the call re-sorts the row it came from."""
    S = KC.scene_and_reference("r65")
    rows, cur, nn = 65, 2, 30
    G = CV.Graph.from_dense(S["state"])
    cand = CV.best_covisibility_keyframes(G, cur, nn)
    assert 3 < len(cand) < nn
    padded = cand + [-1] * (nn - len(cand))
    ref = kf_reference(S, padded)
    assert (ref["report"][:, 0] == CU.CULLED).sum() > 1 and (ref["report"][:, 0] == CU.SKIPPED_ENTRY).sum() == nn - len(cand)
    assert ref["n_ord"][cur] < S["state"]["n_ord"][cur]             # the current row was re-sorted by the call
    c = Scene(env, S["T"], S["state"])
    d_t, d_c, d_cur = up(env, np.full(nn, SENTINEL, i32)), up(env, np.full(1, SENTINEL, i32)), up(env, np.array([cur], i32))
    env["torch"].cuda.synchronize()
    env["m"].CovisibleTargetsDevice(rows, c.state["ord_kf"].data_ptr(), c.state["n_ord"].data_ptr(), 0, 1, d_cur.data_ptr(), nn, 0,
                                    d_t.data_ptr(), d_c.data_ptr())
    got = c.key_frames(padded, S["id0"], S["mono"], d_cand=d_t).results()
    assert_equal(got, ref, KF_OUT, "targets chain")
    # the head of the row's own list, which the call re-sorts, as the candidate list: the call works on its copy
    c = Scene(env, S["T"], S["state"])
    U = len(cand)
    got = c.key_frames(cand, S["id0"], S["mono"], d_cand=c.state["ord_kf"][cur]).results()
    assert_equal(got, kf_reference(S, cand), KF_OUT, "own list as candidates")


def test_chain_into_update_connections(env):
    """Both culling calls, the table out swapped in after each, then UpdateConnectionsDevice and ChildrenFromParents on what
    they left, against the seqref chain."""
    import test_covisibility_cpu as CC
    S = KC.scene_and_reference("r65")
    T, state = S["T"], S["state"]
    rec = S["mp"][1000]["recent"]
    mp = S["mp"][1000]["out"]
    total = int(mp["obs_start_out"][-1])
    T1 = dict(T, slot_point=mp["slot_point"], flags=mp["flags"], obs_start=mp["obs_start_out"], ref_obs=mp["ref_obs_out"],
              obs_kf=np.where(np.arange(T["obs_cap"]) < total, mp["obs_kf_out"], 0).astype(i32),
              obs_idx=np.where(np.arange(T["obs_cap"]) < total, mp["obs_idx_out"], 0).astype(i32))
    kf = KC.reference_key_frames(T1, state, S["cand"], S["id0"], S["mono"], KC.TH_DEPTH)
    upd = [2, 0, 7, 1]
    T2 = dict(slot_point=kf["slot_point"], n=T["n"], obs_start=kf["obs_start_out"], obs_kf=kf["obs_kf_out"], flags=kf["flags"])
    state2 = {k: kf[k] for k in KC.STATE_KEYS if k != "first_conn"}
    state2["first_conn"] = state["first_conn"]
    out, rep, _ = CC.run_reference(T2, state2, upd, S["id0"])
    # the device: one set of buffers, the table swapped by exchanging the records' pointers
    c = Scene(env, T, state).map_points(rec, S["th_obs"])
    for a, b in (("obs_start", "obs_start_out"), ("obs_kf", "obs_kf_out"), ("obs_idx", "obs_idx_out"), ("ref_obs", "ref_obs_out")):
        c.tab[a], c.io[b] = c.io[b], c.tab[a]
    c.key_frames(S["cand"], S["id0"], S["mono"])
    for a, b in (("obs_start", "obs_start_out"), ("obs_kf", "obs_kf_out"), ("obs_idx", "obs_idx_out"), ("ref_obs", "ref_obs_out")):
        c.tab[a], c.io[b] = c.io[b], c.tab[a]
    d_upd, d_rep = up(env, np.array(upd, i32)), up(env, np.full((len(upd), 8), SENTINEL, i32))
    env["torch"].cuda.synchronize()
    tab = dict(slot_point=c.io["slot_point"], n=c.tab["n"], obs_start=c.tab["obs_start"], obs_kf=c.tab["obs_kf"], flags=c.io["flags"])
    env["m"].UpdateConnectionsDevice(T["rows"], T["cap"], T["np"], T["pcap"], tab, c.state, S["id0"], len(upd), d_upd.data_ptr(),
                                     d_rep.data_ptr())
    got = c.results()
    assert np.array_equal(d_rep.cpu().numpy(), rep)
    for k in KC.STATE_KEYS:
        assert np.array_equal(bits(got[k].reshape(np.asarray(out[k]).shape)), bits(out[k])), k
    n2 = int(kf["obs_start_out"][-1])
    assert np.array_equal(c.tab["obs_start"].cpu().numpy(), kf["obs_start_out"])
    assert np.array_equal(c.tab["obs_kf"].cpu().numpy()[:n2], kf["obs_kf_out"][:n2])
    assert np.array_equal(got["report"][:len(S["cand"])], kf["report"])
    assert not np.array_equal(kf["report"], S["kf"]["report"])      # the points the first call culled changed the verdicts


def _local_map_scene():
    """Scene A of the local map (12 rows of 256 slots, 400 points, two current frames) with what culling reads on top:
    key-point indices for the observations, a bank of key points, poses and descriptors, the graph UpdateConnections gives.
    Rows 5 and 8 see their points at a coarse octave and keep only points that five rows and more observe, so both are
    culled."""
    import test_covisibility_cpu as CC
    import test_localmap_cpu as LC
    import test_seqref_projection_cpu as PC
    S = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in LC.scene_and_reference("A")[0].items()}
    rows, cap, n_pts, pcap = S["rows"], S["cap"], S["np"], S["pcap"]
    rng = np.random.default_rng(77)
    lists = [[int(k) for k in S["obs_kf"][S["obs_start"][p]:S["obs_start"][p + 1]]] for p in range(n_pts)]
    for p in range(n_pts):
        if len(lists[p]) < 5:
            for r in (5, 8):
                if r in lists[p]:
                    lists[p].remove(r)
                    S["slot_point"][r][S["slot_point"][r] == p] = -1
    S["obs_start"] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(i32)
    S["obs_kf"] = np.array([k for x in lists for k in x] + [0, 0], i32)
    S["obs_idx"] = np.array([int(np.nonzero(S["slot_point"][k] == p)[0][0]) for p, x in enumerate(lists) for k in x] + [0, 0], i32)
    S["obs_cap"] = len(S["obs_kf"])
    S["ref_obs"] = np.array([int(rng.integers(0, len(x))) if x else -1 for x in lists], i32)
    S["octave"] = rng.integers(0, 3, (rows, cap)).astype(i32)
    S["octave"][[5, 8]] = 6
    S["depth"], S["u_right"], S["not_erase"] = np.zeros((rows, cap), f32), None, np.zeros(rows, u8)
    S["to_be_erased"] = np.zeros(rows, u8)
    S["child"] = np.concatenate([S["child"], np.full(rows, SENTINEL, i32)])[:rows].astype(i32)
    bank = np.zeros((rows, cap), KC.kp_array(S["octave"]).dtype)
    bank["x"], bank["y"] = rng.uniform(0, PC.W, (rows, cap)), rng.uniform(0, PC.H, (rows, cap))
    bank["octave"] = S["octave"]
    S["bank_keys"], S["bank_desc"] = bank, rng.integers(0, 256, (rows, cap, 32), dtype=u8)
    S["bank_T"] = [PC.pose(rng, small=False) for _ in range(rows)]
    T = {k: S[k] for k in CC.TABLE_KEYS}
    T.update(rows=rows, cap=cap, np=n_pts, pcap=pcap)
    state, _, _ = CC.run_reference(T, CV.Graph(rows).dense(), list(range(rows)), 0)
    return S, state


def test_chain_into_the_local_map_and_the_map_point_refresh(env):
    """CullKeyFramesDevice, the table out swapped in, then UpdateLocalMapDevice (slot_point, kf_bad, covis, parent, child,
    the table, flags as the call left them) and UpdateMapPointsDevice (the table with obs_idx and ref_obs, kf_bad, flags)
    on the same buffers, against seqref.culling chained into seqref.localmap and seqref.mappoint."""
    import test_localmap_cpu as LC
    import test_localmap_gpu as LG
    import test_mappoint_cpu as MC
    import test_mappoint_gpu as MG
    from seqref import localmap as LM
    from seqref import mappoint as MP
    S, state = _local_map_scene()
    rows, cap, n_pts, pcap = S["rows"], S["cap"], S["np"], S["pcap"]
    cand = [5, 1, 8, 2]
    kf = KC.reference_key_frames(S, state, cand, 0, True, KC.TH_DEPTH)
    assert kf["report"][:, 0].tolist() == [CU.CULLED, CU.NOT_CULLED, CU.CULLED, CU.NOT_CULLED] and kf["report"][:, 3].sum() > 100
    n_left = int(kf["obs_start_out"][-1])
    S2 = dict(S, slot_point=kf["slot_point"], kf_bad=kf["kf_bad"], covis=kf["covis"], parent=kf["parent"], flags=kf["flags"],
              child_start=kf["child_start"], child=kf["child"][:int(kf["child_start"][-1])], obs_start=kf["obs_start_out"],
              obs_kf=kf["obs_kf_out"][:n_left])
    R2 = LM.update_local_map(S2, S["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"], pcap=pcap)
    _, R = LC.scene_and_reference("A")
    assert any(not np.array_equal(R["local_kf"][f], R2["local_kf"][f]) for f in range(S["frames"]))      # the culled rows are gone
    keys = [S["bank_keys"][r] for r in range(rows)]
    desc = [S["bank_desc"][r] for r in range(rows)]
    pd, nrm, mx, mn = MC.sentinels(n_pts)
    ref_mp = MP.update_map_points(S["scam"], MC.BOTH, S["bank_T"], keys, desc, kf["kf_bad"], kf["obs_start_out"], kf["obs_kf_out"],
                                  kf["obs_idx_out"], kf["ref_obs_out"], S["world"], kf["flags"], pd, nrm, mx, mn)
    assert (ref_mp[5] == MP.UPDATED).sum() > 100 and n_left < S["obs_start"][-1] - 100
    # the device chain on one set of buffers
    c = Scene(env, S, state).key_frames(cand, 0, True)
    lm = LG.Call(env, S)
    lm.tab.update(slot_point=c.io["slot_point"], kf_bad=c.io["kf_bad"], covis=c.state["covis"], parent=c.state["parent"],
                  child_start=c.io["child_start"], child=c.io["child"], obs_start=c.io["obs_start_out"], obs_kf=c.io["obs_kf_out"],
                  flags=c.io["flags"])
    got_lm = lm.update().results()
    bank = MG.upload_bank(env, keys, desc, S["bank_T"], None, cap)
    t = env["torch"]
    out = [up(env, a) for a in MC.sentinels(pcap)]
    best = t.full((pcap,), MG.PATTERN, dtype=t.int32, device=env["dev"])
    status = t.full((pcap,), MG.STATUS_FILL, dtype=t.uint8, device=env["dev"])
    d_world = up(env, S["world"])
    t.cuda.synchronize()
    env["m"].UpdateMapPointsDevice(S["cam"], MC.BOTH, bank["T"].data_ptr(), bank["k"].data_ptr(), bank["d"].data_ptr(),
                                   bank["n"].data_ptr(), cap, n_pts, pcap, c.io["obs_start_out"].data_ptr(),
                                   c.io["obs_kf_out"].data_ptr(), c.io["obs_idx_out"].data_ptr(), c.io["ref_obs_out"].data_ptr(),
                                   d_world.data_ptr(), c.io["flags"].data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                   out[2].data_ptr(), out[3].data_ptr(), status.data_ptr(), d_best_obs=best.data_ptr(),
                                   d_kf_bad=c.io["kf_bad"].data_ptr())
    got = c.results()
    ref = dict(kf, first_conn=state["first_conn"])
    assert_equal(got, ref, KF_OUT, "chain")
    LG.assert_equal_to_reference(got_lm, S2, R2, LG.DEVICE_TAILS, "chain")
    MG.assert_equal_to_reference([a.cpu().numpy() for a in out] + [best.cpu().numpy(), status.cpu().numpy()], ref_mp, MC.BOTH, n_pts,
                                 "chain")
