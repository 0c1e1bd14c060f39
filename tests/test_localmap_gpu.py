"""orbhip_update_local_map_device / orbhip_update_local_map / orbhip_track_local_map_device (Tracking::UpdateLocalKeyFrames,
UpdateLocalPoints and SearchLocalPoints over tables) against tests/seqref/localmap.py, byte for byte: the three scenes of
test_localmap_cpu.py (every status and every way the walk ends), two calls on one handle, the host entry and its range
checks, the chained call against the three separate entries and against the seqref chain, and the edge shapes."""
import numpy as np
import pytest

import test_localmap_cpu as LC
import test_seqref_projection_cpu as PC
from seqref import localmap as LM

pytestmark = pytest.mark.gpu

f32, i32, u8 = np.float32, np.int32, np.uint8
SENTINEL = LC.SENTINEL
FPAT = np.array([SENTINEL], i32).view(f32)[0]
DEVICE_TAILS = dict(local_kf=SENTINEL, votes=None, local_point=SENTINEL, world_l=FPAT, normal_l=FPAT, max_dist_l=FPAT,
                    min_dist_l=FPAT, desc_l=0xA5, flags_l=0xA5, taken=0xA5)
HOST_FILL = 77


@pytest.fixture(scope="module")
def env():
    import torch
    import orb_slam2_comment_amd as pkg
    E = dict(pkg=pkg, torch=torch, dev=torch.device("cuda:0"), m=pkg.ORBmatcher(LC.NNRATIO, True))
    yield E
    E["m"].close()


def up(E, a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(u8).reshape(a.shape + (a.dtype.itemsize,))
    if a.size == 0:
        a = np.zeros(16, u8)                                      # an empty list still needs an address
    return E["torch"].from_numpy(a).to(E["dev"])


def previous_lists(S):
    """The scene's previous local key-frame lists with the sentinel behind their counts."""
    lk = np.array(S["local_kf"], i32)
    for f in range(S["frames"]):
        lk[f, int(S["n_local_kf"][f]):] = SENTINEL
    return lk


class Call:
    """The tables of a scene and sentinel-filled outputs on the device."""

    def __init__(self, E, S, frames=None, kf_bad=True):
        self.E, self.S = E, S
        self.frames = S["frames"] if frames is None else frames
        self.tab = {k: up(E, S[k]) for k in LC.TABLE_KEYS if k != "kf_bad"}
        if kf_bad:
            self.tab["kf_bad"] = up(E, S["kf_bad"])
        io = LC.sentinel_io(S["frames"], S["rows"], S["cap"], S["pcap"], S["frame_point"], S["frame_n"], previous_lists(S),
                            S["n_local_kf"])
        self.io = {k: up(E, a) for k, a in io.items()}
        E["torch"].cuda.synchronize()

    def dims(self):
        S = self.S
        return self.frames, S["rows"], S["cap"], S["np"], S["pcap"]

    def update(self):
        self.E["m"].UpdateLocalMapDevice(*self.dims(), self.tab, self.io)
        return self

    def results(self):
        self.E["m"].sync()
        return {k: a.cpu().numpy() for k, a in self.io.items()}


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(u8)


def assert_equal_to_reference(got, S, R, tails, where, frames=None, lk_in=None):
    """Every output against seqref's as bytes; behind the counts the arrays hold `tails` (the sentinels of a device call,
    the fill of the host mirror), and frames that were not asked for are untouched."""
    frames = S["frames"] if frames is None else frames
    lk_in = previous_lists(S) if lk_in is None else lk_in
    rep = np.array(R["report"][:frames])
    assert np.array_equal(got["report"][:frames], rep), (where, got["report"][:frames].tolist(), rep.tolist())
    assert np.array_equal(got["frame_point"][:frames], R["frame_point"][:frames]), where
    assert np.array_equal(got["votes"][:frames], R["votes"][:frames]), where
    assert np.array_equal(got["n_local_kf"][:frames], rep[:, 2]) and np.array_equal(got["np_l"][:frames], rep[:, 6]), where
    for f in range(frames):
        nk, npt, nf = int(rep[f, 2]), int(rep[f, 6]), int(S["frame_n"][f])
        assert np.array_equal(got["local_kf"][f, :nk], R["local_kf"][f]), (where, f)
        assert np.array_equal(got["local_kf"][f, nk:], lk_in[f, nk:]), (where, f)              # in/out: the caller's bytes
        pts = R["local_point"][f]
        assert np.array_equal(got["local_point"][f, :npt], pts), (where, f, np.nonzero(got["local_point"][f, :npt] != pts)[0][:8])
        w, nrm, mx, mn, d = LM.gather(S, pts)
        for k, ref in (("world_l", w), ("normal_l", nrm), ("max_dist_l", mx), ("min_dist_l", mn), ("desc_l", d),
                       ("flags_l", R["flags_l"][f])):
            assert np.array_equal(bits(got[k][f, :npt]), bits(ref)), (where, f, k)
        assert np.array_equal(got["taken"][f, :nf], R["taken"][f, :nf]), (where, f)
        for k, n in (("local_point", npt), ("world_l", npt), ("normal_l", npt), ("max_dist_l", npt), ("min_dist_l", npt),
                     ("desc_l", npt), ("flags_l", npt), ("taken", nf)):
            tail = got[k][f, n:]
            assert np.array_equal(bits(tail), bits(np.full(tail.shape, tails[k], tail.dtype))), (where, f, k)


def assert_untouched(got, S, frames_from):
    io = LC.sentinel_io(S["frames"], S["rows"], S["cap"], S["pcap"], S["frame_point"], S["frame_n"], previous_lists(S), S["n_local_kf"])
    for k, a in io.items():
        assert np.array_equal(bits(got[k][frames_from:]), bits(a[frames_from:])), k


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_update_local_map_device_equals_seqref(env, name):
    S, R = LC.scene_and_reference(name)
    got = Call(env, S).update().results()
    assert_equal_to_reference(got, S, R, DEVICE_TAILS, "device " + name)


def test_two_calls_on_one_handle_are_independent(env):
    """Scene B, then scene A with fewer frames, then scene B again on the same handle: the workspace (first-occurrence keys,
    frame-held marks) of a call does not leak into the next, and a call writes only the frames it was asked for."""
    SB, RB = LC.scene_and_reference("B")
    SA, RA = LC.scene_and_reference("A")
    b1, a, b2 = Call(env, SB), Call(env, SA, frames=1), Call(env, SB)
    b1.update()
    a.update()
    b2.update()
    ga = a.results()
    assert_equal_to_reference(b1.results(), SB, RB, DEVICE_TAILS, "first B")
    assert_equal_to_reference(ga, SA, RA, DEVICE_TAILS, "A after B", frames=1)
    assert_untouched(ga, SA, 1)
    assert_equal_to_reference(b2.results(), SB, RB, DEVICE_TAILS, "B after A")
    # a second call on its own outputs: the lists are in/out, the rest is rebuilt from them
    S, R = LC.scene_and_reference("C")
    c = Call(env, S).update()
    first = c.results()
    c.update()
    again = c.results()
    assert_equal_to_reference(first, S, R, DEVICE_TAILS, "C")
    lk = np.array(first["local_kf"])
    R2 = LM.update_local_map(S, first["frame_point"], S["frame_n"], lk, first["n_local_kf"], pcap=S["pcap"])
    assert_equal_to_reference(again, S, R2, DEVICE_TAILS, "C again", lk_in=lk)


def test_without_kf_bad_no_row_is_bad(env):
    S, _ = LC.scene_and_reference("C")
    S2 = dict(S)
    S2["kf_bad"] = None
    R = LM.update_local_map(S2, S["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"], pcap=S["pcap"])
    assert LC.report(R, 2)["status"] == LM.OK
    got = Call(env, S, kf_bad=False).update().results()
    assert_equal_to_reference(got, S2, R, DEVICE_TAILS, "no kf_bad")


# ---- host entry ---------------------------------------------------------------------------------------------------------------
def host_call(env, S, **changes):
    T = {k: S[k] for k in LC.TABLE_KEYS}
    T.update(changes)
    return env["m"].UpdateLocalMap(T, changes.get("frame_point", S["frame_point"]), S["frame_n"],
                                   changes.get("local_kf", S["local_kf"]), S["n_local_kf"], fill=HOST_FILL)


@pytest.mark.parametrize("name", ["A", "C"])
def test_host_entry_equals_the_device_entry(env, name):
    S, R = LC.scene_and_reference(name)
    got = host_call(env, S)
    tails = {k: HOST_FILL for k in DEVICE_TAILS}
    assert_equal_to_reference(got, S, R, tails, "host " + name, lk_in=np.array(S["local_kf"]))
    dev = Call(env, S).update().results()
    for f in range(S["frames"]):
        npt = int(dev["np_l"][f])
        for k in ("local_point", "world_l", "normal_l", "max_dist_l", "min_dist_l", "desc_l", "flags_l"):
            assert np.array_equal(bits(got[k][f, :npt]), bits(dev[k][f, :npt])), k
    assert np.array_equal(got["report"], dev["report"]) and np.array_equal(got["votes"], dev["votes"])


def test_host_entry_range_checks(env):
    from orb_slam2_comment_amd import capi
    S, _ = LC.scene_and_reference("C")

    def changed(key, index, value):
        a = np.array(S[key]).copy()
        a[index] = value
        return {key: a}
    nobs, nchild = int(S["obs_start"][-1]), int(S["child_start"][-1])
    cases = [changed("obs_kf", nobs - 1, S["rows"]), changed("obs_kf", 0, -1), changed("slot_point", (1, 0), S["np"]),
             changed("slot_point", (2, 1), -2), changed("obs_start", 5, int(S["obs_start"][6]) + 1),
             changed("child_start", 2, int(S["child_start"][3]) + 1), changed("child", nchild - 1, S["rows"]),
             changed("parent", 4, S["rows"]), changed("covis", (1, 0), S["rows"]), changed("n", 3, S["cap"] + 1),
             changed("frame_point", (0, 0), S["np"]), changed("local_kf", (1, 0), S["rows"])]
    for case in cases:
        with pytest.raises(env["pkg"].OrbHipError) as ei:
            host_call(env, S, **case)
        assert ei.value.code == capi.E_ARG, list(case)
    assert np.array_equal(host_call(env, S)["report"], LC.scene_and_reference("C")[1]["report"])      # the handle still works


# ---- the chained call ---------------------------------------------------------------------------------------------------------
def track_arrays(E, S):
    frames, cap, pcap = S["frames"], S["cap"], S["pcap"]
    return dict(Tcw=up(E, np.stack([np.asarray(t, f32)[:3].reshape(12) for t in S["T"]])), kps=up(E, S["keys"]), desc=up(E, S["desc"]),
                q=up(E, np.full((frames, pcap, 40), 0xA5, u8)), assign=up(E, np.full((frames, cap), SENTINEL, i32)),
                nmatches=up(E, np.full(frames, SENTINEL, i32)))


def test_track_local_map_equals_the_three_entries_and_the_seqref_chain(env):
    S, R = LC.scene_and_reference("A")
    m = env["m"]
    one, tr1 = Call(env, S), track_arrays(env, S)
    m.TrackLocalMapDevice(*one.dims(), one.tab, one.io, S["cam"], tr1, LC.VIEW_COS, LC.TH, LC.NNRATIO)
    three, tr3 = Call(env, S).update(), track_arrays(env, S)
    io = three.io
    m.FrustumQueriesDevice(S["frames"], S["cam"], tr3["Tcw"].data_ptr(), S["pcap"], io["np_l"].data_ptr(), io["world_l"].data_ptr(),
                           io["normal_l"].data_ptr(), io["max_dist_l"].data_ptr(), io["min_dist_l"].data_ptr(),
                           io["flags_l"].data_ptr(), LC.VIEW_COS, LC.TH, tr3["q"].data_ptr())
    m.SearchByProjectionPointsDevice(S["frames"], tr3["kps"].data_ptr(), tr3["desc"].data_ptr(), io["frame_n"].data_ptr(), S["cap"],
                                     PC.BOUNDS, tr3["q"].data_ptr(), io["desc_l"].data_ptr(), io["np_l"].data_ptr(), S["pcap"],
                                     tr3["assign"].data_ptr(), tr3["nmatches"].data_ptr(), d_taken=io["taken"].data_ptr())
    g1, g3 = one.results(), three.results()
    t1, t3 = ({k: a.cpu().numpy() for k, a in t.items()} for t in (tr1, tr3))
    for k in ("q", "assign", "nmatches"):
        assert np.array_equal(t1[k], t3[k]), k
    for k in g1:
        if k not in ("frame_point", "report"):
            assert np.array_equal(bits(g1[k]), bits(g3[k])), k
    assert np.array_equal(g1["report"][:, :7], g3["report"][:, :7])
    # the seqref chain: update, frustum, search, assignment
    ref = LC.track_reference()
    Rt = dict(R)
    Rt["report"], Rt["frame_point"] = np.array(R["report"]), np.array(R["frame_point"])
    for f, (q, assign, nm, fp) in enumerate(ref):
        nf, npt = int(S["frame_n"][f]), len(q)
        got_q = t1["q"][f, :npt].copy().view(q.dtype).reshape(npt)
        valid = q["valid"] != 0
        assert np.array_equal(got_q["valid"] != 0, valid)
        assert np.array_equal(got_q[valid].tobytes(), q[valid].tobytes())
        assert (t1["q"][f, npt:] == 0xA5).all()
        assert np.array_equal(t1["assign"][f, :nf], assign) and t1["nmatches"][f] == nm
        Rt["frame_point"][f, :nf] = fp
        Rt["report"][f, 7] = valid.sum()
        assert (fp != R["frame_point"][f, :nf]).sum() > 30          # key points that had no point got one
    assert_equal_to_reference(g1, S, Rt, DEVICE_TAILS, "track")


# ---- edge shapes ----------------------------------------------------------------------------------------------------------------
def test_edge_shapes(env):
    from orb_slam2_comment_amd import capi
    m, pkg = env["m"], env["pkg"]
    S, R = LC.scene_and_reference("C")                              # its frame 1 lists a row with n = 0
    assert S["n"][17] == 0 and 17 in R["local_kf"][1]
    c = Call(env, S, frames=0).update()                             # frames 0: success, nothing written
    assert_untouched(c.results(), S, 0)
    # a frame with n 0 (no votes: the list stays), np 0 (no point is local) and both
    S0 = dict(S)
    S0["frame_n"] = np.array([20, 0, 12], i32)
    R0 = LM.update_local_map(S0, S["frame_point"], S0["frame_n"], S["local_kf"], S["n_local_kf"], pcap=S["pcap"])
    assert LC.report(R0, 1)["status"] == LM.NO_VOTES and np.array_equal(R0["frame_point"][1], S["frame_point"][1])
    assert_equal_to_reference(Call(env, S0).update().results(), S0, R0, DEVICE_TAILS, "frame n 0")
    S1 = dict(S)
    S1.update(np=0, slot_point=np.full_like(S["slot_point"], -1), frame_point=np.full_like(S["frame_point"], -1),
              obs_start=np.zeros(1, i32))
    R1 = LM.update_local_map(S1, S1["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"], pcap=S["pcap"])
    assert [LC.report(R1, f)["n_local_points"] for f in range(3)] == [0, 0, 0]
    assert_equal_to_reference(Call(env, S1).update().results(), S1, R1, DEVICE_TAILS, "np 0")
    # limits and counts, refused before any device work
    c = Call(env, S)
    for dims, code in (((3, S["rows"], 4097, S["np"], S["pcap"]), capi.E_CAPACITY), ((3, 65537, S["cap"], S["np"], S["pcap"]), capi.E_CAPACITY),
                       ((-1, S["rows"], S["cap"], S["np"], S["pcap"]), capi.E_ARG), ((3, S["rows"], S["cap"], -1, S["pcap"]), capi.E_ARG),
                       ((3, S["rows"], S["cap"], S["pcap"] + 1, S["pcap"]), capi.E_ARG), ((3, -1, S["cap"], S["np"], S["pcap"]), capi.E_ARG)):
        with pytest.raises(pkg.OrbHipError) as ei:
            m.UpdateLocalMapDevice(*dims, c.tab, c.io)
        assert ei.value.code == code, dims
    for key, rec in (("slot_point", "tab"), ("flags", "tab"), ("report", "io"), ("frame_point", "io")):
        d = dict(getattr(c, rec))
        d[key] = 0                                                  # a null required pointer
        with pytest.raises(pkg.OrbHipError) as ei:
            m.UpdateLocalMapDevice(*c.dims(), d if rec == "tab" else c.tab, d if rec == "io" else c.io)
        assert ei.value.code == capi.E_ARG, key
    assert_untouched(c.results(), S, 0)
