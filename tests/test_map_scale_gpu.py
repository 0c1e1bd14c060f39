"""The covisibility, local-map and culling entries at the bank sizes the product runs them at, byte for byte against
tests/seqref on sentinel-filled outputs (the protocol, the Call classes and the assert_* helpers are those of
test_covisibility_gpu.py, test_localmap_gpu.py and test_culling_gpu.py; the scenes and their preconditions are in
map_scale_cases.py).  Every test first checks on the reference alone that its case reaches the path it is named for.

Covisibility (UpdateConnectionsDevice, UpdateConnections)
  cv_blocks2     cap 256: two workgroups of k_cv_counters add to the same counter rows
  cv_blocks8     1100 rows, cap 2048: eight workgroups (the clamp), rows with more than 1024 filled slots, voters all over the
                 bank; maxima tied across wavefronts (the lower row in the higher one), across passes of a thread and lanes of a
                 wavefront, and in the fallback; the sort at N = 2048; 555 and 585 qualifying rows; the host entry with 72 resident rows
  cv_wide        one row with 319 qualifying rows: the store loop of the own row and the re-sort count past 256
  cv_full4096    4096 rows: the LDS arrays full, a list of 4095 entries with 4089 ties re-sorted, row 4095 voter and updated
Readers
  CovisibleTargetsDevice on the graphs of cv_blocks8 and cv_full4096: copies of 100 and 4095 entries, second neighbours read
  70 and 300 deep from lists of 555 to 601 entries; ChildrenFromParentsDevice at 4096 rows with one parent's 719 children in
  sixteen passes, and at 1025 rows with one parent for all
Local map (UpdateLocalMapDevice, UpdateLocalMap, TrackLocalMapDevice)
  lm_rows1100    1070 listed rows: the second grid pass of k_lm_first / k_lm_points, carries in k_lm_keyframes and k_lm_scan;
                 rows of 300 and 600 slots with winners and losers in every pass; the reference row tied across passes of its
                 thread, lanes of its wavefront and wavefronts;
                 lists of 17 and 33 votes; a walk past 64 unacceptable children, and past 130
  lm_cap4096     cap 4096, a listed row with every slot taken, a frame of 4096 key points
  lm_rows65536   65536 rows: the last word of the stamp bitset
Culling (CullKeyFramesDevice, CullMapPointsDevice and the host entries)
  cu_rows1100    cap 1536: verdicts over 1300 slots, six erasing workgroups, the re-sort at N = 2048, adoption above row 1024
  cu_full4096    4096 rows: a neighbour's list of 4095 entries re-sorted, children and parent candidates in the last bitset word
cv_blocks8, lm_rows1100 and cu_rows1100 run once more on the same handle after FillScratch(0xA5)."""
import numpy as np
import pytest

import map_scale_cases as C
import test_covisibility_cpu as CC
import test_covisibility_gpu as CG
import test_culling_cpu as KC
import test_culling_gpu as KG
import test_localmap_cpu as LC
import test_localmap_gpu as LG
import test_seqref_projection_cpu as PC
from seqref import covisibility as CV

pytestmark = pytest.mark.gpu

i32, u8 = np.int32, np.uint8
SENTINEL = C.SENTINEL
bits = CG.bits


@pytest.fixture(scope="module")
def env():
    import torch
    import orb_slam2_comment_amd as pkg
    E = dict(pkg=pkg, torch=torch, dev=torch.device("cuda:0"), m=pkg.ORBmatcher(LC.NNRATIO, True))
    yield E
    E["m"].close()


# ---- covisibility ---------------------------------------------------------------------------------------------------------------
def _update(env, S):
    return CG.Call(env, S["T"], S["state"], S["upd"], S["id0"]).update().results()


@pytest.mark.parametrize("name", ["cv_blocks2", "cv_blocks8", "cv_wide", "cv_full4096"])
def test_update_connections_device_equals_seqref(env, name):
    C.preconditions(name)
    S = C.cv_case(name)
    CG.assert_state_equal(_update(env, S), S["out"], S["report"], name)


@pytest.mark.parametrize("name", ["cv_blocks2", "cv_blocks8_host", "cv_wide"])
def test_update_connections_host_entry_equals_seqref_and_the_device_entry(env, name):
    C.preconditions(name.replace("_host", ""))
    S = C.cv_case(name)
    state, report = env["m"].UpdateConnections(S["T"], S["state"], S["upd"], S["id0"])
    host = dict(state, report=report)
    CG.assert_state_equal(host, S["out"], S["report"], "host " + name)
    dev = _update(env, S)
    for k in CC.STATE_KEYS + ("report",):
        assert np.array_equal(bits(host[k]), bits(dev[k])), k


def _graph_on_device(env, case):
    key = ("graph", case)
    if key not in env:
        out = C.cv_case(case)["out"]
        env[key] = (CG.up(env, out["ord_kf"]), CG.up(env, out["n_ord"]), CG.up(env, C.target_bad(case)))
    return env[key]


@pytest.mark.parametrize("case,nn,nn2", C.TARGET_CASES, ids=lambda v: str(v))
def test_covisible_targets_equal_seqref(env, case, nn, nn2):
    C.preconditions(case)
    C.target_preconditions(case, nn, nn2)
    ref = C.target_reference(case, nn, nn2)[0]
    S, cur, bad = C.cv_case(case), C.target_rows(case), C.target_bad(case)
    rows, Q, width = S["T"]["rows"], len(cur), nn * (1 + nn2)
    d_ok, d_no, d_bad = _graph_on_device(env, case)
    d_t, d_c, d_cur = CG.up(env, np.full((Q + 1, width), SENTINEL, i32)), CG.up(env, np.full(Q + 1, SENTINEL, i32)), CG.up(env, cur)
    env["torch"].cuda.synchronize()
    env["m"].CovisibleTargetsDevice(rows, d_ok.data_ptr(), d_no.data_ptr(), d_bad.data_ptr(), Q, d_cur.data_ptr(), nn, nn2,
                                    d_t.data_ptr(), d_c.data_ptr())
    env["m"].sync()
    t, c = d_t.cpu().numpy(), d_c.cpu().numpy()
    assert c[:Q].tolist() == [len(l) for l in ref] and c[Q] == SENTINEL and (t[Q] == SENTINEL).all()
    for q in range(Q):
        assert t[q, :c[q]].tolist() == ref[q] and (t[q, c[q]:] == -1).all(), q
    if not (case == "cv_full4096" and nn == 4096):                  # that one would stage every row of the bank
        host = env["m"].CovisibleTargets(S["out"]["ord_kf"], S["out"]["n_ord"], cur, nn, nn2, bad)
        assert [h.tolist() for h in host] == ref


@pytest.mark.parametrize("name", ["rows4096", "rows1025"])
def test_children_from_parents(env, name):
    C.preconditions("children")
    K = C.children_case(name)
    rows = K["rows"]
    for kf_bad, (start, child) in ((K["bad"], (K["start"], K["child"])), (None, CV.children_from_parents(K["parent"], None))):
        d_s, d_c = CG.up(env, np.full(rows + 2, SENTINEL, i32)), CG.up(env, np.full(rows + 1, SENTINEL, i32))
        d_p, d_b = CG.up(env, K["parent"]), CG.up(env, K["bad"])
        env["torch"].cuda.synchronize()
        env["m"].ChildrenFromParentsDevice(rows, d_p.data_ptr(), d_b.data_ptr() if kf_bad is not None else 0, d_s.data_ptr(),
                                           d_c.data_ptr())
        env["m"].sync()
        s, c = d_s.cpu().numpy(), d_c.cpu().numpy()
        assert np.array_equal(s[:rows + 1], start) and s[rows + 1] == SENTINEL
        assert np.array_equal(c[:len(child)], child) and (c[len(child):] == SENTINEL).all()


# ---- local map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lm_rows1100", "lm_cap4096", "lm_rows65536"])
def test_update_local_map_device_equals_seqref(env, name):
    C.preconditions(name)
    S, R = C.lm_case(name)
    got = LG.Call(env, S).update().results()
    LG.assert_equal_to_reference(got, S, R, LG.DEVICE_TAILS, "device " + name)


def test_update_local_map_host_entry_equals_seqref_and_the_device_entry(env):
    C.preconditions("lm_rows1100")
    S, R = C.lm_case("lm_rows1100")
    got = LG.host_call(env, S)
    LG.assert_equal_to_reference(got, S, R, {k: LG.HOST_FILL for k in LG.DEVICE_TAILS}, "host", lk_in=np.array(S["local_kf"]))
    dev = LG.Call(env, S).update().results()
    for f in range(S["frames"]):
        npt = int(dev["np_l"][f])
        for k in ("local_point", "world_l", "normal_l", "max_dist_l", "min_dist_l", "desc_l", "flags_l"):
            assert np.array_equal(bits(got[k][f, :npt]), bits(dev[k][f, :npt])), k
    assert np.array_equal(got["report"], dev["report"]) and np.array_equal(got["votes"], dev["votes"])


def test_track_local_map_equals_the_three_entries(env):
    """The chained call on lm_rows1100 against UpdateLocalMapDevice, FrustumQueriesDevice and SearchByProjectionPointsDevice
    called one after the other, and its local map against seqref."""
    C.preconditions("lm_rows1100")
    S0, R = C.lm_case("lm_rows1100")
    S = C.lm_add_track_arrays(S0)
    m = env["m"]
    one, tr1 = LG.Call(env, S), LG.track_arrays(env, S)
    m.TrackLocalMapDevice(*one.dims(), one.tab, one.io, S["cam"], tr1, LC.VIEW_COS, LC.TH, LC.NNRATIO)
    three, tr3 = LG.Call(env, S).update(), LG.track_arrays(env, S)
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
    LG.assert_equal_to_reference(g3, S, R, LG.DEVICE_TAILS, "three entries")
    for f in range(S["frames"]):                                    # the chained call applied the assignment to the frame
        nf, a = int(S["frame_n"][f]), t1["assign"][f]
        want = np.where(a[:nf] >= 0, g1["local_point"][f][np.maximum(a[:nf], 0)], R["frame_point"][f, :nf])
        assert np.array_equal(g1["frame_point"][f, :nf], want), f


# ---- culling --------------------------------------------------------------------------------------------------------------------
def _kf_ref(S):
    return dict(S["kf"], first_conn=S["state"]["first_conn"])


@pytest.mark.parametrize("name", ["cu_rows1100", "cu_full4096"])
def test_cull_key_frames_device_equals_seqref(env, name):
    C.preconditions(name)
    S = C.cu_case(name)
    got = KG.Scene(env, S["T"], S["state"]).key_frames(S["cand"], S["id0"], S["mono"]).results()
    KG.assert_equal(got, _kf_ref(S), KG.KF_OUT, name)


def test_cull_map_points_device_equals_seqref(env):
    C.preconditions("cu_rows1100")
    S = C.cu_case("cu_rows1100")
    mp = S["mp"][C.CU_RECENT]
    got = KG.Scene(env, S["T"], S["state"]).map_points(mp["recent"], S["th_obs"]).results()
    KG.assert_equal(got, mp["out"], KG.MP_OUT, "cu_rows1100")
    for k in ("kf_bad", "child", "conn_w", "parent"):               # not this call's business
        assert np.array_equal(bits(got[k]), bits(np.asarray(S["T"].get(k, S["state"].get(k))))), k


def test_cull_host_entries_equal_seqref(env):
    C.preconditions("cu_rows1100")
    S = C.cu_case("cu_rows1100")
    T = dict(S["T"], kps=KC.kp_array(S["T"]["octave"]))
    cand = S["cand"].tolist()
    assert len(set(cand)) == len(cand)                              # the host form wants a row at most once
    io, state, report = env["m"].CullKeyFrames(T, T, S["state"], cand, S["id0"], S["mono"], KC.TH_DEPTH, fill=SENTINEL)
    KG.assert_equal(dict(io, **state, report=report), _kf_ref(S), KG.KF_OUT, "host", tails=False)
    mp = S["mp"][C.CU_RECENT]
    io, kept, status = env["m"].CullMapPoints(T, T, mp["recent"], T["found"], T["visible"], T["first_kf_id"], 100, S["th_obs"],
                                              fill=SENTINEL)
    out = mp["out"]
    KG.assert_equal(io, out, KG.MP_OUT[:6], "host map points", tails=False)
    assert np.array_equal(status, out["status"]) and np.array_equal(kept, out["recent_out"][:int(out["n_recent_out"][0])])


# ---- once more on a poisoned workspace --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cv_blocks8", "lm_rows1100", "cu_rows1100"])
def test_second_run_after_the_scratch_is_filled_with_a5(env, name):
    """The scratch-poison protocol at these sizes: the case grows the handle's slots, FillScratch(0xA5) fills them (integers
    large and negative), and the same case on the same handle still equals the reference."""
    C.preconditions(name)

    def run():
        if name == "cv_blocks8":
            S = C.cv_case(name)
            CG.assert_state_equal(_update(env, S), S["out"], S["report"], name)
        elif name == "lm_rows1100":
            S, R = C.lm_case(name)
            LG.assert_equal_to_reference(LG.Call(env, S).update().results(), S, R, LG.DEVICE_TAILS, name)
        else:
            S = C.cu_case(name)
            got = KG.Scene(env, S["T"], S["state"]).key_frames(S["cand"], S["id0"], S["mono"]).results()
            KG.assert_equal(got, _kf_ref(S), KG.KF_OUT, name)
            mp = S["mp"][C.CU_RECENT]
            got = KG.Scene(env, S["T"], S["state"]).map_points(mp["recent"], S["th_obs"]).results()
            KG.assert_equal(got, mp["out"], KG.MP_OUT, name)
    run()
    assert env["m"].FillScratch(0xA5) > 0
    run()
