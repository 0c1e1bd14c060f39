"""The projection prologues, Fuse and SearchBySim3 on the device against tests/seqref/projection.py: the scenes and the
hand-worked edges of test_seqref_projection_cpu.py through the public entry points, bit for bit against the literal layer
and under that module's measured bounds against the fp64 layer; then the device-resident forms
at the sizes where one-thread-per-point kernels, the record packing of k_fuse_batch and the output strides can go wrong."""
import numpy as np
import pytest

import test_seqref_projection_cpu as C
from seqref import matcher as SM
from seqref import projection as P

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [1, 63, 64, 65, 255, 256, 257, 700]
PATTERN = -0x5A5A5A5B


class DeviceAsOracle:
    """The package's host entry points behind the oracle's Python interface, so that every scene and every hand-worked
    edge of the CPU module runs unchanged against the kernels.  Anything else (the extractor) is the oracle's."""

    def __init__(self, pkg, oracle):
        self.pkg, self.oracle = pkg, oracle
        self.m = pkg.ORBmatcher(0.6, True)

    def __getattr__(self, name):
        return getattr(self.oracle, name)

    def make_frame(self, keys, desc, u_right, bounds, scale_factors, keep):
        return self.pkg.FrameView(keys, desc, scale_factors, bounds, u_right)

    def project_last_frame(self, *a):
        return self.m.ProjectLastFrame(*a)

    def frustum_queries(self, *a):
        return self.m.FrustumQueries(*a)

    def keyframe_queries(self, *a):
        return self.m.KeyFrameQueries(*a)

    def search_best_in_window(self, kf, q, qd, inv_sigma2=None):
        return self.m.SearchBestInWindow(kf, q, qd, inv_sigma2)

    def search_by_sim3(self, *a):
        return self.m.SearchBySim3(*a)


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    import orb_slam2_comment_amd as pkg
    C.key_frames(oracle)
    return dict(pkg=pkg, torch=torch, dev=torch.device("cuda:0"), O=oracle, G=DeviceAsOracle(pkg, oracle))


# ---- the CPU module's scenes and edges, the kernels in the oracle's place ------------------------------------------------

@pytest.mark.parametrize("motion", ["forward", "backward", "neither"])
@pytest.mark.parametrize("mono,th", [(False, 7.0), (True, 15.0)])
def test_project_last_frame_equals_literal(env, motion, mono, th):
    C.test_project_last_frame_oracle_equals_literal(env["G"], motion, mono, th)


@pytest.mark.parametrize("th,seed", [(1.0, 1), (3.0, 2)])
def test_frustum_queries_equal_literal(env, th, seed):
    C.test_frustum_queries_oracle_equals_literal(env["G"], th, seed)


@pytest.mark.parametrize("double_invz,th,seed", [(False, 3.0, 4), (True, 4.0, 5)])
def test_keyframe_queries_equal_literal(env, double_invz, th, seed):
    C.test_keyframe_queries_mode0_oracle_equals_literal(env["G"], double_invz, th, seed)


@pytest.mark.parametrize("sim3_form,th", [(False, 3.0), (True, 4.0)])
def test_prologue_and_best_in_window_equal_literal(env, sim3_form, th):
    C.test_fuse_oracle_equals_literal(env["G"], sim3_form, th)


@pytest.mark.parametrize("s12,seed", [(0.8, 11), (1.05, 12), (1.3, 13)])
def test_search_by_sim3_equals_literal(env, s12, seed):
    """matches12 and nFound against seqref, which composes sR12, sR21 and t21 itself; the floor (n > 100) is asserted on
    seqref's own count."""
    C.test_search_by_sim3_oracle_equals_literal(env["G"], s12, seed)


@pytest.mark.parametrize("edge", [C.test_edge_image_bounds_inclusive_for_frame_exclusive_for_keyframe,
                                  C.test_edge_depth_zero_negative_nan_and_inf, C.test_edge_scale_invariance_range,
                                  C.test_edge_viewing_cosine_limit_radius_switch_and_normal_gate,
                                  C.test_edge_predict_scale_integers_and_clamp, C.test_edge_forward_backward_on_mb,
                                  C.test_edge_octave_outside_the_table, C.test_edge_sim3_composition_by_hand,
                                  C.test_edge_best_in_window], ids=lambda f: f.__name__[10:])
def test_hand_worked_edges(env, edge):
    edge(env["G"])


# ---- sizes around the block and the wavefront, host forms ---------------------------------------------------------------

def _tile(a, n):
    return np.concatenate([a] * (n // len(a) + 1))[:n]


@pytest.fixture(scope="module")
def big(env):
    """700 points per prologue and their literal records, computed once; a prefix of the input gives a prefix of the
    records (one thread, one point)."""
    cam, scam = C.make_cam()
    S = C.last_frame_scene(env["O"], "forward")
    L = {k: _tile(S[k], 700) for k in ("X", "flags", "keys")}
    L.update(Tcw=S["Tcw"], Tlw=S["Tlw"])
    L["q"] = P.project_last_frame(scam, L["Tcw"], L["Tlw"], L["X"], L["flags"], L["keys"], 7.0, False)
    Fm = C.map_scene(21, 700)
    Fm["q"], Fm["vc"] = P.frustum_queries(scam, Fm["T"], Fm["X"], Fm["nrm"], Fm["max_d"], Fm["min_d"], Fm["flags"], 0.5, 3.0)
    Fm["kq"] = P.keyframe_queries(scam, 0, False, Fm["T"], None, Fm["X"], Fm["nrm"], Fm["max_d"], Fm["min_d"], Fm["flags"], 3.0)
    assert 100 < L["q"]["valid"].sum() < 700 and 30 < Fm["q"]["valid"].sum() < 700 and 30 < Fm["kq"]["valid"].sum() < 700
    return cam, scam, L, Fm


@pytest.mark.parametrize("n", SIZES)
def test_host_forms_at_block_and_wavefront_sizes(env, big, n):
    cam, scam, L, Fm = big
    m = env["G"].m
    q = m.ProjectLastFrame(cam, L["Tcw"], L["Tlw"], L["X"][:n], L["flags"][:n], L["keys"][:n], 7.0, False)
    C.assert_queries_equal(q, L["q"][:n], "last")
    q, vc = m.FrustumQueries(cam, Fm["T"], Fm["X"][:n], Fm["nrm"][:n], Fm["max_d"][:n], Fm["min_d"][:n], Fm["flags"][:n], 0.5, 3.0)
    C.assert_queries_equal(q, Fm["q"][:n], "frustum")
    assert np.array_equal(vc.view(np.int32), Fm["vc"][:n].view(np.int32))
    q = m.KeyFrameQueries(cam, 0, False, Fm["T"], None, Fm["X"][:n], Fm["nrm"][:n], Fm["max_d"][:n], Fm["min_d"][:n],
                          Fm["flags"][:n], 3.0)
    C.assert_queries_equal(q, Fm["kq"][:n], "keyframe")


# ---- device-resident forms -------------------------------------------------------------------------------------------

def _up(env, a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return env["torch"].from_numpy(a).to(env["dev"])


def _queries(env, t, shape):
    return t.cpu().numpy().view(np.uint8).reshape(shape + (40,)).copy().view(env["pkg"].QUERY_DTYPE).reshape(shape)


def _frame_rows(env, rows, cap):
    """Key points and descriptors of the given (keys, desc) per frame row in the extractor's output layout."""
    B = len(rows)
    k = np.zeros((B, cap), env["pkg"].KP_DTYPE)
    d = np.zeros((B, cap, 32), np.uint8)
    n = np.zeros(B, np.int32)
    for r, kd in enumerate(rows):
        if kd is not None:
            n[r] = len(kd[0])
            k[r, :n[r]], d[r, :n[r]] = kd
    return k, d, n


def test_project_and_track_last_frame_device(env):
    """8 (current, last) pairs at rows (2, 1), (4, 3), ... of 17 (last_first = 1, last_step = 2), the last frames holding
    n = 1, 63, 64, 65, 255, 256, 257 and 700 points under a cap above every n, general Tlw and Tcw going forward, backward
    and neither in turn: ProjectLastFrameDevice against the literal prologue, records past n untouched, nq == n;
    TrackLastFrameDevice (the same projection body inside k_grid_build_project) against the literal prologue followed by
    seqref's SearchByProjection."""
    t, pkg = env["torch"], env["pkg"]
    cam, scam = C.make_cam()
    (ka, da), (kb, db) = C.key_frames(env["O"])
    cap, pairs = 768, len(SIZES)
    base = [C.last_frame_scene(env["O"], mo) for mo in ("forward", "backward", "neither")]
    scenes = [base[p % 3] for p in range(pairs)]
    last = [(_tile(ka, n), _tile(da, n)) for n in SIZES]
    cur = [(kb, db) if p % 2 == 0 else (kb[:300], db[:300]) for p in range(pairs)]
    rows = [None]
    for p in range(pairs):
        rows += [last[p], cur[p]]
    k, d, n = _frame_rows(env, rows, cap)
    assert cap > n.max()
    world, flags = np.zeros((len(rows), cap, 3), f32), np.zeros((len(rows), cap), np.uint8)
    for p, S in enumerate(scenes):
        world[1 + 2 * p, :SIZES[p]] = _tile(S["X"], SIZES[p])
        flags[1 + 2 * p, :SIZES[p]] = _tile(S["flags"], SIZES[p])
    d_k, d_d, d_n, d_w, d_f = _up(env, k), _up(env, d), _up(env, n), _up(env, world), _up(env, flags)
    d_Tcw = _up(env, np.stack([S["Tcw"][:3].reshape(12) for S in scenes]))
    d_Tlw = _up(env, np.stack([S["Tlw"][:3].reshape(12) for S in scenes]))
    d_q = t.full((pairs, cap, 10), PATTERN, dtype=t.int32, device=env["dev"])
    d_nq = t.full((pairs,), PATTERN, dtype=t.int32, device=env["dev"])
    d_assign = t.full((pairs, cap), PATTERN, dtype=t.int32, device=env["dev"])
    d_nm = t.full((pairs,), PATTERN, dtype=t.int32, device=env["dev"])
    m = pkg.ORBmatcher(0.9, True)
    for mono, th in ((False, 7.0), (True, 15.0)):
        d_q.fill_(PATTERN)
        m.ProjectLastFrameDevice(pairs, cam, d_Tcw.data_ptr(), d_Tlw.data_ptr(), d_k.data_ptr(), d_n.data_ptr(), cap, 1, 2,
                                 d_w.data_ptr(), d_f.data_ptr(), th, mono, d_q.data_ptr(), d_nq.data_ptr())
        m.TrackLastFrameDevice(pairs, cam, d_Tcw.data_ptr(), d_Tlw.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(),
                               cap, 2, 2, 1, 2, d_w.data_ptr(), d_f.data_ptr(), th, mono, d_assign.data_ptr(), d_nm.data_ptr())
        m.sync()
        q = _queries(env, d_q, (pairs, cap))
        raw = d_q.cpu().numpy()
        assign, nm = d_assign.cpu().numpy(), d_nm.cpu().numpy()
        assert d_nq.cpu().numpy().tolist() == SIZES
        total = 0
        for p, S in enumerate(scenes):
            nl = SIZES[p]
            want = P.project_last_frame(scam, S["Tcw"], S["Tlw"], world[1 + 2 * p, :nl], flags[1 + 2 * p, :nl], last[p][0], th, mono)
            C.assert_queries_equal(q[p, :nl], want, "pair %d" % p)
            assert (raw[p, nl:] == PATTERN).all(), p
            F = SM.Frame(cur[p][0], cur[p][1], None, C.BOUNDS, C.SF)
            sn, sassign = SM.search_by_projection_frame(F, want, last[p][1], None, True)
            assert nm[p] == sn and np.array_equal(assign[p, :len(cur[p][0])], sassign), p
            total += sn
        assert total > 100                                 # seqref's own count: the search is not vacuous
    m.close()


def test_frustum_queries_device(env):
    """2 frames, np = (300, 129), pcap = 300: records and view_cos against the literal layer, entries past np untouched."""
    t, pkg = env["torch"], env["pkg"]
    cam, scam = C.make_cam()
    pcap, npts = 300, [300, 129]
    S = [C.map_scene(31, pcap), C.map_scene(32, pcap)]
    st = lambda key: _up(env, np.stack([s[key] for s in S]))  # noqa: E731
    d_T = _up(env, np.stack([s["T"][:3].reshape(12) for s in S]))
    keep = [st("X"), st("nrm"), st("max_d"), st("min_d"), st("flags"), _up(env, np.array(npts, np.int32))]
    d_q = t.full((2, pcap, 10), PATTERN, dtype=t.int32, device=env["dev"])
    d_vc = t.full((2, pcap), -7.0, dtype=t.float32, device=env["dev"])
    m = pkg.ORBmatcher(0.8, True)
    m.FrustumQueriesDevice(2, cam, d_T.data_ptr(), pcap, keep[5].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(),
                           keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), 0.5, 3.0, d_q.data_ptr(), d_vc.data_ptr())
    m.sync()
    q, raw, vc = _queries(env, d_q, (2, pcap)), d_q.cpu().numpy(), d_vc.cpu().numpy()
    for f, s in enumerate(S):
        k = npts[f]
        want, wvc = P.frustum_queries(scam, s["T"], s["X"][:k], s["nrm"][:k], s["max_d"][:k], s["min_d"][:k], s["flags"][:k], 0.5, 3.0)
        C.assert_queries_equal(q[f, :k], want, "frame %d" % f)
        assert np.array_equal(vc[f, :k].view(np.int32), wvc.view(np.int32))
        assert (raw[f, k:] == PATTERN).all() and (vc[f, k:] == -7.0).all()
        assert want["valid"].sum() > 5
    m.close()


WAVE_COUNTS = ([0, 1, 8, 9, 1], [64, 64, 64, 64, 1], [63, 64, 9, 8, 0])     # valid records per wavefront of 257 points, per row


@pytest.fixture(scope="module")
def fuse_case(env):
    """257 map points that pass every gate of key frame `a`, and flag rows that leave exactly 0, 1, 8, 9, 63 and 64 valid
    records in single wavefronts (the packing and the 8-lanes-per-query groups of k_fuse_batch)."""
    cam, scam = C.make_cam()
    S = C.fuse_scene(env["O"], 7)
    ones = np.ones(len(S["X"]), np.uint8)
    allq = P.keyframe_queries(scam, 0, False, S["T"], None, S["X"], S["nrm"], S["max_d"], S["min_d"], ones, 3.0)
    sel = np.nonzero(allq["valid"] == 1)[0][:257]
    assert len(sel) == 257
    fc = {k: np.ascontiguousarray(S[k][sel]) for k in ("X", "nrm", "max_d", "min_d", "pdesc")}
    flags = np.zeros((3, 257), np.uint8)
    rng = np.random.default_rng(3)
    for r, counts in enumerate(WAVE_COUNTS):
        for w, c in enumerate(counts):
            lanes = np.sort(rng.choice(min(64, 257 - 64 * w), c, replace=False))
            flags[r, 64 * w + lanes] = 1
    fc.update(cam=cam, scam=scam, flags=flags, T=S["T"], keys=S["keys"], desc=S["desc"], ur=S["ur"], sig=C.INV_SIGMA2)
    return fc


def _expected_rows(fc, u_right, sim3_form, th):
    """Per target (key frame, the empty frame, the key frame again): seqref's `fuse` and its records, one key frame at a
    time."""
    F = SM.Frame(fc["keys"], fc["desc"], fc["ur"] if u_right else None, C.BOUNDS, C.SF)
    n = len(fc["X"])
    rows = []
    for r in range(3):
        args = (fc["T"], fc["X"], fc["nrm"], fc["max_d"], fc["min_d"], fc["flags"][r])
        q = P.keyframe_queries(fc["scam"], 0, sim3_form, args[0], None, *args[1:], th)
        if r == 1:                                         # the empty key frame
            rows.append((np.full(n, -1, np.int32), np.full(n, 256, np.int32), q))
        else:
            rows.append(P.fuse(F, fc["scam"], *args, fc["pdesc"], th, fc["sig"], sim3_form) + (q,))
    return rows


def _fuse_through_every_entry(env, fc, u_right, sim3_form, th, rows):
    """K = 3 targets (the key frame, an empty frame, the key frame again with other flags), pcap = np + 33: Fuse, FuseBatch
    and FuseDevice with the caller's grids and with grids built inside the call, each row against `rows`; outputs past np
    untouched.  Returns [(entry, row, best_idx, best_dist)] for further assertions."""
    t, pkg, cam = env["torch"], env["pkg"], fc["cam"]
    m = env["G"].m
    n = len(fc["X"])
    got = []
    va = pkg.FrameView(fc["keys"], fc["desc"], C.SF, C.BOUNDS, fc["ur"] if u_right else None)
    v0 = pkg.FrameView(fc["keys"][:0], fc["desc"][:0], C.SF, C.BOUNDS, None)
    args = (fc["X"], fc["nrm"], fc["max_d"], fc["min_d"])
    for r in (0, 2):
        bi, bd = m.Fuse(va, cam, fc["T"], *args, fc["flags"][r], fc["pdesc"], th, fc["sig"], sim3_form)
        got.append(("Fuse", r, bi, bd))
    bi, bd = m.FuseBatch([va, v0, va], cam, [fc["T"]] * 3, *args, fc["flags"], fc["pdesc"], th, fc["sig"], sim3_form)
    got += [("FuseBatch", r, bi[r], bd[r]) for r in range(3)]
    # device-resident: frame rows (the key frame, another one, empty), targets (0, 2, 0)
    cap, pcap = 512, n + 33
    kb, db = C.key_frames(env["O"])[1]
    k, d, nk = _frame_rows(env, [(fc["keys"], fc["desc"]), (kb, db), None], cap)
    assert cap > nk.max()
    ur = np.full((3, cap), -1, f32)
    ur[0, :len(fc["keys"])] = fc["ur"]
    d_k, d_d, d_n, d_ur = _up(env, k), _up(env, d), _up(env, nk), _up(env, ur)
    pad = lambda a, fill: _up(env, np.concatenate([a, np.full((pcap - n,) + a.shape[1:], fill, a.dtype)]))  # noqa: E731
    dX, dN, dMx, dMn, dP = pad(fc["X"], 1e9), pad(fc["nrm"], 1e9), pad(fc["max_d"], 1e9), pad(fc["min_d"], 1e9), pad(fc["pdesc"], 0xAA)
    fl = np.ones((3, pcap), np.uint8)
    fl[:, :n] = fc["flags"]
    d_fl, d_idx = _up(env, fl), _up(env, np.array([0, 2, 0], np.int32))
    d_T = _up(env, np.stack([np.asarray(fc["T"], f32)[:3].reshape(12)] * 3))
    d_cell = t.full((3, cap), -9, dtype=t.int32, device=env["dev"])
    d_items = t.full((3, cap), -9, dtype=t.int32, device=env["dev"])
    d_start = t.full((3, 64 * 48 + 1), -9, dtype=t.int32, device=env["dev"])
    m.AssignFeaturesToGridDevice(3, d_k.data_ptr(), d_n.data_ptr(), cap, C.BOUNDS, d_cell.data_ptr(), d_start.data_ptr(),
                                 d_items.data_ptr())
    for csr in (False, True):
        d_bi = t.full((3, pcap), PATTERN, dtype=t.int32, device=env["dev"])
        d_bd = t.full((3, pcap), PATTERN, dtype=t.int32, device=env["dev"])
        d_q = t.full((3, pcap, 10), PATTERN, dtype=t.int32, device=env["dev"])
        m.FuseDevice(3, d_idx.data_ptr(), cam, d_T.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, n, pcap,
                     dX.data_ptr(), dN.data_ptr(), dMx.data_ptr(), dMn.data_ptr(), dP.data_ptr(), d_fl.data_ptr(), th,
                     fc["sig"], d_bi.data_ptr(), d_bd.data_ptr(), sim3_form=sim3_form,
                     d_u_right=d_ur.data_ptr() if u_right else 0, d_cell_start=d_start.data_ptr() if csr else 0,
                     d_cell_items=d_items.data_ptr() if csr else 0, d_q=d_q.data_ptr())
        m.sync()
        bi, bd, raw = d_bi.cpu().numpy(), d_bd.cpu().numpy(), d_q.cpu().numpy()
        q = _queries(env, d_q, (3, pcap))
        for r in range(3):
            C.assert_queries_equal(q[r, :n], rows[r][2], "row %d" % r)
            got.append(("FuseDevice/%s grid" % ("caller's" if csr else "own"), r, bi[r, :n], bd[r, :n]))
        assert (bi[:, n:] == PATTERN).all() and (bd[:, n:] == PATTERN).all() and (raw[:, n:] == PATTERN).all()
    for entry, r, bi, bd in got:
        assert np.array_equal(bi, rows[r][0]) and np.array_equal(bd, rows[r][1]), (entry, r, np.nonzero(bi != rows[r][0])[0][:5])
    return got


@pytest.mark.parametrize("sim3_form,th", [(False, 3.0), (True, 4.0)])
@pytest.mark.parametrize("u_right", [False, True], ids=["mono", "stereo"])
def test_fuse_host_batch_and_device_equal_literal(env, fuse_case, u_right, sim3_form, th):
    """np = 257, pcap = 290, flag rows that leave 0, 1, 8, 9, 63 and 64 valid records in single wavefronts."""
    rows = _expected_rows(fuse_case, u_right, sim3_form, th)
    for r in (0, 2):
        assert [int(rows[r][2]["valid"][64 * w:64 * w + 64].sum()) for w in range(5)] == WAVE_COUNTS[r]
    assert [int(rows[1][2]["valid"][64 * w:64 * w + 64].sum()) for w in range(5)] == WAVE_COUNTS[1]
    assert (rows[2][1] <= 50).sum() > 100
    _fuse_through_every_entry(env, fuse_case, u_right, sim3_form, th, rows)


@pytest.mark.parametrize("sim3_form", [False, True])
@pytest.mark.parametrize("u_right", [False, True], ids=["mono", "stereo"])
def test_fuse_ties_borders_and_gates_through_every_entry(env, u_right, sim3_form):
    """The hand-placed cases of the CPU module (|dx| == r, |dy| == r, the level window, equal distances in different
    cells, the chi-square gate on (float)7.8 and (float)5.99, a stereo key point next to a monocular one, mvuRight == 0,
    u on mnMaxX) as map points and key points of Fuse, FuseBatch and FuseDevice - so the distance / position / index key and
    the 8-lane minimum of k_fuse_batch meet them - against seqref's `fuse` and against the hand-worked answers."""
    E = C.fuse_edge_scene()
    rows = _expected_rows(E, u_right, sim3_form, E["th"])
    tie = [i for i, a in enumerate(E["answers"]) if a[0] == "tie in two cells"][0]
    assert rows[0][0][tie] == E["answers"][tie][2] and rows[0][1][tie] == 9          # the tie occurs: the higher index wins
    assert rows[0][0][0] == -1 and rows[0][0][1] >= 0                               # and so do the border cases
    for entry, r, bi, bd in _fuse_through_every_entry(env, E, u_right, sim3_form, E["th"], rows):
        if r != 1:
            C.check_fuse_edge_answers(E, bi, bd, rows[r][2], not sim3_form, u_right, E["flags"][r])


def test_kernel_records_against_the_float64_layer(env):
    """The kernels' own records under the constants of the CPU module: values within the bounds, decisions and levels
    equal wherever the fp64 margin clears its bound, at most 2 % of a scene left out."""
    cam, scam = C.make_cam()
    m = env["G"].m
    S = C.last_frame_scene(env["O"], "forward")
    q = m.ProjectLastFrame(cam, S["Tcw"], S["Tlw"], S["X"], S["flags"], S["keys"], 7.0, False)
    cases = [("last", q, None, P.project_last_frame_f64(scam, S["Tcw"], S["Tlw"], S["X"]), (S["flags"] & 1) == 1)]
    S = C.map_scene(1)
    q, vc = m.FrustumQueries(cam, S["T"], S["X"], S["nrm"], S["max_d"], S["min_d"], S["flags"], 0.5, 3.0)
    vc = np.where(q["valid"] == 1, vc, np.nan)
    cases.append(("frustum", q, vc, P.frustum_queries_f64(scam, S["T"], S["X"], S["nrm"], S["max_d"], S["min_d"], 0.5),
                  (S["flags"] & 1) == 1))
    S = C.map_scene(4)
    q = m.KeyFrameQueries(cam, 0, False, S["T"], None, S["X"], S["nrm"], S["max_d"], S["min_d"], S["flags"], 3.0)
    cases.append(("fuse", q, None, P.keyframe_queries_f64(scam, 0, S["T"], None, S["X"], S["nrm"], S["max_d"], S["min_d"]),
                  (S["flags"] & 1) == 1))
    S = C.sim3_scene(env["O"], 1.05, 12)
    S12, S21 = P.sim3_matrices(S["s12"], S["R12"], S["t12"])
    pts = S["pts1"]
    q = m.KeyFrameQueries(cam, 1, True, S["T1w"], S21, pts[0], None, pts[1], pts[2], pts[3], 7.5)
    ref = P.keyframe_queries_f64(scam, 1, S["T1w"], P.sim3_matrices_f64(S["s12"], S["R12"], S["t12"])[1], pts[0], None, pts[1], pts[2])
    ref.pop("ur")
    cases.append(("sim3", q, None, ref, pts[3] == 1))
    for name, q, vc, ref, present in cases:
        lit = dict(u=q["u"], v=q["v"])
        if "ur" in ref:
            lit["ur"] = q["ur"]
        if vc is not None:
            lit["view_cos"] = vc
        dev = C.deviations(lit, ref, q["valid"] == 1)
        assert dev and all(d <= C.BOUND[kind] for kind, d in dev.items()), (name, dev)
        C.decisions_agree(q["valid"], ref["margins"], present, name)
        if "level_real" in ref:
            C.levels_agree(q, ref["level_real"], scam, name)
