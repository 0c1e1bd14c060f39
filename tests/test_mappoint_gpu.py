"""orbhip_update_map_points_device / orbhip_update_map_points (MapPoint::ComputeDistinctiveDescriptors and
MapPoint::UpdateNormalAndDepth from an observation table over the key-frame bank) against tests/seqref/mappoint.py, bit for
bit: the random scene of test_mappoint_cpu.py (observation counts on both sides of the 16-lane group, the 64-lane row and
the LDS path; bad points, bad key frames, bad references), the 2048-observation limit, two calls back to back on one
stream, and the arrays handed to FuseDevice without a host copy."""
import ctypes as C

import numpy as np
import pytest

import test_mappoint_cpu as MC
import test_seqref_projection_cpu as PC
from helpers import synth_frame
from seqref import mappoint as MP
from seqref import matcher as SM
from seqref import projection as P

pytestmark = pytest.mark.gpu

f32 = np.float32
BOTH = MC.BOTH
PATTERN = MC.PATTERN
STATUS_FILL = 0x77


@pytest.fixture(scope="module")
def env():
    import torch
    import orb_slam2_comment_amd as pkg
    E = dict(pkg=pkg, torch=torch, dev=torch.device("cuda:0"), m=pkg.ORBmatcher(0.6, True))
    S = MC.scene_and_reference(BOTH)[0]
    E["S"] = S
    E["bank"] = upload_bank(E, S["keys"], S["desc"], S["T"], S["kf_bad"], MC.CAP)
    yield E
    E["m"].close()


def up(E, a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return E["torch"].from_numpy(a).to(E["dev"])


def upload_bank(E, keys, desc, T, kf_bad, cap):
    """Key-frame rows in the extractor's output layout: d_kps [rows][cap] records, d_desc [rows][cap][32], d_n, d_Tcw."""
    rows = len(keys)
    k = np.zeros((rows, cap), E["pkg"].KP_DTYPE)
    d = np.full((rows, cap, 32), 0xEE, np.uint8)
    n = np.zeros(rows, np.int32)
    for r in range(rows):
        n[r] = len(keys[r])
        k[r, :n[r]] = keys[r]
        d[r, :n[r]] = desc[r]
    return dict(k=up(E, k), d=up(E, d), n=up(E, n), T=up(E, np.stack([np.asarray(t, f32)[:3].reshape(12) for t in T])),
                bad=None if kf_bad is None else up(E, kf_bad), cap=cap)


class Call:
    """One device call: the table and the point arrays on the device, the outputs pre-filled with the sentinel pattern."""

    def __init__(self, E, bank, cam, what, start, okf, oidx, ref, world, flags, np_, pcap, first=0, launch=True):
        t, dev = E["torch"], E["dev"]
        self.E, self.bank, self.cam, self.what, self.np_, self.pcap, self.first = E, bank, cam, what, np_, pcap, first
        self.tab = [up(E, a) for a in (start, okf if len(okf) else np.zeros(1, np.int32), oidx if len(oidx) else np.zeros(1, np.int32))]
        pad = lambda a, fill: np.concatenate([a[first:first + np_], np.full((pcap - np_,) + a.shape[1:], fill, a.dtype)])  # noqa: E731
        self.ref = up(E, pad(np.asarray(ref, np.int32), 0))
        self.world, self.flags = up(E, pad(np.asarray(world, f32), 1e9)), up(E, pad(np.asarray(flags, np.uint8), 1))
        pd, nrm, mx, mn = MC.sentinels(pcap)
        self.out = [up(E, a) for a in (pd, nrm, mx, mn)]
        self.best = t.full((pcap,), PATTERN, dtype=t.int32, device=dev)
        self.status = t.full((pcap,), STATUS_FILL, dtype=t.uint8, device=dev)
        t.cuda.synchronize()
        if launch:
            self.launch()

    def launch(self):
        E, b, cam, what, np_, pcap, first = self.E, self.bank, self.cam, self.what, self.np_, self.pcap, self.first
        E["m"].UpdateMapPointsDevice(cam, what, b["T"].data_ptr(), b["k"].data_ptr(), b["d"].data_ptr(), b["n"].data_ptr(), b["cap"],
                                     np_, pcap, self.tab[0].data_ptr() + 4 * first, self.tab[1].data_ptr(), self.tab[2].data_ptr(),
                                     self.ref.data_ptr(), self.world.data_ptr(), self.flags.data_ptr(), self.out[0].data_ptr(),
                                     self.out[1].data_ptr(), self.out[2].data_ptr(), self.out[3].data_ptr(), self.status.data_ptr(),
                                     d_best_obs=self.best.data_ptr(), d_kf_bad=b["bad"].data_ptr() if b["bad"] is not None else 0)

    def results(self):
        return [a.cpu().numpy() for a in self.out] + [self.best.cpu().numpy(), self.status.cpu().numpy()]


def assert_equal_to_reference(got, ref, what, n, where, first=0, device_form=True):
    """The six arrays against seqref's for points first .. first + n, as bits; everything past n still holds the pattern."""
    pd, nrm, mx, mn, best, status = got
    rpd, rnrm, rmx, rmn, rbest, rstatus = (a[first:first + n] for a in ref)
    assert np.array_equal(status[:n], rstatus), (where, np.nonzero(status[:n] != rstatus)[0][:8], status[:n][status[:n] != rstatus][:8])
    if what & MP.UPDATE_DESCRIPTOR:
        assert np.array_equal(best[:n], rbest), (where, np.nonzero(best[:n] != rbest)[0][:8])
    elif device_form:
        assert (best[:n] == PATTERN).all(), where          # not selected: not written
    assert np.array_equal(pd[:n], rpd), (where, np.nonzero((pd[:n] != rpd).any(1))[0][:8])
    for name, a, b in (("normal", nrm, rnrm), ("max_dist", mx, rmx), ("min_dist", mn, rmn)):
        a, b = a[:n].view(np.int32), b.view(np.int32)
        assert np.array_equal(a, b), (where, name, np.nonzero((a != b).reshape(n, -1).any(1))[0][:8])
    if device_form:
        s = MC.sentinels(len(pd) - n)
        assert np.array_equal(pd[n:], s[0]) and all(np.array_equal(a[n:].view(np.int32), b.view(np.int32))
                                                    for a, b in zip((nrm, mx, mn), s[1:])), where
        assert (best[n:] == PATTERN).all() and (status[n:] == STATUS_FILL).all(), where


# ---- the random scene ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [MP.UPDATE_DESCRIPTOR, MP.UPDATE_NORMAL_DEPTH, BOTH], ids=["descriptor", "normal_depth", "both"])
def test_random_scene_device_and_host_equal_seqref(env, what):
    S, ref = MC.scene_and_reference(what)
    MC.assert_scene_is_not_vacuous(S, MC.scene_and_reference(BOTH)[1])      # from seqref, before any device work
    c = Call(env, env["bank"], S["cam"], what, S["obs_start"], S["obs_kf"], S["obs_idx"], S["ref_obs"], S["world"], S["flags"],
             MC.NPTS, MC.PCAP)
    env["m"].sync()
    assert_equal_to_reference(c.results(), ref, what, MC.NPTS, "device")
    # a skipped point keeps the pattern in the reference as well: the comparison above covers "written only where ..."
    skipped = np.nonzero(np.isin(ref[5], (MP.BAD, MP.NO_OBSERVATION)))[0]
    assert len(skipped) > 30 and (ref[0][skipped] == 0xA5).all()
    # host form
    pkg = env["pkg"]
    KFs = [pkg.FrameView(S["keys"][r], S["desc"][r], PC.SF, PC.BOUNDS) for r in range(MC.ROWS)]
    got = env["m"].UpdateMapPoints(S["cam"], what, KFs, S["T"], S["kf_bad"], S["obs_start"], S["obs_kf"], S["obs_idx"], S["ref_obs"],
                                   S["world"], S["flags"], *MC.sentinels(MC.NPTS))
    assert_equal_to_reference(got, ref, what, MC.NPTS, "host", device_form=False)
    if not what & MP.UPDATE_DESCRIPTOR:
        assert (got[4] == -1).all()


def test_a_prefix_of_the_points_and_no_bad_key_frames(env):
    """np = 37 of the same table (three workgroups of k_update_points, the last one partly filled), d_kf_bad null."""
    S = env["S"]
    n = 37
    pd, nrm, mx, mn = MC.sentinels(n)
    ref = MP.update_map_points(S["scam"], BOTH, S["T"], S["keys"], S["desc"], None, S["obs_start"][:n + 1], S["obs_kf"], S["obs_idx"],
                               S["ref_obs"], S["world"], S["flags"], pd, nrm, mx, mn)
    bank = dict(env["bank"], bad=None)
    c = Call(env, bank, S["cam"], BOTH, S["obs_start"], S["obs_kf"], S["obs_idx"], S["ref_obs"], S["world"], S["flags"], n, n + 5)
    env["m"].sync()
    assert_equal_to_reference(c.results(), ref, BOTH, n, "prefix")
    assert ref[5][MC.ONLY_BAD_KF_POINT] == MP.UPDATED


# ---- the limit of 2048 observations --------------------------------------------------------------------------------------
def test_limit_of_2048_observations(env):
    """N = 7, 2048, 2049, 40: the longest list that is served (rows and key points repeating, a quarter of it on bad key
    frames, most of its descriptors read past the LDS stage), one too many, and their neighbours."""
    S = env["S"]
    rng = np.random.default_rng(5)
    counts = [7, 2048, 2049, 40]
    slots = [rng.choice(2 * MC.FAMILY_SLOTS, N, replace=N > 2 * MC.FAMILY_SLOTS) + 3 * MC.FAMILY_SLOTS for N in counts]
    okf = np.concatenate([s % MC.ROWS for s in slots]).astype(np.int32)
    oidx = np.concatenate([s // MC.ROWS for s in slots]).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ref_obs = np.array([3, 1500, 7, 39], np.int32)
    world = rng.normal(0, 8, (4, 3)).astype(f32)
    flags = np.ones(4, np.uint8)
    ref = MP.update_map_points(S["scam"], BOTH, S["T"], S["keys"], S["desc"], S["kf_bad"], start, okf, oidx, ref_obs, world, flags,
                               *MC.sentinels(4))
    assert ref[5].tolist() == [MP.UPDATED, MP.UPDATED, MP.TOO_MANY, MP.UPDATED]
    assert ref[4][1] >= 0 and (ref[0][2] == 0xA5).all()
    c = Call(env, env["bank"], S["cam"], BOTH, start, okf, oidx, ref_obs, world, flags, 4, 6)
    env["m"].sync()
    assert_equal_to_reference(c.results(), ref, BOTH, 4, "limit")
    KFs = [env["pkg"].FrameView(S["keys"][r], S["desc"][r], PC.SF, PC.BOUNDS) for r in range(MC.ROWS)]
    got = env["m"].UpdateMapPoints(S["cam"], BOTH, KFs, S["T"], S["kf_bad"], start, okf, oidx, ref_obs, world, flags, *MC.sentinels(4))
    assert_equal_to_reference(got, ref, BOTH, 4, "limit, host", device_form=False)


def test_more_long_points_than_workgroups_of_the_worklist_kernel(env):
    """1300 points, 1094 of them with 17 observations and 6 with 65 (map_scale_cases.upd_case): more long points than
    k_update_points_long has workgroups, so the worklist is walked with the grid stride.  Device and host form."""
    import map_scale_cases as SC
    SC.preconditions("upd_long")
    S, K = env["S"], SC.upd_case()
    n = K["n"]
    c = Call(env, env["bank"], S["cam"], BOTH, K["start"], K["okf"], K["oidx"], K["ref_obs"], K["world"], K["flags"], n, n + 7)
    env["m"].sync()
    assert_equal_to_reference(c.results(), K["ref"], BOTH, n, "long points")
    KFs = [env["pkg"].FrameView(S["keys"][r], S["desc"][r], PC.SF, PC.BOUNDS) for r in range(MC.ROWS)]
    got = env["m"].UpdateMapPoints(S["cam"], BOTH, KFs, S["T"], S["kf_bad"], K["start"], K["okf"], K["oidx"], K["ref_obs"], K["world"],
                                   K["flags"], *MC.sentinels(n))
    assert_equal_to_reference(got, K["ref"], BOTH, n, "long points, host", device_form=False)


# ---- two calls back to back ----------------------------------------------------------------------------------------------
def test_two_calls_back_to_back_on_one_stream(env):
    """Points 0 .. 149 and 150 .. 299 of the scene as two calls without a synchronisation between them, then the other way
    round: each gives the rows of a call on its own (a stale worklist counter or stale LDS would not)."""
    S, ref = MC.scene_and_reference(BOTH)
    half = MC.NPTS // 2

    def call(first, launch=True):
        return Call(env, env["bank"], S["cam"], BOTH, S["obs_start"], S["obs_kf"], S["obs_idx"], S["ref_obs"], S["world"], S["flags"],
                    half, half + 3, first=first, launch=launch)
    alone = []
    for first in (0, half):
        c = call(first)
        env["m"].sync()
        alone.append(c.results())
        assert_equal_to_reference(alone[-1], ref, BOTH, half, "alone %d" % first, first=first)
    for order in ((0, half), (half, 0)):
        a, b = call(order[0], launch=False), call(order[1], launch=False)      # every upload is done before the first launch
        a.launch()
        b.launch()
        env["m"].sync()
        for c, first in ((a, order[0]), (b, order[1])):
            got, want = c.results(), alone[0 if first == 0 else 1]
            assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, want)), (order, first)


# ---- arguments against a live handle ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written(env):
    pkg, t = env["pkg"], env["torch"]
    from orb_slam2_comment_amd import capi
    S, b, m = env["S"], env["bank"], env["m"]
    L, h = capi.lib(), m._h
    n, pcap = 20, 24
    c = Call(env, b, S["cam"], BOTH, S["obs_start"], S["obs_kf"], S["obs_idx"], S["ref_obs"], S["world"], S["flags"], n, pcap)
    m.sync()
    done = c.results()
    dp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def device(what=BOTH, np_=n, pcap_=pcap, cap=b["cap"], **null):
        a = dict(T=dp(b["T"]), k=dp(b["k"]), d=dp(b["d"]), start=dp(c.tab[0]), okf=dp(c.tab[1]), oidx=dp(c.tab[2]), ref=dp(c.ref),
                 world=dp(c.world), flags=dp(c.flags), pd=dp(c.out[0]), nrm=dp(c.out[1]), mx=dp(c.out[2]), mn=dp(c.out[3]),
                 status=dp(c.status))
        a.update({k: None for k in null})
        return L.orbhip_update_map_points_device(h, C.byref(S["cam"]), what, a["T"], a["k"], a["d"], dp(b["n"]), cap, dp(b["bad"]),
                                                 np_, pcap_, a["start"], a["okf"], a["oidx"], a["ref"], a["world"], a["flags"],
                                                 a["pd"], a["nrm"], a["mx"], a["mn"], dp(c.best), a["status"])
    for what in (0, 4, 7, -1):
        assert device(what=what) == capi.E_ARG
    assert device(np_=-1) == capi.E_ARG and device(np_=pcap + 1) == capi.E_ARG and device(cap=0) == capi.E_ARG
    assert device(cap=4097) == capi.E_CAPACITY
    for name in ("start", "okf", "oidx", "flags", "status", "d", "pd", "T", "k", "ref", "world", "nrm", "mx", "mn"):
        assert device(**{name: True}) == capi.E_ARG, name
    # a pointer the selected bit does not need may be null
    assert device(what=MP.UPDATE_DESCRIPTOR, T=True, k=True, ref=True, world=True, nrm=True, mx=True, mn=True) == capi.OK
    assert device(what=MP.UPDATE_NORMAL_DEPTH, d=True, pd=True) == capi.OK
    assert device(np_=0) == capi.OK and device(np_=0, pcap_=0, start=True, status=True) == capi.OK
    m.sync()
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(c.results(), done))
    # host form: rows and key points outside the bank, a decreasing obs_start
    KFs = [pkg.FrameView(S["keys"][r], S["desc"][r], PC.SF, PC.BOUNDS) for r in range(MC.ROWS)]
    start, okf, oidx = S["obs_start"][:n + 1].copy(), S["obs_kf"].copy(), S["obs_idx"].copy()

    def host(start=start, okf=okf, oidx=oidx, what=BOTH):
        return m.UpdateMapPoints(S["cam"], what, KFs, S["T"], S["kf_bad"], start, okf, oidx, S["ref_obs"][:n], S["world"][:n],
                                 S["flags"][:n], *MC.sentinels(n))
    host()
    for bad in (dict(okf=np.where(np.arange(len(okf)) == 5, MC.ROWS, okf)), dict(okf=np.where(np.arange(len(okf)) == 5, -1, okf)),
                dict(oidx=np.where(np.arange(len(oidx)) == 9, MC.NKEYS, oidx)), dict(oidx=np.where(np.arange(len(oidx)) == 9, -1, oidx)),
                dict(start=np.concatenate([start[:6], [start[6] - 9], start[7:]])), dict(what=0), dict(what=8)):
        with pytest.raises(capi.OrbHipError) as e:
            host(**{k: (np.ascontiguousarray(v, np.int32) if k != "what" else v) for k, v in bad.items()})
        assert e.value.code == capi.E_ARG, bad.keys()
    empty = m.UpdateMapPoints(S["cam"], BOTH, KFs, S["T"], None, [0], [], [], [], np.zeros((0, 3), f32), [], *MC.sentinels(0))
    assert all(len(a) == 0 for a in empty)


# ---- end to end: refresh, then Fuse, nothing on the host in between -------------------------------------------------------
SHIFTS = [(0, 0), (4, 2), (2, 1), (6, 3)]


def test_refreshed_arrays_feed_fuse_device_without_a_host_copy(env):
    """Four key frames extracted at 320x240 (one image, shifted), map points from the key points of frame 0 observed where
    the shifted frames have the same corner: UpdateMapPointsDevice writes descriptor, normal and depth range, FuseDevice
    reads them on the same stream; the rows equal seqref's Fuse run on seqref's refreshed arrays."""
    t, pkg, m = env["torch"], env["pkg"], env["m"]
    W, H, K = PC.W, PC.H, len(SHIFTS)
    cam, scam = PC.make_cam()
    ext = pkg.ORBextractor(PC.NF, 1.2, 8, 20, 7)
    cap = ext.capacity(H, W)
    d_img = up(env, np.stack([synth_frame(41, W, H, shift_xy=s) for s in SHIFTS]))
    d_k = t.zeros((K, cap, 7), dtype=t.int32, device=env["dev"])
    d_d = t.zeros((K, cap, 32), dtype=t.uint8, device=env["dev"])
    d_n = t.zeros(K, dtype=t.int32, device=env["dev"])
    t.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), K, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    ext.sync()
    n = d_n.cpu().numpy()
    hk = d_k.cpu().numpy().view(np.uint8).reshape(K, cap, 28).view(pkg.KP_DTYPE).reshape(K, cap)
    hd = d_d.cpu().numpy()
    kd = [(hk[f, :n[f]].copy(), hd[f, :n[f]].copy()) for f in range(K)]
    assert n.min() > 300
    rng = np.random.default_rng(17)
    T0 = PC.pose(rng, small=False)
    T = [T0] + [(PC.pose(rng).astype(np.float64) @ T0.astype(np.float64)).astype(f32) for _ in range(K - 1)]
    npts = 300
    k0 = kd[0][0][:npts]
    X = PC.back_project(np.stack([k0["x"], k0["y"]], 1), rng.uniform(3, 30, npts), T0)
    start, okf, oidx, ref_obs = [0], [], [], []
    for i in range(npts):
        obs = [(0, i)]
        for f in range(1, K):
            kf = kd[f][0]
            d2 = (kf["x"] - (k0["x"][i] + SHIFTS[f][0])) ** 2 + (kf["y"] - (k0["y"][i] + SHIFTS[f][1])) ** 2
            d2 = np.where(kf["octave"] == k0["octave"][i], d2, 1e9)
            if d2.min() < 4.0:
                obs.append((f, int(np.argmin(d2))))
        obs = [obs[j] for j in rng.permutation(len(obs))]
        ref_obs.append(obs.index((0, i)))
        okf += [o[0] for o in obs]
        oidx += [o[1] for o in obs]
        start.append(len(okf))
    start, okf, oidx, ref_obs = (np.array(a, np.int32) for a in (start, okf, oidx, ref_obs))
    assert (np.diff(start) >= 3).sum() > 100                       # most corners are found again in the shifted frames
    pflags = np.where(rng.random(npts) < 0.1, 0, 1).astype(np.uint8)
    init = (np.zeros((npts, 32), np.uint8), np.tile(f32([0, 0, 1]), (npts, 1)), np.ones(npts, f32), np.full(npts, 0.1, f32))
    pd, nrm, mx, mn, best, status = MP.update_map_points(scam, BOTH, T, [k for k, _ in kd], [d for _, d in kd], None, start, okf,
                                                         oidx, ref_obs, X, pflags, *init)
    assert (status == MP.UPDATED).sum() > 250
    fflags = ((rng.random((K, npts)) < 0.9) & (pflags[None, :] == 1)).astype(np.uint8)
    th = 3.0
    rows = [P.fuse(SM.Frame(kd[f][0], kd[f][1], None, PC.BOUNDS, PC.SF), scam, T[f], X, nrm, mx, mn, fflags[f], pd, th, PC.INV_SIGMA2,
                   False) for f in range(K)]
    assert (rows[0][1] <= 50).sum() > 100                          # frame 0 finds its own points: the search is not vacuous
    # the device: table and point arrays up, two calls on the matcher's stream, one synchronisation at the end
    pcap = npts + 9
    d_T = up(env, np.stack([np.asarray(x, f32)[:3].reshape(12) for x in T]))
    tab = [up(env, a) for a in (start, okf, oidx, ref_obs)]
    padded = lambda a, fill: up(env, np.concatenate([a, np.full((pcap - npts,) + a.shape[1:], fill, a.dtype)]))  # noqa: E731
    dX, dpf = padded(X, 1e9), padded(pflags, 1)
    dP, dN, dMx, dMn = (padded(a, f) for a, f in zip(init, (0xAA, 1e9, 1e9, 1e9)))
    ff = np.ones((K, pcap), np.uint8)
    ff[:, :npts] = fflags
    d_ff = up(env, ff)
    d_idx = up(env, np.arange(K, dtype=np.int32))
    d_status = t.full((pcap,), STATUS_FILL, dtype=t.uint8, device=env["dev"])
    d_bi = t.full((K, pcap), PATTERN, dtype=t.int32, device=env["dev"])
    d_bd = t.full((K, pcap), PATTERN, dtype=t.int32, device=env["dev"])
    t.cuda.synchronize()
    m.UpdateMapPointsDevice(cam, BOTH, d_T.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, npts, pcap,
                            tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), dX.data_ptr(), dpf.data_ptr(),
                            dP.data_ptr(), dN.data_ptr(), dMx.data_ptr(), dMn.data_ptr(), d_status.data_ptr())
    m.FuseDevice(K, d_idx.data_ptr(), cam, d_T.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), cap, npts, pcap,
                 dX.data_ptr(), dN.data_ptr(), dMx.data_ptr(), dMn.data_ptr(), dP.data_ptr(), d_ff.data_ptr(), th, PC.INV_SIGMA2,
                 d_bi.data_ptr(), d_bd.data_ptr())
    m.sync()
    assert np.array_equal(d_status.cpu().numpy()[:npts], status)
    assert np.array_equal(dP.cpu().numpy()[:npts], pd) and np.array_equal(dN.cpu().numpy()[:npts].view(np.int32), nrm.view(np.int32))
    bi, bd = d_bi.cpu().numpy(), d_bd.cpu().numpy()
    for f in range(K):
        assert np.array_equal(bi[f, :npts], rows[f][0]) and np.array_equal(bd[f, :npts], rows[f][1]), f
    assert (bi[:, npts:] == PATTERN).all() and (bd[:, npts:] == PATTERN).all()
