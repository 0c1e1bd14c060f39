"""Scenes that take the three optimiser entries past one chunk, one grid and one tile block; shared by
test_optimizer_scale_cpu.py and test_optimizer_scale_gpu.py.  The builders, pack / unpack / run_host, prefilled and assert_same
are those of test_lba_cpu.py, test_gba_cpu.py and test_essgraph_cpu.py; only the bulk observation helper is new (one numpy pass
per row instead of one Python call per observation).

Every case names the thresholds it must cross; gba_ / lba_ / eg_preconditions(name) check them on the reference's report, so a later
change of a grid size or a capacity shows up as a failed precondition, not as a silently shrunken test.

Which reference a case has (REFERENCE below): tests/seqref where that runs in a few seconds, else the one-thread host program
(tests/cpp/*_host.cpp, g++ -ffp-contract=off); test_optimizer_scale_cpu.py pins host == seqref on every case of the first kind."""
import functools

import numpy as np

import test_essgraph_cpu as KE
import test_gba_cpu as KG
import test_lba_cpu as KL
from orb_slam2_comment_amd import capi
from seqref import gba as G
from seqref import lba as L
from seqref.sim3opt import sim3_inverse

f32, f64, i32, u8 = np.float32, np.float64, np.int32, np.uint8

# ---------------------------------------------------------------------------------------------------------------------
# The kernel-private sizes the cases are built around (the public ones come from capi).  Each names its source line.
CHUNK = 1024            # orbhip_gba.hip:33 kBig, orbhip_essgraph.hip:30 kBig, orbhip_lba.hip:31 kSetupThreads: lanes of a setup / finish workgroup
ITEM = 256              # orbhip_gba.hip:33 kItem, orbhip_essgraph.hip:30 kItem, orbhip_lba.hip:31 kItemThreads, orbhip_ldlt.h:24 kItem
WAVE = 64               # orbhip_lba_core.h:24 kLbaWave, orbhip_essgraph_core.h:30 kEgWave
LBA_ITEM_BLOCKS = 120   # orbhip_lba.hip:31 kItemBlocks
LBA_SCHUR_BLOCKS = 256  # orbhip_lba.hip:31 kSchurBlocks
GBA_ITEM_BLOCKS = 240   # orbhip_gba.hip:33 kItemBlocks
GBA_SCHUR_BLOCKS = 1024  # orbhip_gba.hip:33 kSchurBlocks
EG_ITEM_BLOCKS = 240    # orbhip_essgraph.hip:30 kItemBlocks
GBA_NB = 24             # orbhip_gba_core.h:19 kGbaNb: columns of a panel
EG_NB = 28              # orbhip_essgraph_core.h:29 kEgNb with the product's ORBHIP_EG_PANEL of 4
TILE = 64               # orbhip_ldlt.h:24 kTile

LBA_ITEMS = LBA_ITEM_BLOCKS * ITEM                          # 30 720: the second pass of an LBA item loop starts here
GBA_ITEMS = GBA_ITEM_BLOCKS * ITEM                          # 61 440
LBA_SCHUR_WAVES = LBA_SCHUR_BLOCKS * ITEM // WAVE           # 1024 pose pairs per pass of k_lba_schur
GBA_SCHUR_WAVES = GBA_SCHUR_BLOCKS * ITEM // WAVE           # 4096 pose pairs per pass of k_gba_schur
EG_TEAMS = EG_ITEM_BLOCKS * ITEM // WAVE                    # 960 edges per pass of k_eg_eval / k_eg_blocks
LBA_SETUP_WAVES = CHUNK // WAVE                             # 16 free poses per pass of the edge index of k_lba_setup


def bwd_block1_free(nb, per_pose):
    """Free vertices from which block 1 of k_bwd_upd has work: a panel that starts above column ITEM (orbhip_ldlt.h)."""
    return (ITEM // nb + 1) * nb // per_pose + 1


REFERENCE = dict(
    gba=dict(pts="seqref", pts_perm="seqref", pts_points_plus_one="seqref", pts_edges_plus_one="seqref", pts_null="seqref",
             rows1100="seqref", f70="seqref", pivot="seqref", f250="host", e61k="host", full512="host"),
    lba=dict(pts1100="seqref", f40="seqref", f129="seqref", f128="host", e31k="host"),
    eg=dict(rows1100="seqref", e960="seqref", pts1100="seqref", f150="host"))


# ---------------------------------------------------------------------------------------------------------------------
# observations in bulk
def bulk_observe(sc, pts, rows, stereo, noise=0.3, offset=None):
    """Scene.observe for arrays: observation k is point pts[k] in row rows[k].  The slots of a row are taken in the order of k,
    and a point's observations are listed in that order too.  offset [k, 2]: a displacement in pixels (gross outliers)."""
    fx, fy, cx, cy, bf = KL.CAM
    pts, rows, stereo = np.asarray(pts, np.int64), np.asarray(rows, np.int64), np.asarray(stereo, bool)
    slot = np.zeros(len(pts), np.int64)
    for r in np.unique(rows):
        k = np.nonzero(rows == r)[0]
        s = int(sc.n[r]) + np.arange(len(k))
        assert s[-1] < sc.cap, "row %d is full" % r
        slot[k] = s
        Xc = sc.X[pts[k]] @ sc.R[r].T + sc.t[r]
        sig = 1.2 ** sc.kps["octave"][r, s].astype(f64)
        z = Xc[:, 2]
        u = fx * Xc[:, 0] / z + cx + sc.rng.normal(0, noise, len(k)) * sig
        v = fy * Xc[:, 1] / z + cy + sc.rng.normal(0, noise, len(k)) * sig
        if offset is not None:
            u, v = u + offset[k, 0], v + offset[k, 1]
        sc.kps["x"][r, s], sc.kps["y"][r, s] = u, v
        sc.ur[r, s] = np.where(stereo[k], u - bf / z, -1.0)
        sc.slot_point[r, s] = pts[k]
        sc.n[r] += len(k)
    for p, r, s in zip(pts.tolist(), rows.tolist(), slot.tolist()):
        sc.obs[p].append((r, s))


def _points_in_front(sc, count, x_hi):
    for X in np.c_[sc.rng.uniform(-2, x_hi, count), sc.rng.uniform(-2, 2, count), sc.rng.uniform(6, 16, count)]:
        sc.point(X)


def _random_observers(sc, npts, rows, k):
    """k distinct rows of `rows` for each of npts points, ascending per point: (pts, rows) for bulk_observe."""
    rows = np.asarray(rows)
    pick = np.sort(np.argsort(sc.rng.random((npts, len(rows))), axis=1)[:, :k], axis=1)
    return np.repeat(np.arange(npts), k), rows[pick].reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# global bundle adjustment
GBA_CASES = list(REFERENCE["gba"])
GBA_PTS = 1500                                                                  # listed points of the `pts` family: two chunks


def _gba_scene_pts(null=False):
    """Rows 0 (mnId 0) and 1-8 are the vertices; row 9 is bad (listed); row 10 is the newest and is not listed, so its
    observations are skipped through maxKFid; row 11 is old and not listed: a null vertex, observed in the `null` form only.
    Point p is of kind p % 5: 0, 1, 2 ordinary (two observers among rows 0-8); 3 seen by rows 9 and 10 only, so it is removed;
    4 ordinary with a third observation by row 10 (and a fourth by row 11 in the `null` form).  Every 13th point is not PRESENT.
    Each kind occurs in both chunks of 1024 listed points."""
    sc = KL.Scene(12, 800, GBA_PTS, 101)
    KL._line_of_cameras(sc, range(12), step=0.6)
    sc.bad[9] = 1
    _points_in_front(sc, GBA_PTS, 0.6 * 12 + 2)
    kind = np.arange(GBA_PTS) % 5
    P, R = _random_observers(sc, GBA_PTS, range(9), 2)
    keep = kind[P] != 3
    P, R = P[keep], R[keep]
    extra = [(p, r) for p in range(GBA_PTS) for r in ((9, 10) if kind[p] == 3 else (10, 11) if kind[p] == 4 and null else (10,) if kind[p] == 4 else ())]
    P, R = np.r_[P, [e[0] for e in extra]], np.r_[R, [e[1] for e in extra]]
    order = np.lexsort((R, P))
    P, R = P[order], R[order]
    bulk_observe(sc, P, R, sc.rng.random(len(P)) < 0.5)
    sc.flags[np.arange(GBA_PTS) % 13 == 7] = 0
    kf_id = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 40, 5]
    return sc, kf_id


@functools.lru_cache(maxsize=None)
def gba_case(name):
    if name in ("pts", "pts_perm", "pts_points_plus_one", "pts_edges_plus_one", "pts_null"):
        sc, kf_id = _gba_scene_pts(null=name == "pts_null")
        b = KG._case(sc, kf_id=kf_id, iterations=2, kf_list=list(range(10)))
        if name == "pts_perm":                                                  # vpMP in an order of its own, a few left out
            perm = np.random.default_rng(7).permutation(GBA_PTS)[:GBA_PTS - 9]
            b = dict(b, pt_list=[int(p) for p in perm], mode=G.IN_PLACE)
        if name == "pts_points_plus_one":
            b = dict(b, max_points=int(gba_reference("pts")["report"][3]) - 1)
        if name == "pts_edges_plus_one":
            b = dict(b, max_edges=int(gba_reference("pts")["report"][5] + gba_reference("pts")["report"][6]) - 1)
        return b
    if name == "rows1100":
        # 1100 rows listed in an order of its own; 38 are good, half of them in either chunk of the list; the row of mnId 0
        # is the last good one of the list
        rows, rng = 1100, np.random.default_rng(102)
        sc = KL.Scene(rows, 40, 160, 102)
        kf_list = [int(r) for r in rng.permutation(rows)]
        at = sorted(rng.choice(CHUNK, 19, replace=False).tolist()) + sorted((CHUNK + rng.choice(rows - CHUNK, 19, replace=False)).tolist())
        good = [kf_list[k] for k in at]
        sc.bad[:] = 1
        KL._line_of_cameras(sc, good, step=0.3)
        for r in good:
            sc.bad[r] = 0
        _points_in_front(sc, 160, 0.3 * 38 + 2)
        P, R = _random_observers(sc, 160, good, 4)
        order = np.lexsort((R, P))
        bulk_observe(sc, P[order], R[order], sc.rng.random(len(P)) < 0.5)
        some_bad = [r for r in range(rows) if sc.bad[r]][:30]
        for p in range(0, 160, 5):                                              # and observations by bad rows: skipped
            sc.observe(p, some_bad[p // 5 % 30])
        kf_id = np.arange(1, rows + 1)
        kf_id[good[-1]] = 0
        b = KG._case(sc, kf_id=kf_id, iterations=2, kf_list=kf_list)
        b["id0_at"] = at[-1]
        b["good_at"] = at
        return b
    if name == "f70":
        return KG._case(KG.make_scene(170, 71, 212, 16, see=0.0, min_obs=3), iterations=2)
    if name == "pivot":
        # 9 free poses; a point at zero depth in the input estimate of free pose 5, observed by free poses 5 and 7 only: the first
        # panel (poses 0-3) factorises, the second meets a pivot that is a NaN
        sc = KG.make_scene(171, 10, 60, 48, see=0.5, pcap=61)
        p = sc.point([3.0, 0.1, 9.0])
        sc.observe(p, 6)
        sc.observe(p, 8, stereo=True)
        b = KG._case(sc, iterations=2)
        t = b["tables"]
        t["Tcw"][6] = np.c_[np.eye(3), np.zeros(3)].reshape(12).astype(f32)
        t["world"][p] = (0.0, 0.0, 0.0)
        b["zero_point"] = p
        return b
    if name == "f250":
        return KG._case(_gba_sparse(172, 251, 3), iterations=1)
    if name == "full512":
        # ORBHIP_GBA_MAX_KF counts vertices, the fixed row included: 512 good rows are 511 free poses (n = 3066), and the 513th
        # row is the refusal test_gba_cpu.py already has (rows_513)
        return KG._case(_gba_sparse(173, capi.GBA_MAX_KF, 2), iterations=1)
    if name == "e61k":
        # 41 rows, 62 000 points with two observers each: 124 000 edges, so the loops over points wrap too.  The input estimate is
        # far off (0.1 rad, 0.4 m, points 1 m), so that the gain ratio of the first trial lies where g2o does not clamp the factor
        # of lambda (see gba_preconditions): only then does the chi2 sum of a trial -- the one place the errors of k_gba_trial
        # go -- reach the outputs, through the damping of the second iteration
        return _gba_e61k((0.1, 0.4), 1.0)
    raise KeyError(name)


def _gba_e61k(pose_noise, point_noise):
    sc = KL.Scene(41, 3500, 62000, 174)
    KL._line_of_cameras(sc, range(41), step=0.3)
    _points_in_front(sc, 62000, 0.3 * 41 + 2)
    P, R = _random_observers(sc, 62000, range(41), 2)
    bulk_observe(sc, P, R, sc.rng.random(len(P)) < 0.5)
    return KG._case(sc, iterations=2, pose_noise=pose_noise, point_noise=point_noise)


def _gba_sparse(seed, rows, per_pose):
    """per_pose points for every row, each seen by three neighbouring rows: a banded system with few points and edges."""
    npts = per_pose * rows
    sc = KL.Scene(rows, 16, npts, seed)
    KL._line_of_cameras(sc, range(rows), step=0.25)
    first = np.minimum(np.arange(npts) // per_pose, rows - 3)
    for X in np.c_[0.25 * first + sc.rng.uniform(-1, 1.5, npts), sc.rng.uniform(-2, 2, npts), sc.rng.uniform(6, 16, npts)]:
        sc.point(X)
    P = np.repeat(np.arange(npts), 3)
    R = (first[:, None] + np.arange(3)[None, :]).reshape(-1)
    bulk_observe(sc, P, R, sc.rng.random(len(P)) < 0.5)
    return sc


def gba_host_state(b):
    """(lambda, rho, chi2) where the last trial of the host program leaves Levenberg-Marquardt (gba_host ... state)."""
    import subprocess

    def run(d):
        fin, fout = d / "s.in", d / "s.out"
        fin.write_bytes(KG.pack(b, KG.prefilled(b), None))
        subprocess.run([KG.host_program(), "ba", str(fin), str(fout), "0", "state"], check=True)
        return [float(v) for v in np.frombuffer(fout.read_bytes()[-24:], f64)]
    return _in_tmp(run)


@functools.lru_cache(maxsize=None)
def gba_reference(name):
    b = gba_case(name)
    if REFERENCE["gba"][name] == "seqref":
        return KG.run_seqref(b)
    return _in_tmp(lambda d: {k: np.array(v) for k, v in KG.run_host(b, d, name).items()})


def _in_tmp(fn):
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory(prefix="optimizer_scale_") as d:
        return fn(pathlib.Path(d))


@functools.lru_cache(maxsize=None)                                               # a case that passed is not checked again
def gba_preconditions(name):
    """Raises AssertionError naming the precondition that the reference's report does not meet."""
    b, ref = gba_case(name), gba_reference(name)
    rep = [int(v) for v in ref["report"]]
    nfree, npts, ne = rep[2], rep[3], rep[5] + rep[6]
    if name in ("pts_points_plus_one", "pts_edges_plus_one"):
        assert rep[0] == capi.GBA_CAPACITY, "%s: status %d is not ORBHIP_GBA_CAPACITY" % (name, rep[0])
        assert npts > CHUNK, "%s: %d points included, the excess does not lie past the first chunk of %d" % (name, npts, CHUNK)
        return
    assert rep[0] == capi.GBA_OK, "%s: status %d" % (name, rep[0])
    assert rep[10] >= 1, "%s: no trial" % name
    if name != "pivot":
        assert _gba_moved(b, ref), "%s: no Levenberg-Marquardt step was accepted" % name
    if name.startswith("pts"):
        listed = b["np"] if b["pt_list"] is None else len(b["pt_list"])
        assert listed > CHUNK and npts > CHUNK, "%s: %d listed and %d included points do not pass %d" % (name, listed, npts, CHUNK)
        order = list(range(b["np"])) if b["pt_list"] is None else b["pt_list"]
        t = b["tables"]
        for lo in range(0, listed, CHUNK):
            kinds = {int(p) % 5 for p in order[lo:lo + CHUNK] if t["flags"][p]}
            assert kinds == {0, 1, 2, 3, 4}, "%s: the chunk at %d lacks a kind of point (%s)" % (name, lo, sorted(kinds))
        assert rep[4] > 0 and rep[7] > 0, "%s: removed %d, skipped %d" % (name, rep[4], rep[7])
        assert (rep[8] > 0) == (name == "pts_null"), "%s: %d null observations" % (name, rep[8])
    if name == "rows1100":
        assert len(b["kf_list"]) > CHUNK and rep[1] <= 64, "%s: %d listed rows, %d vertices" % (name, len(b["kf_list"]), rep[1])
        assert min(b["good_at"]) < CHUNK <= max(b["good_at"]) and b["id0_at"] >= CHUNK, "%s: the good rows are not in both chunks" % name
        assert nfree == rep[1] - 1, "%s: no fixed row" % name
    if name == "f70":
        assert nfree * nfree > GBA_SCHUR_WAVES, "%s: %d free poses do not wrap k_gba_schur" % (name, nfree)
        assert nfree >= bwd_block1_free(GBA_NB, 6), "%s: %d free poses leave block 1 of k_bwd_upd idle" % (name, nfree)
        assert 6 * nfree > 4 * TILE + GBA_NB, "%s: fewer than five trailing tile rows" % name
    if name == "f250":
        assert nfree * nfree > GBA_ITEMS, "%s: %d free poses do not wrap the cov zeroing" % (name, nfree)
    if name == "e61k":
        assert ne > GBA_ITEMS and npts > GBA_ITEMS and rep[1] <= 41, "%s: %d edges, %d points do not pass %d" % (name, ne, npts, GBA_ITEMS)
        # lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)): a function of rho only for (2 rho - 1)^3 between 1/3 and 2/3
        rho = gba_host_state(dict(b, iterations=1))[1]
        assert 1.0 / 3.0 < (2 * rho - 1) ** 3 < 2.0 / 3.0 and rep[9] == 2, \
            "%s: the gain ratio %.4f of the first trial is clamped away, the sum over the trial's errors leaves no trace" % (name, rho)
    if name == "full512":
        assert rep[1] == capi.GBA_MAX_KF and nfree == rep[1] - 1, "%s: %d vertices, %d free poses" % (name, rep[1], nfree)
    if name == "pivot":
        assert nfree > 2 * GBA_NB // 6, "%s: one panel only" % name
        t = b["tables"]
        p = b["zero_point"]
        seen = [int(t["obs_kf"][o]) for o in range(t["obs_start"][p], t["obs_start"][p + 1])]
        assert min(seen) - 1 >= GBA_NB // 6, "%s: the zero-depth point is seen by a pose of the first panel" % name
        tr = {}
        KG.run_seqref(b, trace=tr)
        assert tr["decisions"][0][0] is False and tr["decisions"][0][3] == G.DBL_MAX, "%s: the first trial did not fail" % name


def _gba_moved(b, ref):
    t = b["tables"]
    out = ref["TcwGBA"] if b["mode"] == G.STAGED else ref["Tcw"]
    out = np.asarray(out).reshape(-1, 12)
    rows = [r for r in range(b["rows"]) if t["kf_id"][r] != 0 and not t["kf_bad"][r] and (b["kf_list"] is None or r in b["kf_list"])]
    return any(out[r].tobytes() != KG._round_trip(t["Tcw"][r]).tobytes() for r in rows)


# ---------------------------------------------------------------------------------------------------------------------
# local bundle adjustment
LBA_CASES = list(REFERENCE["lba"])


def _lba_window(seed, nlocal, npts, per_point, cap, id0=True, extra_rows=2, gross=0.0):
    """Rows 0 .. nlocal - 1 are local (cur = 0, the others in its covisibility list; row nlocal - 1 is the row of mnId 0 when
    id0), followed by extra_rows fixed cameras.  Every point gets per_point observers among all rows; a fraction `gross` of the
    observations is displaced by 15 to 40 pixels."""
    rows = nlocal + extra_rows
    sc = KL.Scene(rows, cap, npts, seed)
    KL._line_of_cameras(sc, range(rows), step=8.0 / rows)
    _points_in_front(sc, npts, 10.0)
    P, R = _random_observers(sc, npts, range(rows), per_point)
    ang, mag = sc.rng.uniform(0, 2 * np.pi, len(P)), sc.rng.uniform(15, 40, len(P))
    off = np.where((sc.rng.random(len(P)) < gross)[:, None], np.c_[mag * np.cos(ang), mag * np.sin(ang)], 0.0)
    bulk_observe(sc, P, R, sc.rng.random(len(P)) < 0.5, offset=off)
    t = sc.tables(0, list(range(1, nlocal)), pose_noise=(0.002, 0.01), point_noise=0.02)
    total = int(t["obs_start"][-1])
    return KL._case(t, 0, nlocal - 1 if id0 else -1, npts, total)


@functools.lru_cache(maxsize=None)
def lba_case(name):
    if name == "pts1100":
        # rows 0-5 local (cur = 0 sees every point, so the local points are 0 .. 1099 in order), 6-9 fixed; rows 8 and 9 see
        # points from 1040 on only: fixed cameras found through the second chunk; 3 % gross outliers, in both chunks
        npts = 1100
        sc = KL.Scene(10, 1200, npts, 201)
        KL._line_of_cameras(sc, range(10), step=0.6)
        _points_in_front(sc, npts, 8.0)
        P, R = _random_observers(sc, npts, range(1, 8), 2)
        late = np.arange(1040, npts)
        P = np.r_[np.arange(npts), P, late, late[::2]]
        R = np.r_[np.zeros(npts, np.int64), R, np.full(len(late), 8), np.full(len(late[::2]), 9)]
        order = np.lexsort((R, P))
        P, R = P[order], R[order]
        gross = sc.rng.random(len(P)) < 0.03
        ang, mag = sc.rng.uniform(0, 2 * np.pi, len(P)), sc.rng.uniform(15, 40, len(P))
        off = np.where(gross[:, None], np.c_[mag * np.cos(ang), mag * np.sin(ang)], 0.0)
        bulk_observe(sc, P, R, sc.rng.random(len(P)) < 0.5, offset=off)
        t = sc.tables(0, [1, 2, 3, 4, 5], pose_noise=(0.002, 0.01), point_noise=0.02)
        return KL._case(t, 0, -1, npts, int(t["obs_start"][-1]))
    if name == "f40":
        return _lba_window(202, 40, 160, 4, 40, id0=False)
    if name == "f128":
        return _lba_window(203, capi.LBA_MAX_LOCAL + 1, 390, 3, 24)
    if name == "f129":
        return _lba_window(204, capi.LBA_MAX_LOCAL + 2, 390, 3, 24)
    if name == "e31k":
        # 16 local rows and 2 fixed, 32 000 points with two observers each: 64 000 edges, 1 % gross outliers; the loops over
        # points wrap too
        return _lba_window(205, 16, 32000, 2, 3900, id0=False, gross=0.01)
    raise KeyError(name)


def _lba_seqref_fast(b):
    """tests/seqref/lba.py with the trailing update of its LDLt done row-wise in numpy (gba.ldlt_solve_rows, which
    test_gba_cpu.py pins to lba.ldlt_solve bit for bit): the pure-Python one takes n^3 / 6 interpreted steps per trial."""
    keep = L.ldlt_solve
    L.ldlt_solve = lambda A, rhs: keep(A, rhs) if len(rhs) <= G.SMALL else G.ldlt_solve_rows(A, rhs)
    try:
        return KL.run_seqref(b)
    finally:
        L.ldlt_solve = keep


@functools.lru_cache(maxsize=None)
def lba_reference(name):
    b = lba_case(name)
    if REFERENCE["lba"][name] == "seqref":
        r = _lba_seqref_fast(b)
        return dict(KL.as_arrays(b, r))
    got = _in_tmp(lambda d: {k: np.array(v) for k, v in KL.run_host(b, d, name).items()})
    got.pop("trace")
    got["erase"] = got["erase"].reshape(-1, 3)
    got["Tcw"], got["world"] = got["Tcw"].reshape(-1, 12), got["world"].reshape(-1, 3)
    return got


@functools.lru_cache(maxsize=None)                                               # a case that passed is not checked again
def lba_preconditions(name):
    b, ref = lba_case(name), lba_reference(name)
    rep = [int(v) for v in ref["report"]]
    nfree = rep[1] - (1 if b["id0_row"] >= 0 else 0)
    if name == "f129":
        assert rep[0] == capi.LBA_CAPACITY, "%s: status %d is not ORBHIP_LBA_CAPACITY" % (name, rep[0])
        assert nfree == capi.LBA_MAX_LOCAL + 1, "%s: %d free poses" % (name, nfree)
        return
    assert rep[0] == capi.LBA_OK, "%s: status %d" % (name, rep[0])
    assert rep[9] >= 1 and rep[11] >= 1, "%s: a round without a trial" % name
    t = b["tables"]
    moved = any(ref["Tcw"][r].tobytes() != KG._round_trip(t["Tcw"][r]).tobytes() for r in ref["local_kf"][:rep[1]] if r != b["id0_row"])
    assert moved, "%s: no Levenberg-Marquardt step was accepted" % name
    ne = rep[4] + rep[5]
    if name == "pts1100":
        assert rep[3] > CHUNK, "%s: %d local points" % (name, rep[3])
        pos = {int(p): i for i, p in enumerate(ref["local_point"][:rep[3]])}
        late = [row for row in ref["erase"][:rep[7]].tolist() if pos[row[2]] >= CHUNK]
        assert late and len(late) < rep[7], "%s: the erase rows do not come from both chunks" % name
        fixed = ref["fixed_kf"][:rep[2]].tolist()
        assert 8 in fixed and 9 in fixed and min(int(p) for p in range(b["np"]) if any(r in (8, 9) for r, _s in _obs(t, p))) >= CHUNK, \
            "%s: no fixed camera is first seen through the second chunk" % name
    if name == "f40":
        assert nfree > LBA_SETUP_WAVES and nfree * nfree > LBA_SCHUR_WAVES, "%s: %d free poses" % (name, nfree)
    if name == "f128":
        assert nfree == capi.LBA_MAX_LOCAL and rep[1] == nfree + 1, "%s: %d free poses of %d local rows" % (name, nfree, rep[1])
    if name == "e31k":
        assert ne > LBA_ITEMS and rep[3] > LBA_ITEMS, "%s: %d edges, %d points do not pass %d" % (name, ne, rep[3], LBA_ITEMS)


def _obs(t, p):
    return [(int(t["obs_kf"][o]), int(t["obs_idx"][o])) for o in range(int(t["obs_start"][p]), int(t["obs_start"][p + 1]))]


# ---------------------------------------------------------------------------------------------------------------------
# essential graph
EG_CASES = list(REFERENCE["eg"])


def _csr_lists(start, flat, rows):
    return {r: [int(v) for v in flat[start[r]:start[r + 1]]] for r in range(rows) if start[r + 1] > start[r]}


def _eg_ordered(conn_w, good):
    """test_essgraph_cpu._ordered for the rows of `good` only (the other rows have no connection)."""
    rows = len(conn_w)
    ord_kf, ord_w, n_ord = np.zeros((rows, rows), i32), np.zeros((rows, rows), i32), np.zeros(rows, i32)
    for r in good:
        c = np.nonzero(conn_w[r] > 0)[0]
        c = c[np.lexsort((c, -conn_w[r][c]))]
        n_ord[r] = len(c)
        ord_kf[r, :len(c)], ord_w[r, :len(c)] = c, conn_w[r][c]
    return ord_kf, ord_w, n_ord


def eg_embed(b, rows, pos):
    """The graph of case b among `rows` rows: its row k becomes row pos[k], every other row is bad.  Every table is indexed by
    row, so any injective pos gives a valid scene; the order of the vertices becomes that of pos."""
    T, old = b["tables"], b["rows"]
    pos = np.asarray(pos, np.int64)
    to = lambda a: np.where(np.asarray(a) >= 0, pos[np.maximum(np.asarray(a), 0)], -1).astype(i32)  # noqa: E731
    N = {}
    N["kf_bad"] = np.ones(rows, u8)
    N["kf_bad"][pos] = T["kf_bad"]
    N["kf_id"] = (4 * old + np.arange(rows)).astype(i32)
    N["kf_id"][pos] = T["kf_id"]
    N["parent"] = np.full(rows, -1, i32)
    N["parent"][pos] = to(T["parent"])
    N["conn_w"] = np.zeros((rows, rows), i32)
    N["conn_w"][np.ix_(pos, pos)] = T["conn_w"]
    N["ord_kf"], N["ord_w"], N["n_ord"] = _eg_ordered(N["conn_w"], pos.tolist())
    for key in ("loop", "lc"):
        lists = _csr_lists(T[key + "_start"], T[key + "_kf"], old)
        N[key + "_start"], N[key + "_kf"], _ = KE._csr({int(pos[r]): [int(pos[c]) for c in v] for r, v in lists.items()}, rows)
    for key in ("corrected", "non_corrected"):
        N[key] = np.zeros((rows, 8), f64)
        N[key][:, 3] = N[key][:, 7] = 1.0
        N[key][pos] = T[key]
    for key in ("in_corrected", "in_non_corrected"):
        N[key] = np.zeros(rows, u8)
        N[key][pos] = T[key]
    N["Tcw"] = np.tile(np.c_[np.eye(3), np.zeros(3)].reshape(12).astype(f32), (rows, 1))
    N["Tcw"][pos] = T["Tcw"]
    N["flags"], N["world"] = T["flags"], T["world"]
    for key in ("ref_kf", "corrected_by_kf", "corrected_ref"):
        N[key] = to(T[key])
    return dict(b, tables=N, rows=rows, cur=int(pos[b["cur"]]), loop_row=int(pos[b["loop_row"]]), pos=pos)


def _eg_dense(rows, seed):
    """A ring whose rows are all covisible: every pair further apart than three rows has a weight of 100 to 159 (the pairs three
    apart keep theirs, below 100, or GetCovisiblesByWeight would return nothing), three old loop edges, and a third row with
    loop connections."""
    b = KE.ring(rows, seed, band=2, npts=12, loops={20: [4], 4: [20], 33: [9], 9: [33], 41: [17], 17: [41]}, max_edges=2000)
    T, cur = b["tables"], b["cur"]
    rng = np.random.default_rng(seed + 1)
    W = T["conn_w"]
    for a in range(rows):
        for c in range(a - 3):
            if (a, c) not in ((cur, 0), (cur, 1), (cur - 1, 0), (cur - 1, 1)):
                W[a][c] = W[c][a] = 100 + int(rng.integers(0, 60))
    T["ord_kf"], T["ord_w"], T["n_ord"] = KE._ordered(W)
    lc = _csr_lists(T["lc_start"], T["lc_kf"], rows)
    lc[cur - 2] = [0, 2]
    T["lc_start"], T["lc_kf"], _ = KE._csr(lc, rows)
    return b


@functools.lru_cache(maxsize=None)
def eg_case(name):
    if name == "rows1100":
        # a ring of 40 rows among 1100: 19 of them in the first chunk of 1024 rows and 21 in the second; the loop key frame
        # (ring row 0) and the current one (39) in the second chunk, ring row 38 -- the other row with loop connections -- in
        # the first, so both edge passes start the second chunk with a carry
        rng = np.random.default_rng(301)
        b = KE.ring(40, 301, band=2, npts=20, loops={20: [4], 4: [20]})
        lo = rng.choice(CHUNK, 19, replace=False).tolist()
        hi = (CHUNK + rng.choice(1100 - CHUNK, 21, replace=False)).tolist()
        pos = [0] * 40
        pos[0], pos[39], pos[38] = hi.pop(), hi.pop(), lo.pop()
        rest = lo + hi
        for k, r in enumerate(range(1, 38)):
            pos[r] = rest[k]
        return eg_embed(b, 1100, pos)
    if name == "e960":
        return _eg_dense(47, 302)
    if name == "pts1100":
        return KE.ring(8, 303, npts=1100)
    if name == "f150":
        return KE.ring(151, 304, band=2, npts=12, loops={100: [30], 30: [100]}, drift=(0.001, -0.001, 0.0015, 0.004))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def eg_reference(name):
    b = eg_case(name)
    if REFERENCE["eg"][name] == "seqref":
        return KE.as_arrays(b, KE.run_seqref(b))
    got = _in_tmp(lambda d: {k: np.array(v) for k, v in KE.run_host(b, d, name).items()})
    got.pop("tried")
    return got


@functools.lru_cache(maxsize=None)                                               # a case that passed is not checked again
def eg_preconditions(name):
    b, ref = eg_case(name), eg_reference(name)
    T = b["tables"]
    rep = [int(v) for v in ref["report"]]
    ne, nfree = sum(rep[2:6]), rep[1] - 1
    assert rep[0] == capi.EG_OK, "%s: status %d" % (name, rep[0])
    assert rep[9] >= 1, "%s: no trial" % name
    # Scw is the estimate the optimisation starts from (vScw) and Swc the inverse of the one it ends with (vCorrectedSwc)
    good = [r for r in range(b["rows"]) if not T["kf_bad"][r] and r != b["loop_row"]]
    moved = any(np.array(sim3_inverse([float(v) for v in ref["Scw"][r]]), f64).tobytes() != np.ascontiguousarray(ref["Swc"][r]).tobytes() for r in good)
    assert moved, "%s: no Levenberg-Marquardt step was accepted" % name
    if name == "rows1100":
        good = np.nonzero(T["kf_bad"] == 0)[0]
        assert b["rows"] > CHUNK and good.min() < CHUNK <= good.max() and rep[1] == len(good), "%s: the good rows are not in both chunks" % name
        assert b["loop_row"] >= CHUNK, "%s: the loop key frame is in the first chunk" % name
        lc_rows = [r for r in range(b["rows"]) if T["lc_start"][r + 1] > T["lc_start"][r]]
        assert min(lc_rows) < CHUNK <= max(lc_rows) and rep[2] >= 2, "%s: the loop connections do not carry across chunks" % name
    if name == "e960":
        assert ne > EG_TEAMS, "%s: %d edges do not pass the %d teams" % (name, ne, EG_TEAMS)
        assert nfree >= bwd_block1_free(EG_NB, 7), "%s: %d free vertices leave block 1 of k_bwd_upd idle" % (name, nfree)
        assert rep[4] >= 3 and rep[2] >= 4, "%s: %d old loop edges, %d loop connections" % (name, rep[4], rep[2])
    if name == "pts1100":
        present = np.nonzero(T["flags"] & 1)[0]
        assert b["pcap"] > CHUNK and present.max() >= CHUNK and rep[11] == len(present), "%s: no present point in the second chunk" % name
        assert any(ref["world"][p].tobytes() != T["world"][p].tobytes() for p in present if p >= CHUNK), "%s: no point of the second chunk moved" % name
    if name == "f150":
        assert nfree >= 150 and rep[10] == 7 * nfree, "%s: %d free vertices" % (name, nfree)
