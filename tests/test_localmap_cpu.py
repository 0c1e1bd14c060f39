"""tests/seqref/localmap.py (Tracking::UpdateLocalKeyFrames, UpdateLocalPoints and the bookkeeping of SearchLocalPoints restated
from the reference text) against cases worked by hand, one per rule; the scenes tests/test_localmap_gpu.py and
tests/test_cpp_localmap_gpu.py run the kernels on, with a non-vacuity check computed from seqref alone; the declarations and
the argument checks of the C-ABI entries.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

import test_seqref_projection_cpu as PC
from seqref import localmap as LM
from seqref import matcher as SM
from seqref import projection as P

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT, OBSERVED = P.POINT_PRESENT, P.POINT_OBSERVED
GOOD = PRESENT | OBSERVED
KEY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                      ("class_id", "<i4")])
TABLE_KEYS = ("slot_point", "n", "kf_bad", "covis", "child_start", "child", "parent", "obs_start", "obs_kf", "flags", "world",
              "normal", "max_dist", "min_dist", "point_desc")
VIEW_COS, TH, NNRATIO = 0.5, 1.0, 0.8          # src/Tracking.cc:1175, :1185, :1184


# ---- small tables by hand -----------------------------------------------------------------------------------------------------
def tables(rows, cap, slots, obs, flags=None, kf_bad=(), covis=None, children=None, parent=None, pcap=None):
    """slots[r] = the point indices of row r's slots (-1 = none); obs[p] = the rows observing point p, in list order."""
    n_pts = len(obs)
    pcap = n_pts if pcap is None else pcap
    T = {}
    T["slot_point"] = np.full((rows, cap), -1, np.int32)
    T["n"] = np.zeros(rows, np.int32)
    for r, s in (slots.items() if isinstance(slots, dict) else enumerate(slots)):
        T["slot_point"][r, :len(s)] = s
        T["n"][r] = len(s)
    T["kf_bad"] = np.zeros(rows, np.uint8)
    T["kf_bad"][list(kf_bad)] = 1
    T["covis"] = np.full((rows, 10), -1, np.int32)
    for r, c in (covis or {}).items():
        T["covis"][r, :len(c)] = c
    ch = [list((children or {}).get(r, ())) for r in range(rows)]
    T["child_start"] = np.concatenate([[0], np.cumsum([len(c) for c in ch])]).astype(np.int32)
    T["child"] = np.array([x for c in ch for x in c], np.int32)
    T["parent"] = np.full(rows, -1, np.int32)
    for r, p in (parent or {}).items():
        T["parent"][r] = p
    T["obs_start"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    T["obs_kf"] = np.array([r for o in obs for r in o], np.int32)
    T["flags"] = np.zeros(pcap, np.uint8)
    T["flags"][:n_pts] = GOOD if flags is None else flags
    idx = np.arange(pcap, dtype=f32)
    T["world"] = np.stack([idx, idx + f32(0.5), idx + f32(0.25)], 1)
    T["normal"] = np.stack([-idx, idx * f32(2), idx + f32(7)], 1)
    T["max_dist"], T["min_dist"] = idx + f32(100), idx + f32(1)
    T["point_desc"] = (np.arange(pcap * 32) % 251).astype(np.uint8).reshape(pcap, 32)
    return T


def run(T, frame_points, prev=None):
    """seqref on one or more frames given as lists of point indices; prev[f] = the previous local key-frame list."""
    frames, rows = len(frame_points), len(T["n"])
    cap = max([T["slot_point"].shape[1]] + [len(fp) for fp in frame_points])
    fp = np.full((frames, cap), -1, np.int32)
    for f, a in enumerate(frame_points):
        fp[f, :len(a)] = a
    lk = np.full((frames, rows), -1, np.int32)
    nlk = np.zeros(frames, np.int32)
    for f, a in enumerate(prev or []):
        lk[f, :len(a)] = a
        nlk[f] = len(a)
    return LM.update_local_map(T, fp, [len(a) for a in frame_points], lk, nlk)


def report(R, f=0):
    return dict(zip(LM.REPORT_FIELDS, R["report"][f].tolist()))


def test_tie_in_votes_goes_to_the_lower_row_and_a_larger_count_later_wins():
    T = tables(4, 4, [[], [0], [1], [2]], obs=[[1, 2], [2, 1], [3, 3, 3]])
    R = run(T, [[0, 1]])
    assert R["votes"][0].tolist() == [0, 2, 2, 0] and report(R)["ref_row"] == 1 and report(R)["ref_votes"] == 2
    R = run(T, [[0, 1, 2]])                                       # row 3 repeated three times in one list: counted each time
    assert R["votes"][0].tolist() == [0, 2, 2, 3] and report(R)["ref_row"] == 3 and report(R)["ref_votes"] == 3
    assert R["local_kf"][0].tolist() == [1, 2, 3] and report(R)["status"] == LM.OK


def test_bad_row_with_the_most_votes_is_neither_reference_nor_listed():
    T = tables(3, 4, [[0], [1], [2]], obs=[[0, 1, 2], [0, 1], [0]], kf_bad=[0])
    R = run(T, [[0, 1, 2]])
    rep = report(R)
    assert R["votes"][0].tolist() == [3, 2, 1] and R["local_kf"][0].tolist() == [1, 2]
    assert (rep["status"], rep["n_voted"], rep["n_local_kf"], rep["ref_row"], rep["ref_votes"]) == (LM.OK, 3, 2, 1, 2)
    assert R["local_point"][0].tolist() == [1, 2]                # row 0's point is not local


def test_all_voted_rows_bad():
    T = tables(3, 4, [[0], [0], [1]], obs=[[0, 1], [2]], kf_bad=[0, 1])
    R = run(T, [[0]], prev=[[2]])
    rep = report(R)
    assert (rep["status"], rep["n_voted"], rep["n_local_kf"], rep["ref_row"], rep["ref_votes"], rep["walk_end"]) == \
        (LM.ALL_BAD, 2, 0, -1, 0, LM.WALK_EXHAUSTED)
    assert len(R["local_kf"][0]) == 0 and len(R["local_point"][0]) == 0          # the list was cleared (:1259)


def test_no_votes_keeps_the_old_list_and_rebuilds_the_points_from_it():
    T = tables(3, 4, [[0, 1], [2], [3, 0]], obs=[[0, 2], [0], [1], [2]])
    for frame in ([], [-1, -1]):
        R = run(T, [frame], prev=[[2, 0]])
        rep = report(R)
        assert (rep["status"], rep["n_voted"], rep["n_local_kf"], rep["ref_row"]) == (LM.NO_VOTES, 0, 2, -1)
        assert R["local_kf"][0].tolist() == [2, 0] and R["local_point"][0].tolist() == [3, 0, 1]
    T["flags"][0] = OBSERVED                                      # the only frame point is bad: nulled, nobody votes
    R = run(T, [[0]], prev=[[2, 0]])
    assert report(R)["status"] == LM.NO_VOTES and R["frame_point"][0, 0] == -1 and R["local_point"][0].tolist() == [3, 1]


def test_covisible_skipped_when_stamped_or_bad_and_second_child_taken():
    T = tables(6, 4, [[0], [0], [], [], [], []], obs=[[0, 1]], kf_bad=[2], covis={0: [1, 2, 3, 4], 1: [0, 3]},
               children={0: [1, 4, 5]}, parent={1: 0})
    R = run(T, [[0]])
    assert R["local_kf"][0].tolist() == [0, 1, 3, 4] and report(R)["walk_end"] == LM.WALK_EXHAUSTED
    assert report(R)["n_local_kf"] == 4


def test_a_bad_parent_is_still_appended():
    T = tables(6, 4, [[0]] + [[]] * 5, obs=[[0]], kf_bad=[5], parent={0: 5})
    R = run(T, [[0]])
    assert R["local_kf"][0].tolist() == [0, 5] and report(R)["walk_end"] == LM.WALK_PARENT


def test_parents_break_ends_the_walk_not_the_visit():
    T = tables(6, 4, [[0], [0], [0], [], [], []], obs=[[0, 1, 2]], covis={0: [5], 1: [4]}, parent={0: 3})
    R = run(T, [[0]])
    assert R["local_kf"][0].tolist() == [0, 1, 2, 5, 3] and report(R)["walk_end"] == LM.WALK_PARENT      # 4 never added
    T["parent"][0] = 1                                            # a stamped parent does not break
    R = run(T, [[0]])
    assert R["local_kf"][0].tolist() == [0, 1, 2, 5, 4] and report(R)["walk_end"] == LM.WALK_EXHAUSTED


def test_the_80_limit():
    T = tables(100, 2, [[0]] * 100, obs=[list(range(85))], covis={0: [90]})
    R = run(T, [[0]])
    assert report(R)["walk_end"] == LM.WALK_LIMIT and report(R)["n_local_kf"] == 85 and 90 not in R["local_kf"][0]
    # 79 voted rows: visits 0 and 1 run at sizes 79 and 80 and append; visit 2 meets 81 > 80
    T = tables(100, 2, [[0]] * 100, obs=[list(range(79))], covis={r: [79 + r] for r in range(79)})
    R = run(T, [[0]])
    assert R["local_kf"][0].tolist() == list(range(81)) and report(R)["walk_end"] == LM.WALK_LIMIT


def test_point_in_two_slots_of_one_row_is_listed_once():
    T = tables(2, 4, [[1, 0, 1, 2], [2, 0, 3]], obs=[[0, 1], [0, 0], [0, 1], [1]])
    R = run(T, [[3]], prev=[[]])
    assert R["local_kf"][0].tolist() == [1] and R["local_point"][0].tolist() == [2, 0, 3]
    R = run(T, [[0]])
    assert R["local_kf"][0].tolist() == [0, 1] and R["local_point"][0].tolist() == [1, 0, 2, 3] and R["met"][0] == 7


def test_bad_frame_point_is_nulled_and_does_not_vote():
    T = tables(3, 4, [[0], [1], [1]], obs=[[0], [1, 2]], flags=[GOOD, OBSERVED])
    R = run(T, [[1, 0, -1]])
    assert R["frame_point"][0, :3].tolist() == [-1, 0, -1] and R["votes"][0].tolist() == [1, 0, 0]
    assert R["local_kf"][0].tolist() == [0] and R["taken"][0, :3].tolist() == [0, 1, 0]


def test_frame_held_point_gets_flag_zero_and_taken_follows_observed():
    T = tables(2, 4, [[0, 1, 2, 3], [3, 2]], obs=[[0], [0], [0, 1], [0, 1]], flags=[GOOD, PRESENT, PRESENT, GOOD])
    R = run(T, [[1, -1, 3]])
    assert R["local_point"][0].tolist() == [0, 1, 2, 3]
    assert R["flags_l"][0].tolist() == [GOOD, 0, PRESENT, 0]
    assert R["taken"][0, :3].tolist() == [0, 0, 1]               # point 1 is held but nobody observes it: the slot stays open
    w, nrm, mx, mn, d = LM.gather(T, R["local_point"][0])
    assert np.array_equal(w, T["world"][:4]) and np.array_equal(d, T["point_desc"][:4]) and mx.tolist() == [100, 101, 102, 103]


# ---- the scenes of the GPU tests -------------------------------------------------------------------------------------------------
SENTINEL = -0x5A5A5A5B


def _finish(S, rng, rows, cap, npts, pcap, point_rows, bad_rows, bad_points):
    """Tables from point_rows[p] = the rows observing p: every observation takes a slot of its row (a few points take two
    slots of their first row), the slots of a row are shuffled among some empty ones."""
    per_row = [[] for _ in range(rows)]
    for p, rs in enumerate(point_rows):
        for r in rs:
            per_row[r].append(p)
        if p % 37 == 0 and len(rs):
            per_row[rs[0]].append(p)
    S["slot_point"] = np.full((rows, cap), -1, np.int32)
    S["n"] = np.zeros(rows, np.int32)
    for r in range(rows):
        s = per_row[r] + [-1] * min(cap - len(per_row[r]), 3 + r % 13)
        assert len(s) <= cap
        S["slot_point"][r, :len(s)] = rng.permutation(np.array(s, np.int32))
        S["n"][r] = len(s)
    S["obs_start"] = np.concatenate([[0], np.cumsum([len(rs) for rs in point_rows])]).astype(np.int32)
    S["obs_kf"] = np.array([r for rs in point_rows for r in rs] + [0], np.int32)
    S["kf_bad"] = np.zeros(rows, np.uint8)
    S["kf_bad"][list(bad_rows)] = 1
    flags = np.zeros(pcap, np.uint8)
    flags[:npts] = PRESENT | (rng.random(npts) < 0.85) * OBSERVED
    flags[list(bad_points)] &= ~np.uint8(PRESENT)
    S["flags"] = flags
    S.update(rows=rows, cap=cap, np=npts, pcap=pcap)
    return S


def _graph(S, rows, covis, children, parent):
    S["covis"] = np.full((rows, 10), -1, np.int32)
    for r, c in covis.items():
        S["covis"][r, :len(c)] = c
    ch = [list(children.get(r, ())) for r in range(rows)]
    S["child_start"] = np.concatenate([[0], np.cumsum([len(c) for c in ch])]).astype(np.int32)
    S["child"] = np.array([x for c in ch for x in c] + [0], np.int32)
    S["parent"] = np.full(rows, -1, np.int32)
    for r, p in parent.items():
        S["parent"][r] = p


def _random_point_arrays(S, rng, pcap):
    S["world"] = rng.normal(0, 8, (pcap, 3)).astype(f32)
    S["normal"] = rng.normal(0, 1, (pcap, 3)).astype(f32)
    S["max_dist"] = rng.uniform(5, 50, pcap).astype(f32)
    S["min_dist"] = (S["max_dist"] / f32(3.58)).astype(f32)
    S["point_desc"] = rng.integers(0, 256, (pcap, 32), dtype=np.uint8)


def scene_a(seed=5):
    """12 rows, cap 256, about 150 slots per row, 400 points in arrays of 512, rows 3 and 9 bad, about 10 % bad points, two
    current frames of 150 and 140 key points with poses, key points and descriptors.  Point p is anchored to key point
    (p // 2) % frame_n of frame p % 2: it projects onto it at the key point's octave and carries its descriptor with a few
    bits flipped, so the search has something to find and several points compete for one key point.  Points anchored to
    frame 1 are observed by rows 0-6 only, so frame 1's walk has rows left to add."""
    rows, cap, npts, pcap, frames = 12, 256, 400, 512, 2
    rng = np.random.default_rng(seed)
    cam, scam = PC.make_cam()
    S = dict(cam=cam, scam=scam, frames=frames, frame_n=np.array([150, 140], np.int32))
    bad_points = rng.choice(npts, npts // 10, replace=False)
    point_rows = []
    for p in range(npts):
        allowed = np.arange(rows) if p % 2 == 0 else np.arange(7)
        point_rows.append(rng.choice(allowed, rng.integers(2, 7), replace=False).tolist())
    _finish(S, rng, rows, cap, npts, pcap, point_rows, (3, 9), bad_points)
    parent = {r: int(rng.choice([x for x in range(r) if x not in (3, 9)])) for r in range(1, rows)}     # no bad parents
    children = {}
    for r, p in parent.items():
        children.setdefault(p, []).append(r)
    _graph(S, rows, {r: rng.permutation(np.delete(np.arange(rows), r))[:rng.integers(3, 11)].tolist() for r in range(rows)},
           children, parent)
    # the current frames
    T0 = PC.pose(rng, small=False)
    S["T"] = [T0, (PC.pose(rng).astype(f64) @ T0.astype(f64)).astype(f32)]
    keys = np.zeros((frames, cap), KEY_DTYPE)
    keys["x"], keys["y"] = rng.uniform(10, PC.W - 10, (frames, cap)), rng.uniform(10, PC.H - 10, (frames, cap))
    keys["octave"], keys["angle"], keys["size"] = rng.integers(0, 8, (frames, cap)), rng.uniform(0, 360, (frames, cap)), 31
    S["keys"], S["desc"] = keys, rng.integers(0, 256, (frames, cap, 32), dtype=np.uint8)
    _random_point_arrays(S, rng, pcap)
    for p in range(npts):
        f = p % 2
        k = (p // 2) % int(S["frame_n"][f])
        T = S["T"][f]
        X = PC.back_project(np.array([keys["x"][f, k], keys["y"][f, k]], f64) + rng.normal(0, 0.4, 2), rng.uniform(2, 30, 1), T)[0]
        Ow = -(T[:3, :3].astype(f64).T @ T[:3, 3].astype(f64))
        d = X.astype(f64) - Ow
        dist = np.linalg.norm(d)
        S["world"][p], S["normal"][p] = X, (d / dist).astype(f32)
        S["max_dist"][p] = f32(dist * float(PC.SF[keys["octave"][f, k]]) * 0.97)
        S["min_dist"][p] = f32(S["max_dist"][p] / PC.SF[7])
        bits = np.unpackbits(S["desc"][f, k])
        bits[rng.choice(256, rng.integers(0, 7), replace=False)] ^= 1
        S["point_desc"][p] = np.packbits(bits)
    fp = np.full((frames, cap), -1, np.int32)
    for f in range(frames):
        for k in range(int(S["frame_n"][f])):
            if rng.random() < 0.55:
                fp[f, k] = 2 * k + f                              # the first point anchored to this key point
    S["frame_point"] = fp
    S["local_kf"] = np.full((frames, rows), -1, np.int32)
    S["n_local_kf"] = np.zeros(frames, np.int32)
    return S


def scene_b(seed=6):
    """96 rows of cap 64, no parents.  Frame 0 holds points that 90 rows observe: the limit stops the walk at its first
    visit.  Frame 1's points are observed by rows 0-69 only, and every row has an unvoted covisible and an unvoted child, so
    the walk runs until the size passes 80."""
    rows, cap, npts, pcap, frames = 96, 64, 600, 640, 2
    rng = np.random.default_rng(seed)
    S = dict(frames=frames, frame_n=np.array([64, 60], np.int32))
    point_rows = []
    for p in range(npts):
        allowed, lo = (np.arange(90), 4) if p % 2 == 0 else (np.arange(70), 1)
        point_rows.append(rng.choice(allowed, rng.integers(lo, lo + 5), replace=False).tolist())
    _finish(S, rng, rows, cap, npts, pcap, point_rows, (10, 75), rng.choice(npts, 50, replace=False))
    _graph(S, rows, {r: [(r + 1) % 70, 70 + (r * 7) % 26, 70 + (r * 11 + 3) % 26] for r in range(70)},
           {r: [(r + 2) % 70, 70 + (r * 5 + 1) % 26] for r in range(70)}, {})
    _random_point_arrays(S, rng, pcap)
    fp = np.full((frames, cap), -1, np.int32)
    for f in range(frames):
        fp[f, :S["frame_n"][f]] = rng.choice(np.arange(f, npts, 2), int(S["frame_n"][f]), replace=False)
    S["frame_point"] = fp
    S["local_kf"] = np.full((frames, rows), -1, np.int32)
    S["n_local_kf"] = np.zeros(frames, np.int32)
    return S


def scene_c(seed=7):
    """20 rows of cap 64, three frames.  Frame 0: the second visited row has an unvoted parent, the break leaves later rows
    unvisited.  Frame 1 holds nothing but bad points: no votes, the previous list (which names a row with n = 0) stays.
    Frame 2's points are observed by bad rows only."""
    rows, cap, npts, pcap, frames = 20, 64, 120, 128, 3
    rng = np.random.default_rng(seed)
    S = dict(frames=frames, frame_n=np.array([20, 9, 12], np.int32))
    point_rows = []
    for p in range(npts):
        if p < 80:
            allowed = np.array([1, 2, 4, 5, 6, 8])
        elif p < 100:
            allowed = np.array([12, 13])                          # the bad rows
        else:
            allowed = np.array([9, 10, 14, 15, 16])
        point_rows.append(rng.choice(allowed, rng.integers(1, len(allowed) + 1), replace=False).tolist())
    bad_points = list(range(60, 70))
    _finish(S, rng, rows, cap, npts, pcap, point_rows, (12, 13), bad_points)
    assert S["n"][17] > 0
    S["n"][17] = 0                                               # a listed row without slots
    _graph(S, rows, {1: [2, 4, 3], 2: [1, 7], 4: [18], 5: [19]}, {1: [2, 11], 5: [0]}, {1: 2, 2: 17, 4: 3})
    _random_point_arrays(S, rng, pcap)
    fp = np.full((frames, cap), -1, np.int32)
    fp[0, :20] = rng.choice(60, 20, replace=False)
    fp[1, :9] = rng.choice(bad_points, 9, replace=False)
    fp[2, :12] = rng.choice(np.arange(80, 100), 12, replace=False)
    S["frame_point"] = fp
    S["local_kf"] = np.full((frames, rows), -1, np.int32)
    S["n_local_kf"] = np.array([0, 4, 2], np.int32)
    S["local_kf"][1, :4] = [15, 17, 9, 14]
    S["local_kf"][2, :2] = [1, 2]
    return S


SCENES = dict(A=scene_a, B=scene_b, C=scene_c)
_CACHE = {}


def scene_and_reference(name):
    """The scene and seqref's answer for it, computed once and shared; nobody writes to them."""
    if name not in _CACHE:
        S = SCENES[name]()
        R = LM.update_local_map(S, S["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"], pcap=S["pcap"])
        for a in list(S.values()) + [R["frame_point"], R["votes"], R["taken"], R["report"]]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = (S, R)
    return _CACHE[name]


def search_chain(S, R, f, reverse=False):
    """The two existing halves of SearchLocalPoints from seqref for frame f of scene A: frustum queries of the gathered local
    points, the points search against the current frame, and the assignment applied.  reverse: the local list backwards.
    Returns (q, assign, nmatches, frame_point)."""
    pts, fl = R["local_point"][f], R["flags_l"][f]
    if reverse:
        pts, fl = pts[::-1], fl[::-1]
    w, nrm, mx, mn, d = LM.gather(S, pts)
    q, _ = P.frustum_queries(S["scam"], S["T"][f], w, nrm, mx, mn, fl, VIEW_COS, TH)
    nf = int(S["frame_n"][f])
    F = SM.Frame(S["keys"][f, :nf], S["desc"][f, :nf], None, PC.BOUNDS, PC.SF)
    nm, assign = SM.search_by_projection_points(F, q, d, R["taken"][f, :nf], nnratio=NNRATIO)
    return q, assign, nm, LM.apply_assignment(R["frame_point"][f, :nf], pts, assign)


def track_reference():
    """search_chain for both frames of scene A, computed once."""
    if "track" not in _CACHE:
        S, R = scene_and_reference("A")
        _CACHE["track"] = [search_chain(S, R, f) for f in range(S["frames"])]
    return _CACHE["track"]


def test_scenes_are_not_vacuous():
    statuses, ends = set(), set()
    for name in SCENES:
        S, R = scene_and_reference(name)
        for f in range(S["frames"]):
            rep = report(R, f)
            statuses.add(rep["status"])
            ends.add(rep["walk_end"])
            assert rep["n_local_points"] == len(R["local_point"][f]) <= S["np"] and rep["n_local_kf"] == len(R["local_kf"][f])
            assert len(set(R["local_kf"][f].tolist())) == len(R["local_kf"][f])
    assert statuses == {LM.OK, LM.NO_VOTES, LM.ALL_BAD} and ends == {LM.WALK_EXHAUSTED, LM.WALK_LIMIT, LM.WALK_PARENT}
    S, R = scene_and_reference("A")
    assert 130 <= S["n"].mean() <= 170 and (S["flags"][:S["np"]] & PRESENT == 0).sum() == 40
    for f in range(2):
        n_local = len(R["local_point"][f])
        assert n_local > 250 and R["met"][f] - n_local >= R["met"][f] // 4          # the de-duplication drops a quarter
        assert (R["flags_l"][f] == 0).sum() * 10 >= n_local                          # a tenth is frame-held
        assert (R["frame_point"][f] != S["frame_point"][f]).sum() >= 3               # bad frame points were nulled
        assert report(R, f)["status"] == LM.OK
    assert report(R, 0)["walk_end"] == LM.WALK_EXHAUSTED and report(R, 0)["n_voted"] == 12 and report(R, 0)["n_local_kf"] == 10
    assert report(R, 1)["n_local_kf"] > report(R, 1)["n_voted"]                      # frame 1's walk added rows
    S, R = scene_and_reference("B")
    assert report(R, 0)["walk_end"] == LM.WALK_LIMIT and report(R, 0)["n_local_kf"] > 81      # stopped at its first visit
    assert report(R, 1)["walk_end"] == LM.WALK_LIMIT and report(R, 1)["n_local_kf"] == 81 and report(R, 1)["n_voted"] <= 70
    S, R = scene_and_reference("C")
    assert [report(R, f)["status"] for f in range(3)] == [LM.OK, LM.NO_VOTES, LM.ALL_BAD]
    assert report(R, 0)["walk_end"] == LM.WALK_PARENT and R["local_kf"][0].tolist()[-1] == 17 and 18 not in R["local_kf"][0]
    assert R["local_kf"][1].tolist() == [15, 17, 9, 14] and len(R["local_point"][1]) > 10 and (R["frame_point"][1] == -1).all()
    assert len(R["local_kf"][2]) == 0 and len(R["local_point"][2]) == 0


def test_the_order_of_the_local_list_is_visible_in_the_search():
    S, R = scene_and_reference("A")
    total = 0
    for f, (q, assign, nm, fp) in enumerate(track_reference()):
        assert q["valid"].sum() > 100 and nm >= (assign >= 0).sum() > 40      # nmatches counts a stolen key point twice
        _, _, nm_r, fp_r = search_chain(S, R, f, reverse=True)
        total += int((fp != fp_r).sum())
    assert total >= 5                                             # another order, another owner of some key points


# ---- C ABI without a device -------------------------------------------------------------------------------------------------------
def c_records(capi, T, io):
    rt, rio = capi.LocalMapTables(), capi.LocalMapIO()
    for k in TABLE_KEYS:
        if T.get(k) is not None:
            setattr(rt, k, capi.ptr(T[k]).value)
    for k, a in io.items():
        setattr(rio, k, capi.ptr(a).value)
    return rt, rio


def sentinel_io(frames, rows, cap, pcap, frame_point=None, frame_n=None, local_kf=None, n_local_kf=None):
    i32 = np.int32
    pat = np.array([SENTINEL], i32).view(f32)[0]
    return dict(frame_point=np.full((frames, cap), -1, i32) if frame_point is None else np.array(frame_point, i32, order="C"),
                frame_n=np.zeros(frames, i32) if frame_n is None else np.array(frame_n, i32),
                local_kf=np.full((frames, rows), SENTINEL, i32) if local_kf is None else np.array(local_kf, i32, order="C"),
                n_local_kf=np.zeros(frames, i32) if n_local_kf is None else np.array(n_local_kf, i32),
                votes=np.full((frames, rows), SENTINEL, i32), local_point=np.full((frames, pcap), SENTINEL, i32),
                world_l=np.full((frames, pcap, 3), pat, f32), normal_l=np.full((frames, pcap, 3), pat, f32),
                max_dist_l=np.full((frames, pcap), pat, f32), min_dist_l=np.full((frames, pcap), pat, f32),
                desc_l=np.full((frames, pcap, 32), 0xA5, np.uint8), flags_l=np.full((frames, pcap), 0xA5, np.uint8),
                np_l=np.full(frames, SENTINEL, i32), taken=np.full((frames, cap), 0xA5, np.uint8),
                report=np.full((frames, 8), SENTINEL, i32))


def test_local_map_entries_exist_and_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device: the entries are exported with the declared signatures and refuse a null
    handle and bad counts with ORBHIP_E_ARG without touching HIP or the outputs.  The checks against a live handle are in
    tests/test_localmap_gpu.py."""
    from orb_slam2_comment_amd import capi
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("orbhip_update_local_map", "orbhip_update_local_map_device", "orbhip_track_local_map_device"):
        assert name in names
    assert (capi.LOCALMAP_OK, capi.LOCALMAP_NO_VOTES, capi.LOCALMAP_ALL_BAD) == (LM.OK, LM.NO_VOTES, LM.ALL_BAD) == (0, 1, 2)
    assert (capi.LOCALMAP_WALK_EXHAUSTED, capi.LOCALMAP_WALK_LIMIT, capi.LOCALMAP_WALK_PARENT) == \
        (LM.WALK_EXHAUSTED, LM.WALK_LIMIT, LM.WALK_PARENT) == (0, 1, 2)
    assert (capi.POINT_PRESENT, capi.POINT_OBSERVED) == (PRESENT, OBSERVED)
    assert tuple(k for k, _ in capi.LocalMapTables._fields_) == TABLE_KEYS
    L = capi.lib()
    T = tables(2, 4, [[0], [0]], obs=[[0, 1]])
    io = sentinel_io(1, 2, 4, 1, frame_point=[[0, -1, -1, -1]], frame_n=[1])
    before = {k: a.copy() for k, a in io.items()}
    rt, rio = c_records(capi, T, io)
    cam = PC.make_cam()[0]
    tr = capi.LocalMapTrack()

    def calls(m, frames=1, rows=2, cap=4, n=1, pcap=1):
        return (L.orbhip_update_local_map(m, frames, rows, cap, n, pcap, C.byref(rt), C.byref(rio)),
                L.orbhip_update_local_map_device(m, frames, rows, cap, n, pcap, C.byref(rt), C.byref(rio)),
                L.orbhip_track_local_map_device(m, frames, rows, cap, n, pcap, C.byref(rt), C.byref(rio), C.byref(cam), C.byref(tr),
                                                0.5, 1.0, 0.8))
    for kw in ({}, dict(frames=-1), dict(rows=-1), dict(n=-1), dict(n=2, pcap=1), dict(cap=0), dict(frames=0)):
        assert calls(None, **kw) == (capi.E_ARG,) * 3, kw
    assert L.orbhip_update_local_map_device(None, 1, 2, 4, 1, 1, None, C.byref(rio)) == capi.E_ARG
    assert L.orbhip_update_local_map_device(None, 1, 2, 4, 1, 1, C.byref(rt), None) == capi.E_ARG
    assert all(np.array_equal(io[k].view(np.uint8), before[k].view(np.uint8)) for k in io)


def test_mirrors_declare_the_local_map_interface():
    import orb_slam2_comment_amd as pkg
    for name in ("UpdateLocalMap", "UpdateLocalMapDevice", "TrackLocalMapDevice"):
        assert callable(getattr(pkg.ORBmatcher, name))
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for sym in ("ORBHIP_LOCALMAP_OK       0", "ORBHIP_LOCALMAP_NO_VOTES 1", "ORBHIP_LOCALMAP_ALL_BAD  2",
                "ORBHIP_LOCALMAP_WALK_EXHAUSTED 0", "ORBHIP_LOCALMAP_WALK_LIMIT     1", "ORBHIP_LOCALMAP_WALK_PARENT    2"):
        assert "#define " + sym in hdr
    for name in ("orbhip_update_local_map_device", "orbhip_track_local_map_device", "orbhip_update_local_map"):
        assert "int %s(" % name in hdr
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for name in ("UpdateLocalMap", "UpdateLocalMapDevice", "TrackLocalMapDevice"):
        assert "void %s(" % name in hpp


if __name__ == "__main__":
    for name_ in SCENES:
        S_, R_ = scene_and_reference(name_)
        print(name_, R_["report"].tolist(), [len(a) for a in R_["local_point"]], R_["met"])
