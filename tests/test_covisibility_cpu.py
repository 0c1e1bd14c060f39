"""tests/seqref/covisibility.py (KeyFrame::UpdateConnections, AddConnection, UpdateBestCovisibles, GetBestCovisibilityKeyFrames
and the target list of LocalMapping::SearchInNeighbors restated from the reference text) against cases worked by hand, one
per rule; the scenes tests/test_covisibility_gpu.py and tests/test_cpp_covisibility_gpu.py run the kernels on, with a
non-vacuity check computed from seqref alone; the declarations and the argument checks of the C-ABI entries.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

from seqref import covisibility as CV

i32, u8 = np.int32, np.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT = CV.POINT_PRESENT
TABLE_KEYS = ("slot_point", "n", "obs_start", "obs_kf", "flags")
STATE_KEYS = ("conn_w", "ord_kf", "ord_w", "n_ord", "covis", "first_conn", "parent")
SENTINEL = -0x5A5A5A5B
HUB = 4                        # a row the update lists of the scenes never name


# ---- small tables by hand -----------------------------------------------------------------------------------------------------
def tables(rows, cap, obs, flags=None, slots=None, pcap=None):
    """obs[p] = the rows observing point p, in list order.  Every observing row holds the point in its next free slot unless
    slots[r] = the point indices of row r's slots (-1 = none) says otherwise."""
    n_pts = len(obs)
    pcap = n_pts if pcap is None else pcap
    per_row = [[] for _ in range(rows)]
    for p, rs in enumerate(obs):
        for r in dict.fromkeys(rs):
            per_row[r].append(p)
    for r, s in (slots or {}).items():
        per_row[r] = list(s)
    T = dict(slot_point=np.full((rows, cap), -1, i32), n=np.zeros(rows, i32))
    for r, s in enumerate(per_row):
        assert len(s) <= cap
        T["slot_point"][r, :len(s)] = s
        T["n"][r] = len(s)
    T["obs_start"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(i32)
    T["obs_kf"] = np.array([r for o in obs for r in o] + [0], i32)
    T["flags"] = np.zeros(pcap, u8)
    T["flags"][:n_pts] = PRESENT if flags is None else flags
    return T


def shared(rows, pairs, cap=64):
    """Tables in which rows a and b share pairs[(a, b)] points that nobody else observes."""
    obs = []
    for (a, b), k in pairs.items():
        obs += [[a, b]] * k
    return tables(rows, cap, obs)


def update(G, T, rows_list, id0_row=-1, info=None, touched=None):
    rep = CV.update_connections_list(G, rows_list, T["slot_point"], T["n"], T["obs_start"], T["obs_kf"], T["flags"], id0_row, info,
                                     touched)
    return [dict(zip(CV.REPORT_FIELDS, r.tolist())) for r in rep]


def test_counts_of_14_15_16():
    T = shared(4, {(0, 1): 14, (0, 2): 15, (0, 3): 16})
    G = CV.Graph(4)
    rep = update(G, T, [0])[0]
    assert G.ord_kf[0] == [3, 2] and G.ord_w[0] == [16, 15]
    assert G.conn[0] == {1: 14, 2: 15, 3: 16}                    # the whole counter
    assert G.conn[1] == {} and G.ord_kf[1] == []                  # 14 < 15: no AddConnection
    assert G.conn[2] == {0: 15} and G.ord_kf[2] == [0] and G.conn[3] == {0: 16} and G.ord_w[3] == [16]
    assert rep == dict(status=CV.OK, n_voted=3, n_ordered=2, max_row=3, max_votes=16, parent_set=3, n_resorted=2, fallback=0)
    assert G.parent == [3, -1, -1, -1] and G.first_conn == [False, True, True, True]


def test_equal_weights_put_the_higher_row_first():
    T = shared(4, {(0, 1): 15, (0, 3): 15, (0, 2): 16})
    G = CV.Graph(4)
    update(G, T, [0])
    assert G.ord_kf[0] == [2, 3, 1] and G.ord_w[0] == [16, 15, 15]
    assert G.dense()["covis"][0].tolist() == [2, 3, 1] + [-1] * 7


def test_fallback_with_two_equal_maxima_takes_the_lower_row():
    T = shared(4, {(0, 2): 3, (0, 1): 3, (0, 3): 2}, cap=16)
    G = CV.Graph(4)
    info = {}
    rep = update(G, T, [0], info=info)[0]
    assert G.ord_kf[0] == [1] and G.ord_w[0] == [3] and G.conn[0] == {1: 3, 2: 3, 3: 2}
    assert G.conn[1] == {0: 3} and G.conn[2] == {} and G.conn[3] == {}
    assert (rep["fallback"], rep["max_row"], rep["max_votes"], rep["n_resorted"], rep["n_ordered"]) == (1, 1, 3, 1, 1)
    assert info["fallback_to_max"] == 1


def test_empty_counter_leaves_first_conn_set_and_writes_nothing():
    T = tables(3, 4, [[0], [0], [1, 2]])                          # row 0 observes only points nobody else sees
    G = CV.Graph(3)
    G.conn[0], G.ord_kf[0], G.ord_w[0] = {2: 5}, [2], [5]
    info = {}
    rep = update(G, T, [0], info=info)[0]
    assert rep == dict(status=CV.EMPTY, n_voted=0, n_ordered=1, max_row=-1, max_votes=0, parent_set=-1, n_resorted=0, fallback=0)
    assert G.first_conn[0] and G.parent[0] == -1 and G.conn[0] == {2: 5} and G.ord_kf[0] == [2]
    assert info == dict(own_row_skip=2, empty_counter=1)


def test_row_repeated_in_an_observation_list_counts_each_time():
    T = tables(3, 4, [[0, 1, 1], [0, 1, 2, 2, 2]])
    G = CV.Graph(3)
    update(G, T, [0])
    assert G.conn[0] == {1: 3, 2: 3} and G.ord_kf[0] == [1]       # fallback, the lower of the equal maxima


def test_empty_slot_and_bad_point_do_not_count():
    T = tables(3, 8, [[0, 1], [0, 1], [0, 2], [0, 2]], flags=[PRESENT, 0, PRESENT, PRESENT], slots={0: [0, -1, 1, 2, -1, 3]})
    G = CV.Graph(3)
    info = {}
    update(G, T, [0], info=info)
    assert G.conn[0] == {1: 1, 2: 2} and G.ord_kf[0] == [2] and info["empty_slot"] == 2 and info["bad_point"] == 1


def test_the_asymmetry_of_the_own_row():
    """Row c = 0 is updated and keeps its weight-3 entry in conn_w but not in ord_kf; a later update of r = 1 with a changed
    weight re-sorts row 0 from the full map and brings the entry in; one with an equal weight leaves the row alone."""
    pairs = {(0, 1): 15, (0, 2): 3}
    G = CV.Graph(3)
    update(G, shared(3, pairs), [0])
    assert G.conn[0] == {1: 15, 2: 3} and G.ord_kf[0] == [1] and G.ord_w[0] == [15]
    pairs[(0, 1)] = 16
    T = shared(3, pairs)
    info = {}
    rep = update(G, T, [1], info=info)[0]
    assert G.conn[0] == {1: 16, 2: 3} and G.ord_kf[0] == [1, 2] and G.ord_w[0] == [16, 3]
    assert rep["n_resorted"] == 1 and info["resort"] == 1 and "equal_weight_return" not in info
    G.ord_kf[0], G.ord_w[0] = [7, 7, 7], [9, 9, 9]                # marks: an untouched row keeps them
    info = {}
    rep = update(G, T, [1], info=info)[0]
    assert G.ord_kf[0] == [7, 7, 7] and G.ord_w[0] == [9, 9, 9] and rep["n_resorted"] == 0 and info["equal_weight_return"] == 1


def test_update_list_a_b_a():
    T = shared(3, {(0, 1): 20, (1, 2): 15, (0, 2): 2})
    G = CV.Graph(3)
    info = {}
    rep = update(G, T, [0, 1, 0], id0_row=0, info=info)
    assert [r["n_resorted"] for r in rep] == [1, 1, 0]           # 0 connects 1; 1 connects 2 (0 has 20 already); nothing new
    assert [r["parent_set"] for r in rep] == [-1, 0, -1]
    assert G.ord_kf == [[1], [0, 2], [1]] and G.ord_w == [[20], [20, 15], [15]]
    assert G.conn[0] == {1: 20, 2: 2} and G.conn[2] == {1: 15}   # row 2 never ran UpdateConnections: no entry for row 0
    assert info["equal_weight_return"] == 2 and info["id0_row"] == 2 and info["first_connection"] == 1
    # the same result as three single calls
    H = CV.Graph(3)
    for r in (0, 1, 0):
        update(H, T, [r], id0_row=0)
    assert all(np.array_equal(G.dense()[k], H.dense()[k]) for k in STATE_KEYS)


def test_the_id0_row_never_gets_a_parent():
    T = shared(2, {(0, 1): 15})
    G = CV.Graph(2)
    rep = update(G, T, [0, 1, 0], id0_row=0)
    assert G.parent == [-1, 0] and G.first_conn == [True, False] and [r["parent_set"] for r in rep] == [-1, 0, -1]


def _graph_with_lists(rows, lists):
    G = CV.Graph(rows)
    for r, l in lists.items():
        G.ord_kf[r], G.ord_w[r] = list(l), list(range(100, 100 - len(l), -1))
        G.conn[r] = dict(zip(G.ord_kf[r], G.ord_w[r]))
    return G


def test_target_lists():
    G = _graph_with_lists(8, {0: [1, 2, 3], 1: [4, 0, 2, 5], 2: [4, 1, 6], 3: [7]})
    bad = np.zeros(8, u8)
    info = {}
    # 1: appended and stamped; its seconds 4, (0 = cur), 2, (5 cut by nn2 = 3).  2: not stamped, appended; 4 again, 1 stamped, 6.
    assert CV.fuse_targets(G, 0, 3, 3, bad, info) == [1, 4, 2, 2, 4, 6, 3, 7]
    assert info == dict(second_is_cur=1, second_bad_or_stamped=1)
    bad[2] = 1                                                    # a bad first neighbour is skipped, and so is a bad second
    info = {}
    assert CV.fuse_targets(G, 0, 10, 5, bad, info) == [1, 4, 5, 3, 7]
    assert info == dict(second_is_cur=1, second_bad_or_stamped=1, first_bad_or_stamped=1, fewer_than_nn=1)
    assert CV.covisible_targets(G, [0, 1, 5], 3, 0, bad) == [[1, 2, 3], [4, 0, 2], []]       # verbatim: bad rows stay
    assert CV.covisible_targets(G, [0], 10, 0) == [[1, 2, 3]]


def test_children_of_a_bad_rows_parent():
    parent = np.array([-1, 0, 0, 1, 0, 1], i32)
    bad = np.array([0, 0, 1, 0, 0, 0], u8)
    start, child = CV.children_from_parents(parent, bad)
    assert start.tolist() == [0, 2, 4, 4, 4, 4, 4] and child.tolist() == [1, 4, 3, 5]      # 2 erased itself from row 0
    start, child = CV.children_from_parents(parent, None)
    assert start.tolist() == [0, 3, 5, 5, 5, 5, 5] and child.tolist() == [1, 2, 4, 3, 5]


# ---- the scenes of the GPU tests ----------------------------------------------------------------------------------------------
def random_scene(rows, seed, npts=300, cap=64, obs_lo=2, obs_hi=12, obs_lengths=None, hub=False):
    """`rows` bank rows of `cap` slots and about `npts` points in arrays of npts + 20.  A point is observed by rows near a
    centre among the first min(rows, 24) rows, so neighbouring rows share 15 points and more, and now and then by a far
    row; a few lists name a row twice; a tenth of the points is bad; every row has some empty slots; the last active row
    holds nothing and row 1 (when there are 30 rows or more) only points of its own.  obs_lengths: every list has one of
    these lengths instead (rows repeat where the bank is smaller).  hub: row HUB starts with an entry for every other row in
    conn_w, weights 1-4, so its re-sort has rows - 1 keys with many ties.  Returns (tables, state, update_rows, id0_row)."""
    rng = np.random.default_rng(seed)
    active = min(rows, 24)
    own_row = 1 if rows >= 30 else -1
    point_rows = []
    for p in range(npts):
        k = int(rng.integers(obs_lo, obs_hi + 1)) if obs_lengths is None else int(obs_lengths[p % len(obs_lengths)])
        centre = int(rng.integers(0, active))
        near = [(centre + d) % active for d in range(-4, 5)]
        rs = [int(x) for x in rng.permutation(list(dict.fromkeys(near)))[:min(k, active)]]
        if rows > active and rng.random() < 0.3:
            rs.append(int(rng.integers(active, rows)))
        while len(rs) < k and obs_lengths is not None:
            rs.append(int(rng.integers(0, rows)))                 # repeats: the list is longer than the bank is wide
        if p % 29 == 0 and rs:
            rs.append(rs[0])                                      # a row named twice
        rs = [r for r in rs if r != own_row and r != active - 1] if rows >= 4 else rs
        point_rows.append(rs)
    if own_row >= 0:
        point_rows += [[own_row]] * 5
    n_pts = len(point_rows)
    pcap = n_pts + 20
    per_row = [[] for _ in range(rows)]
    for p, rs in enumerate(point_rows):
        for r in dict.fromkeys(rs):
            if len(per_row[r]) < cap - 4:
                per_row[r].append(p)
    T = dict(slot_point=np.full((rows, cap), -1, i32), n=np.zeros(rows, i32))
    for r in range(rows):
        s = per_row[r] + [-1] * (1 + r % 4)
        T["slot_point"][r, :len(s)] = rng.permutation(np.array(s, i32))
        T["n"][r] = len(s)
    T["obs_start"] = np.concatenate([[0], np.cumsum([len(rs) for rs in point_rows])]).astype(i32)
    T["obs_kf"] = np.array([r for rs in point_rows for r in rs] + [0], i32)
    T["flags"] = np.zeros(pcap, u8)
    T["flags"][:n_pts] = PRESENT
    T["flags"][rng.choice(n_pts, n_pts // 10, replace=False)] = 0
    T.update(rows=rows, cap=cap, np=n_pts, pcap=pcap)
    G = CV.Graph(rows)
    if hub and rows > 1:
        G.conn[HUB] = {c: int(rng.integers(1, 5)) for c in range(rows) if c != HUB}
    fill = dict(ord_kf=np.full((rows, rows), SENTINEL, i32), ord_w=np.full((rows, rows), SENTINEL, i32),
                covis=np.full((rows, 10), SENTINEL, i32))
    state = G.dense(fill)
    return T, state, G


def run_reference(T, state, update_rows, id0_row=-1, info=None):
    """seqref on dense state arrays: the new state, the report and the set of rows whose lists were rewritten.  A rewrite
    stores the new list and the head; entries behind it and the rows nobody rewrote keep what they held."""
    G = CV.Graph.from_dense(state)
    G.mirror = {k: np.array(state[k], i32).copy() for k in ("ord_kf", "ord_w", "covis")}
    touched = set()
    rep = CV.update_connections_list(G, update_rows, T["slot_point"], T["n"], T["obs_start"], T["obs_kf"], T["flags"], id0_row, info,
                                     touched)
    return G.dense(), rep, touched


_CACHE = {}


def scene_and_reference(name):
    """The named scene, its update list and seqref's answer, computed once and shared; nobody writes to them."""
    if name not in _CACHE:
        kind, rows = name
        if kind == "random":
            T, state, _ = random_scene(rows, 100 + rows, hub=rows >= 65)
            upd = [r % rows for r in (2, 0, 3, 2, 7, 1, 23, rows - 1)]
        elif kind == "strides":
            T, state, _ = random_scene(rows, 7, npts=60, obs_lengths=(17, 33))
            upd = [0, 5, 0]
        else:
            raise KeyError(name)
        id0 = 0 if rows > 1 else -1
        info = {}
        out, rep, touched = run_reference(T, state, upd, id0, info)
        for a in list(T.values()) + list(state.values()) + list(out.values()) + [rep]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = dict(T=T, state=state, upd=np.array(upd, i32), id0=id0, out=out, report=rep, touched=touched, info=info)
    return _CACHE[name]


def test_random_scene_takes_every_branch():
    T, state, G = random_scene(40, 11)
    assert T["rows"] == 40 and T["cap"] == 64 and 290 <= T["np"] <= 320
    lens = np.diff(T["obs_start"])[:300]
    assert lens.min() >= 1 and lens.max() <= 13
    info = {}
    upd = list(range(40)) + [3, 2, 5]
    out, rep, touched = run_reference(T, state, upd, 0, info)
    for key in ("empty_slot", "bad_point", "own_row_skip", "empty_counter", "fallback_to_max", "equal_weight_return", "resort",
                "first_connection", "id0_row", "not_first_connection"):
        assert info.get(key, 0) > 0, (key, info)
    assert (rep[:, 4] >= CV.TH).sum() >= 10 and (rep[:, 2] >= 3).sum() >= 8          # thresholds reached, lists of three and more
    G2 = CV.Graph.from_dense(out)
    bad = np.zeros(40, u8)
    bad[[4, 9]] = 1
    info = {}
    lists = CV.covisible_targets(G2, range(40), 10, 5, bad, info)
    for key in ("first_bad_or_stamped", "second_bad_or_stamped", "second_is_cur", "fewer_than_nn"):
        assert info.get(key, 0) > 0, (key, info)
    assert any(len(l) != len(set(l)) for l in lists)              # a second neighbour came twice
    assert max(len(l) for l in lists) > 10


def test_gpu_scenes_are_not_vacuous():
    for rows in (2, 63, 64, 65, 257):
        S = scene_and_reference(("random", rows))
        assert (S["report"][:, 0] == CV.OK).any() and len(S["touched"]) >= 2, rows
    S = scene_and_reference(("random", 1))
    assert (S["report"][:, 0] == CV.EMPTY).all() and not S["touched"]
    for rows in (65, 257):                                         # the hub: a list of rows - 1 entries with ties
        S = scene_and_reference(("random", rows))
        assert HUB in S["touched"] and HUB not in S["upd"] and S["out"]["n_ord"][HUB] == rows - 1
        w = S["out"]["ord_w"][HUB, :rows - 1]
        assert (np.diff(w) == 0).sum() > rows // 2
    S = scene_and_reference(("random", 64))
    assert (S["report"][:, 7] == 1).any() and (S["report"][:, 7] == 0).any() and (S["report"][:, 0] == CV.EMPTY).any()
    assert S["info"].get("equal_weight_return", 0) > 0
    S = scene_and_reference(("strides", 40))
    lens = np.diff(S["T"]["obs_start"])
    assert {17, 33} <= set(lens.tolist()) and (S["report"][:, 4] >= CV.TH).all()


# ---- C ABI without a device ---------------------------------------------------------------------------------------------------
def c_records(capi, T, S):
    rt, rs = capi.CovisTables(), capi.CovisState()
    for k in TABLE_KEYS:
        setattr(rt, k, capi.ptr(T[k]).value)
    for k in STATE_KEYS:
        setattr(rs, k, capi.ptr(S[k]).value)
    return rt, rs


def test_covisibility_entries_exist_and_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device.  The entries are exported with the declared signatures; the host entries
    check counts, pointers and every range before they look at the handle, so with a null handle each violation is refused
    with ORBHIP_E_ARG and named by orbhip_last_error without touching HIP, the state or the outputs, and valid arguments
    reach the handle check (ORBHIP_E_ARG, no message of a range check).  The checks against a live handle are in
    tests/test_covisibility_gpu.py."""
    from orb_slam2_comment_amd import capi
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("orbhip_update_connections", "orbhip_update_connections_device", "orbhip_covisible_targets",
                 "orbhip_covisible_targets_device", "orbhip_children_from_parents_device"):
        assert name in names
    assert (capi.CONNECTIONS_OK, capi.CONNECTIONS_EMPTY) == (CV.OK, CV.EMPTY) == (0, 1)
    assert capi.CONNECTIONS_REPORT == CV.REPORT_FIELDS and capi.POINT_PRESENT == PRESENT
    assert tuple(k for k, _ in capi.CovisTables._fields_) == TABLE_KEYS
    assert tuple(k for k, _ in capi.CovisState._fields_) == STATE_KEYS
    L = capi.lib()
    T0 = shared(3, {(0, 1): 2, (1, 2): 1}, cap=4)
    S0 = CV.Graph(3).dense()
    S0["ord_kf"][0, :2], S0["n_ord"][0], S0["ord_kf"][1, :1], S0["n_ord"][1] = [1, 2], 2, [2], 1
    upd0, rep0 = np.array([1, 0], i32), np.full((2, 8), SENTINEL, i32)

    def update(m=None, rows=3, cap=4, n=3, pcap=3, id0=-1, U=2, upd=upd0, T=T0, S=S0, device=False):
        rt, rs = c_records(capi, T, S)
        fn = L.orbhip_update_connections_device if device else L.orbhip_update_connections
        return fn(m, rows, cap, n, pcap, C.byref(rt), C.byref(rs), id0, U, capi.ptr(upd), capi.ptr(rep0))

    def last():
        return (L.orbhip_last_error() or b"").decode()

    def changed(A, key, index, value):
        B = dict(A)
        B[key] = np.array(A[key]).copy()
        B[key][index] = value
        return B
    before = {k: np.array(a).copy() for k, a in list(T0.items()) + list(S0.items())}
    for device in (False, True):
        for kw in (dict(rows=-1), dict(n=-1), dict(n=4, pcap=3), dict(cap=0), dict(U=-1), dict(id0=3), dict(id0=-2), dict(upd=None), {}):
            assert update(device=device, **kw) == capi.E_ARG, (device, kw)
        assert update(device=device, rows=4097) == capi.E_CAPACITY and "4096" in last()
        assert update(device=device, cap=4097) == capi.E_CAPACITY
    for case, word in ((dict(upd=np.array([1, 3], i32)), "list entry 1"), (dict(upd=np.array([-1, 0], i32)), "list entry 0"),
                       (dict(T=changed(T0, "obs_kf", 1, 3)), "observation 1"), (dict(T=changed(T0, "obs_kf", 0, -1)), "observation 0"),
                       (dict(T=changed(T0, "slot_point", (1, 0), 3)), "point index"),
                       (dict(T=changed(T0, "slot_point", (0, 1), -2)), "point index"),
                       (dict(T=changed(T0, "obs_start", 1, 5)), "non-decreasing"), (dict(T=changed(T0, "obs_start", 0, -1)), "below 0"),
                       (dict(T=changed(T0, "n", 2, 5)), "bank row 2"), (dict(T=changed(T0, "n", 0, -1)), "bank row 0"),
                       (dict(S=changed(S0, "n_ord", 1, 4)), "n_ord of bank row 1")):
        assert update(**case) == capi.E_ARG and word in last(), (list(case), word, last())
    assert np.array_equal(rep0, np.full((2, 8), SENTINEL, i32))
    assert all(np.array_equal(before[k], a) for k, a in list(T0.items()) + list(S0.items()))

    targets, counts = np.full((2, 4), SENTINEL, i32), np.full(2, SENTINEL, i32)
    cur0 = np.array([0, 1], i32)

    def target_lists(rows=3, Q=2, nn=2, nn2=1, cur=cur0, S=S0, device=False, ord_kf=True):
        fn = L.orbhip_covisible_targets_device if device else L.orbhip_covisible_targets
        return fn(None, rows, capi.ptr(S["ord_kf"]) if ord_kf else None, capi.ptr(S["n_ord"]), None, Q, capi.ptr(cur), nn, nn2,
                  capi.ptr(targets), capi.ptr(counts))
    for device in (False, True):
        for kw in (dict(rows=-1), dict(Q=-1), dict(nn=0), dict(nn2=-1), dict(nn=4097), dict(ord_kf=False), {}):
            assert target_lists(device=device, **kw) == capi.E_ARG, (device, kw)
        assert target_lists(device=device, rows=4097) == capi.E_CAPACITY
    for case, word in ((dict(cur=np.array([0, 3], i32)), "a current row"), (dict(S=changed(S0, "ord_kf", (0, 1), 3)), "a first neighbour"),
                       (dict(S=changed(S0, "ord_kf", (1, 0), -1)), "a second neighbour"),
                       (dict(S=changed(S0, "n_ord", 0, 4)), "n_ord of bank row 0")):
        assert target_lists(**case) == capi.E_ARG and word in last(), (list(case), word, last())
    assert (targets == SENTINEL).all() and (counts == SENTINEL).all()
    par = np.zeros(3, i32)
    assert L.orbhip_children_from_parents_device(None, 3, capi.ptr(par), None, capi.ptr(par), capi.ptr(par)) == capi.E_ARG
    assert L.orbhip_children_from_parents_device(None, 4097, capi.ptr(par), None, capi.ptr(par), capi.ptr(par)) == capi.E_CAPACITY
    assert L.orbhip_children_from_parents_device(None, 3, None, None, capi.ptr(par), capi.ptr(par)) == capi.E_ARG


def test_mirrors_declare_the_covisibility_interface():
    import orb_slam2_comment_amd as pkg
    methods = ("UpdateConnections", "UpdateConnectionsDevice", "CovisibleTargets", "CovisibleTargetsDevice",
               "ChildrenFromParentsDevice")
    for name in methods:
        assert callable(getattr(pkg.ORBmatcher, name))
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for sym in ("ORBHIP_CONNECTIONS_OK    0", "ORBHIP_CONNECTIONS_EMPTY 1"):
        assert "#define " + sym in hdr
    for name in ("orbhip_update_connections_device", "orbhip_update_connections", "orbhip_covisible_targets_device",
                 "orbhip_covisible_targets", "orbhip_children_from_parents_device"):
        assert "int %s(" % name in hdr
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for name in methods:
        assert "void %s(" % name in hpp
    mk = open(os.path.join(ROOT, "orb_slam2_comment_amd", "csrc", "Makefile")).read()
    assert "orbhip_covisibility.hip" in mk


if __name__ == "__main__":
    for name_ in [("random", r) for r in (1, 2, 63, 64, 65, 257)] + [("strides", 40)]:
        S_ = scene_and_reference(name_)
        print(name_, S_["report"].tolist(), sorted(S_["touched"]), S_["info"])
