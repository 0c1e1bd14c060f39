"""Scenes that take the map-maintenance entries (covisibility, local map, culling) to the bank sizes the product runs them at;
shared by test_map_scale_cpu.py and test_map_scale_gpu.py.  The scenes of test_covisibility_cpu.py, test_localmap_cpu.py and
test_culling_cpu.py were sized for the sequential reference: at most 257 bank rows of 64 slots, every vote in the first 24 rows.
Here the generators place votes, ties, full rows and children where a case needs them, in bulk; random_scene, cull_scene,
run_reference's protocol, reference_key_frames, reference_map_points, _finish, _graph and sentinel_io are those of the three
modules.  The reference is tests/seqref throughout, byte for byte: everything here is integer or bitwise work.

Every case lists the thresholds it must cross (CROSSES); preconditions(name) asserts them on the reference's report, info and
arrays alone, so a later change of a grid size shows up as a failed precondition and not as a silently shrunken test."""
import functools

import numpy as np

import test_covisibility_cpu as CC
import test_culling_cpu as KC
import test_localmap_cpu as LC
from seqref import covisibility as CV
from seqref import culling as CU
from seqref import localmap as LM

i32, u8, f32 = np.int32, np.uint8, np.float32
SENTINEL = CC.SENTINEL

# ---------------------------------------------------------------------------------------------------------------------
# The kernel-private sizes the cases are built around.  Each names its source line; test_map_scale_cpu.py reads them back.
WG = 256                    # __launch_bounds__(256) of every kernel but k_cv_targets and the walks: rows, slots or positions per pass
WAVE = 64                   # wave64: the chunk of k_cv_targets' ballot loop, of the child loop of k_lm_keyframes, of kf_reparent
GROUP = 16                  # orbhip_covisibility.hip:19 kCvGroup, orbhip_localmap.hip:22 kLmGroup, orbhip_culling.hip:28 kCuGroup
CV_MAX_ROWS = 4096          # orbhip_covisibility.hip:20 kCvMaxRows: the LDS histogram, the LDS sort keys, the stamp bitset
CU_MAX_ROWS = 4096          # orbhip_culling.hip:29 kCuMaxRows
CV_BLOCK_SLOTS, CV_MAX_BLOCKS = 128, 8    # orbhip_covisibility.hip:268 slot_blocks = max(1, min(8, (cap + 127) / 128))
CU_BLOCK_SLOTS, CU_MAX_BLOCKS = 256, 16   # orbhip_culling.hip:465 slot_blocks = max(1, min(16, (cap + 255) / 256))
CV_TH = 15                  # orbhip_covisibility.hip:21 kCvTh
LM_POS_BLOCKS = 1024        # orbhip_localmap.hip:25 kLmPosBlocks: list positions per pass of k_lm_first / k_lm_points
LM_MAX_KF = 80              # orbhip_localmap.hip:23 kLmMaxKf
LM_MAX_ROWS = 65536         # orbhip_localmap.hip:26 kLmStampWords = 65536 / 32
UPD_LONG_BLOCKS = 1024      # orbhip_matcher.hip:2342 kUpdLongBlocks: worklist entries per pass of k_update_points_long
UPD_GROUP = 16              # orbhip_matcher.hip:2340 kUpdGroup: a longer list is a long point


def cv_slot_blocks(cap):
    return max(1, min(CV_MAX_BLOCKS, (cap + CV_BLOCK_SLOTS - 1) // CV_BLOCK_SLOTS))


def cu_slot_blocks(cap):
    return max(1, min(CU_MAX_BLOCKS, (cap + CU_BLOCK_SLOTS - 1) // CU_BLOCK_SLOTS))


def sort_size(rows):
    """N of k_cv_apply / k_kf_apply: the power of two at or above rows, at least 2."""
    N = 2
    while N < rows:
        N <<= 1
    return N


def where(row):
    """(pass, wavefront, lane) of the thread that meets bank row `row` in a loop of 256 rows per pass."""
    return row // WG, row % WG // WAVE, row % WAVE


# what every case must cross; test_map_scale_cpu.py asserts that every threshold below is named by at least one case
THRESHOLDS = ("cv_counter_blocks_2", "cv_counter_blocks_clamped", "cv_tie_across_waves", "cv_tie_across_passes", "cv_tie_across_lanes",
              "cv_tie_in_fallback", "cv_sort_above_512", "cv_sort_4096", "cv_own_row_above_256", "cv_row_slot_subset",
              "cv_targets_copy_above_64", "cv_targets_second_above_64", "cv_targets_second_above_256", "cv_children_4096",
              "cv_children_across_passes", "lm_votes_stride", "lm_rows_above_256", "lm_rows_above_1024", "lm_tie_across_waves",
              "lm_tie_across_passes", "lm_tie_across_lanes", "lm_children_above_64", "lm_last_stamp_word", "lm_row_above_256_slots", "lm_row_above_512_slots", "lm_cap_4096", "lm_scan_above_256",
              "cu_decide_above_256", "cu_erase_blocks", "cu_sort_1024", "cu_sort_4096", "cu_reparent_above_320", "cu_reparent_last_word",
              "upd_long_above_1024")
CROSSES = dict(
    cv_blocks2=("cv_counter_blocks_2",),
    cv_blocks8=("cv_counter_blocks_clamped", "cv_tie_across_waves", "cv_tie_across_passes", "cv_tie_across_lanes", "cv_tie_in_fallback",
                "cv_sort_above_512", "cv_own_row_above_256", "cv_row_slot_subset", "cv_targets_copy_above_64",
                "cv_targets_second_above_64", "cv_targets_second_above_256"),
    cv_wide=("cv_own_row_above_256",),
    cv_full4096=("cv_sort_4096", "cv_counter_blocks_clamped", "cv_targets_copy_above_64"),
    children=("cv_children_4096", "cv_children_across_passes"),
    lm_rows1100=("lm_votes_stride", "lm_rows_above_256", "lm_rows_above_1024", "lm_tie_across_waves", "lm_tie_across_passes",
                 "lm_tie_across_lanes", "lm_children_above_64", "lm_row_above_256_slots", "lm_row_above_512_slots", "lm_scan_above_256"),
    lm_cap4096=("lm_cap_4096", "lm_row_above_512_slots"),
    lm_rows65536=("lm_last_stamp_word",),
    cu_rows1100=("cu_decide_above_256", "cu_erase_blocks", "cu_sort_1024", "cu_reparent_above_320"),
    cu_full4096=("cu_sort_4096", "cu_reparent_last_word", "cu_reparent_above_320"),
    upd_long=("upd_long_above_1024",))
CASES = list(CROSSES)


def _freeze(*dicts):
    for d in dicts:
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


# ---------------------------------------------------------------------------------------------------------------------
# covisibility
def graph_from_dense(A):
    """CV.Graph.from_dense with the weight maps taken through np.nonzero (test_map_scale_cpu.py pins the two to each other):
    the loop over rows x rows entries of the original is what 4096 rows cost."""
    rows = len(A["n_ord"])
    G = CV.Graph(rows)
    cw = np.asarray(A["conn_w"]).reshape(rows, rows)
    rr, cc = np.nonzero(cw)
    ww = cw[rr, cc]
    cut = np.searchsorted(rr, np.arange(rows + 1))
    for r in np.unique(rr).tolist():
        a, b = cut[r], cut[r + 1]
        G.conn[r] = dict(zip(cc[a:b].tolist(), ww[a:b].tolist()))
    n_ord = np.asarray(A["n_ord"])
    for r in np.nonzero(n_ord)[0].tolist():
        k = int(n_ord[r])
        G.ord_kf[r] = np.asarray(A["ord_kf"][r][:k]).tolist()
        G.ord_w[r] = np.asarray(A["ord_w"][r][:k]).tolist()
    G.first_conn = [bool(x) for x in np.asarray(A["first_conn"]).tolist()]
    G.parent = np.asarray(A["parent"]).tolist()
    return G


def run_reference(T, state, update_rows, id0_row=-1, info=None):
    """CC.run_reference with graph_from_dense."""
    G = graph_from_dense(state)
    G.mirror = {k: np.array(state[k], i32).copy() for k in ("ord_kf", "ord_w", "covis")}
    touched = set()
    rep = CV.update_connections_list(G, update_rows, T["slot_point"], T["n"], T["obs_start"], T["obs_kf"], T["flags"], id0_row, info,
                                     touched)
    return G.dense(), rep, touched


def cv_tables(rows, cap, designs, seed, hub=None):
    """designs: (r, counts, width) with counts = {k: c}: bank row r shares exactly c good points with row k.  A point of the
    design is seen by r and by up to `width` of the rows that still lack points, the neediest first, so the rows of one counter
    are spread over the slots of r (and with them over the workgroups of k_cv_counters); r stands at a varying place of the list.
    Every observer holds the point; a row's slots are shuffled among a few empty ones; behind each design come five bad points
    seen by r and its highest-count rows, which would move a maximum if they counted.  hub: a row that starts with an entry
    for every other row in conn_w (weights 1-4); its lists start empty, as in random_scene(hub=True), and its first re-sort
    brings all the entries in.  Returns (tables, state)."""
    rng = np.random.default_rng(seed)
    point_rows, bad_points = [], []
    for r, counts, width in designs:
        ks = np.array(sorted(counts), np.int64)
        rem = np.array([counts[int(k)] for k in ks], np.int64)
        assert r not in counts and rem.min() > 0
        while rem.max() > 0:
            idx = np.argsort(-rem, kind="stable")[:width]
            idx = np.sort(idx[rem[idx] > 0])
            rem[idx] -= 1
            rs = ks[idx].tolist()
            rs.insert(len(point_rows) % (len(rs) + 1), r)
            point_rows.append(rs)
        top = sorted(counts, key=lambda k: (-counts[k], -k))[:2]
        for _ in range(5):
            bad_points.append(len(point_rows))
            point_rows.append([r] + top)
    n_pts = len(point_rows)
    pcap = n_pts + 20
    per_row = [[] for _ in range(rows)]
    for p, rs in enumerate(point_rows):
        for r in rs:
            per_row[r].append(p)
    T = dict(slot_point=np.full((rows, cap), -1, i32), n=np.zeros(rows, i32))
    for r in range(rows):
        if per_row[r]:
            s = np.array(per_row[r] + [-1] * (1 + r % 4), i32)
            assert len(s) <= cap, "row %d needs %d slots" % (r, len(s))
            T["slot_point"][r, :len(s)] = rng.permutation(s)
            T["n"][r] = len(s)
    T["obs_start"] = np.concatenate([[0], np.cumsum([len(rs) for rs in point_rows])]).astype(i32)
    T["obs_kf"] = np.array([r for rs in point_rows for r in rs] + [0], i32)
    T["flags"] = np.zeros(pcap, u8)
    T["flags"][:n_pts] = CC.PRESENT
    T["flags"][bad_points] = 0
    T.update(rows=rows, cap=cap, np=n_pts, pcap=pcap)
    G = CV.Graph(rows)
    if hub is not None:
        G.conn[hub] = {c: int(rng.integers(1, 5)) for c in range(rows) if c != hub}
    fill = dict(ord_kf=np.full((rows, rows), SENTINEL, i32), ord_w=np.full((rows, rows), SENTINEL, i32),
                covis=np.full((rows, 10), SENTINEL, i32))
    return T, G.dense(fill)


# the rows of cv_blocks8 that are updated, and the rows whose counts are tied at the maximum of each (where() of each in the comment)
B8 = dict(rows=1100, cap=2048,
          A=5, A_TIE=(200, 516),           # 200: pass 0, wavefront 3; 516: pass 2, wavefront 0 -- the lower row in the higher wavefront
          B=6, B_TIE=(300, 522, 556),      # 300 and 556: lane 44 of wavefront 0, passes 1 and 2; 522: lane 10 of wavefront 0, pass 2
          C=7, C_TIE=(700, 1030),          # the fallback: nobody reaches 15; 700: pass 2, wavefront 2; 1030: pass 4, wavefront 0
          H=8, H2=9,                       # the rows of the host entry: they and their voters are 72 rows of the 1100
          UPD=[5, 6, 7, 8, 200, 5, 1099, 9, 0], HOST_UPD=[8, 9, 8])
W_HUB = 77                                 # cv_wide: the updated row
F_HUB, F_UPD = 4, [10, 4095, 2000]         # cv_full4096: the row with 4095 entries, and the update list


def _cv_blocks8():
    rng = np.random.default_rng(802)
    voters = list(range(10, B8["rows"]))

    def design(lo, hi, tie, top):
        c = {k: int(rng.integers(lo, hi)) for k in voters}
        c.update({k: top for k in tie})
        return c
    designs = [(B8["A"], design(8, 23, B8["A_TIE"], 40), 10), (B8["B"], design(8, 23, B8["B_TIE"], 41), 10),
               (B8["C"], design(6, 9, B8["C_TIE"], 9), 6),
               (B8["H"], {10 + 27 * i: int(rng.integers(20, 60)) for i in range(40)}, 1),
               (B8["H2"], {12 + 31 * i: int(rng.integers(10, 40)) for i in range(31)}, 1)]
    return cv_tables(B8["rows"], B8["cap"], designs, 803)


def _cv_wide():
    """Row 77 of 330 shares 15 + k % 6 points with each of the rows 0 .. 319 but itself, and 14 with the rest."""
    counts = {k: 15 + k % 6 for k in range(320) if k != W_HUB}
    counts.update({k: 14 for k in range(320, 330)})
    return cv_tables(330, 768, [(W_HUB, counts, 8)], 804)


def _cv_full4096():
    """4096 rows of 1024 slots.  Row 10 shares 15 to 30 points with 600 rows spread over the bank, the hub and row 4095 among
    them; row 4095 is updated too (its voters: 300 rows), and row 2000 (a voter of both) after them."""
    rng = np.random.default_rng(805)
    v10 = sorted(set(rng.choice(np.arange(11, 4095), 598, replace=False).tolist()) - {2000}) + [F_HUB, 2000, 4095]
    v4095 = sorted(set(rng.choice(np.arange(11, 4095), 299, replace=False).tolist()) - {2000}) + [2000]
    designs = [(10, {k: int(rng.integers(15, 31)) for k in v10}, 16), (4095, {k: int(rng.integers(10, 25)) for k in v4095}, 8)]
    return cv_tables(4096, 1024, designs, 806, hub=F_HUB)


@functools.lru_cache(maxsize=None)
def cv_case(name):
    """dict(T, state, upd, id0, out, report, touched, info): the layout of CC.scene_and_reference."""
    if name == "cv_blocks2":
        T, state, _ = CC.random_scene(65, 801, npts=300, cap=256, hub=True)
        upd, id0 = [2, 0, 3, 2, 7, 1, 23, 64], 0
    elif name == "cv_blocks8":
        (T, state), upd, id0 = _cv_blocks8(), B8["UPD"], 0
    elif name == "cv_blocks8_host":
        S = cv_case("cv_blocks8")
        T, state, upd, id0 = S["T"], S["state"], B8["HOST_UPD"], 0
    elif name == "cv_wide":
        (T, state), upd, id0 = _cv_wide(), [W_HUB, 3], 0
    elif name == "cv_full4096":
        (T, state), upd, id0 = _cv_full4096(), F_UPD, 0
    else:
        raise KeyError(name)
    info = {}
    out, rep, touched = run_reference(T, state, upd, id0, info)
    _freeze(T, state, out, dict(rep=rep))
    return dict(T=T, state=state, upd=np.array(upd, i32), id0=id0, out=out, report=rep, touched=touched, info=info)


def _report(S, u):
    return dict(zip(CV.REPORT_FIELDS, S["report"][u].tolist()))


def _voters_by_block(T, r, blocks):
    """For updated row r: per counter workgroup of k_cv_counters (slot i belongs to workgroup i / 16 % blocks), the set of rows
    its slots vote for."""
    sets = [set() for _ in range(blocks)]
    for i in range(int(T["n"][r])):
        p = int(T["slot_point"][r, i])
        if p >= 0 and T["flags"][p] & CC.PRESENT:
            sets[i // GROUP % blocks].update(int(k) for k in T["obs_kf"][T["obs_start"][p]:T["obs_start"][p + 1]] if k != r)
    return sets


def cv_resident_rows(T, upd):
    """The rows the host entry keeps on the device: the updated rows and the rows their good points' lists name."""
    res = set(int(r) for r in upd)
    for r in set(int(r) for r in upd):
        for i in range(int(T["n"][r])):
            p = int(T["slot_point"][r, i])
            if p >= 0 and T["flags"][p] & CC.PRESENT:
                res.update(int(k) for k in T["obs_kf"][T["obs_start"][p]:T["obs_start"][p + 1]])
    return res


def _tied_maximum(S, u, row, tie, fallback):
    """Entry u updates `row`; its counter (conn_w of the row afterwards, :367) has its maximum at exactly the rows of `tie`."""
    rep, cw = _report(S, u), S["out"]["conn_w"][row]
    assert int(S["upd"][u]) == row and sorted(np.nonzero(cw == cw.max())[0].tolist()) == sorted(tie), (row, np.nonzero(cw == cw.max())[0])
    assert rep["max_row"] == min(tie) and rep["max_votes"] == cw.max() and rep["fallback"] == fallback, rep
    assert (cw.max() < CV_TH) == bool(fallback)


def _filled(T, r):
    return int((T["slot_point"][r, :T["n"][r]] >= 0).sum())


# the readers on the updated graphs: (case, nn, nn2, current rows)
TARGET_CASES = [("cv_blocks8", 100, 0), ("cv_blocks8", 4096, 0), ("cv_blocks8", 10, 70), ("cv_blocks8", 3, 300),
                ("cv_full4096", 100, 0), ("cv_full4096", 4096, 0), ("cv_full4096", 10, 70), ("cv_full4096", 3, 300)]


def target_rows(case):
    if case == "cv_blocks8":
        return np.array([B8["A"], B8["B"], B8["C"], 200, 516, 1099, 0, 37, B8["H"]], i32)
    return np.array([F_HUB, 10, 4095, 2000, 0], i32)


def target_bad(case):
    rows = cv_case(case)["T"]["rows"]
    bad = np.zeros(rows, u8)
    bad[[3, 9, 300, 1000]] = 1
    return bad


@functools.lru_cache(maxsize=None)
def target_reference(case, nn, nn2):
    S = cv_case(case)
    info = {}
    G = graph_from_dense(S["out"])
    lists = CV.covisible_targets(G, target_rows(case), nn, nn2, target_bad(case), info)
    return lists, info, G


def target_preconditions(case, nn, nn2):
    """The lists the readers are asked for are longer than a wavefront where the case says so."""
    lists, info, G = target_reference(case, nn, nn2)
    cur = target_rows(case)
    if nn2 == 0:
        assert max(len(l) for l in lists) > WAVE and max(len(G.ord_kf[c]) for c in cur) > min(nn, 4 * WAVE), (case, nn)
        return
    bad = target_bad(case)
    firsts = [k for c in cur for k in G.ord_kf[c][:nn] if not bad[k]]
    longest = max(len(G.ord_kf[k]) for k in firsts)
    assert nn2 > WAVE and longest > (WG if nn2 > WG else WAVE), (case, nn, nn2, longest)
    assert max(len(l) for l in lists) > nn2 and info.get("second_is_cur", 0) > 0 and info.get("second_bad_or_stamped", 0) > 0, (case, info)


# ChildrenFromParentsDevice: name -> (parent, kf_bad)
CHILD_P, CHILD_LAST = 1500, 4000


@functools.lru_cache(maxsize=None)
def children_case(name):
    if name == "rows4096":
        # parent 1500 has 790 rows, every fifth from 100 to 4045 (passes 0 to 15), 71 of them bad: 719 children; the rows between them are
        # children of 40 other parents, of row 4000 (a parent of the last pass) or of nobody; a tenth of all rows is bad
        rows = 4096
        rng = np.random.default_rng(807)
        others = rng.choice(rows, 40, replace=False)
        parent = np.where(rng.random(rows) < 0.8, others[rng.integers(0, 40, rows)], -1).astype(i32)
        parent[rng.choice(rows, 300, replace=False)] = CHILD_LAST
        parent[100:4050:5] = CHILD_P
        bad = (rng.random(rows) < 0.1).astype(u8)
    elif name == "rows1025":
        rows = 1025
        parent, bad = np.zeros(rows, i32), np.zeros(rows, u8)
        parent[0] = -1
    else:
        raise KeyError(name)
    start, child = CV.children_from_parents(parent, bad)
    _freeze(dict(a=parent, b=bad, c=start, d=child))
    return dict(rows=rows, parent=parent, bad=bad, start=start, child=child)


# ---------------------------------------------------------------------------------------------------------------------
# local map
# the rows tied at the maximum of frame 0; row 200 is the reference row.  200 and 456: lane 8 of wavefront 3, passes 0 and 1 (the
# in-thread rule); 203: lane 11 of wavefront 3, and 453: lane 5 of it, pass 1 -- a higher row in a lower lane (the __shfl_xor
# merge); 516: wavefront 0, pass 2 -- the lower row in the higher wavefront (the cross-wave merge)
LM_TIE = (200, 203, 453, 456, 516)
LM_FAT = (600, 900)         # the rows with more than 256 and more than 512 filled slots
LM_X, LM_Y = 43, 46         # frame 1: the rows with 100 and 130 children


def _lm_rows1100():
    """1100 rows of 640 slots, about 9000 points, two frames.  A row r with r % 37 == 5 is bad: bad rows fall inside every pass.
    Frame 0 holds 130 points with lists of 17 and 33 rows that cover the bank three times over, and points that tie the rows of
    LM_TIE at the maximum; bad row 5 gets more votes than any of them.  Rows 600 and 900 hold 300 and 600 points, shared
    with rows on both sides of them.  Frame 1's points are seen by rows 40-99 only; each of its first rows has a covisible
    nobody voted for, so the walk ends at the limit; row 43 has 100 children of which the first 70 are bad or voted, row 46 has
    130 such children and no other."""
    rows, cap, frames = 1100, 640, 2
    rng = np.random.default_rng(811)
    bad_rows = [r for r in range(rows) if r % 37 == 5]
    point_rows = []
    cover = np.concatenate([rng.permutation(rows) for _ in range(3)])
    at, f0 = 0, []
    for j in range(130):                                        # frame 0: lists of 17 and 33 distinct rows
        k = 17 if j % 2 == 0 else 33
        rs = list(dict.fromkeys(cover[at:at + k].tolist()))
        at += k
        f0.append(len(point_rows))
        point_rows.append(rs)
    assert at >= 2 * rows
    votes = np.bincount(np.concatenate(point_rows), minlength=rows)
    top = int(votes.max()) + 4
    for r in LM_TIE:                                            # the tie at the maximum
        for _ in range(top - int(votes[r])):
            f0.append(len(point_rows))
            point_rows.append([r])
    for _ in range(top + 3 - int(votes[5])):                    # a bad row with the most votes of all
        f0.append(len(point_rows))
        point_rows.append([5])
    voted1 = [r for r in range(40, 100) if r not in bad_rows]
    f1 = []
    for j in range(70):                                         # frame 1
        f1.append(len(point_rows))
        point_rows.append(rng.choice(voted1, int(rng.integers(2, 6)), replace=False).tolist())
    for r in voted1:                                            # every one of them is voted
        f1.append(len(point_rows))
        point_rows.append([r])
    for fat, k in zip(LM_FAT, (300, 600)):                      # the rows with many slots
        for _ in range(k):
            others = rng.choice(rows, int(rng.integers(0, 3)), replace=False).tolist()
            point_rows.append([fat] + [r for r in others if r not in LM_FAT])
    while len(point_rows) < 9000:                               # the bulk: one to three rows each
        point_rows.append([r for r in rng.choice(rows, int(rng.integers(1, 4)), replace=False).tolist() if r not in LM_FAT] or [0])
    npts = len(point_rows)
    pcap = npts + 64
    held = set(f0) | set(f1)
    bad_points = [p for p in rng.choice(npts, npts // 10, replace=False).tolist() if p not in held]
    S = dict(frames=frames)
    LC._finish(S, rng, rows, cap, npts, pcap, point_rows, bad_rows, bad_points)
    fresh = iter(range(1000, 1100))                             # rows nobody of frame 1 voted for, not bad
    covis = {r: [bad_rows[1], voted1[0], next(x for x in fresh if x not in bad_rows)] for r in voted1[:30]}
    pool = bad_rows + voted1                                    # children the walk cannot take
    children = {LM_X: (pool * 2)[:70] + [1090, 1091] + pool[:28], LM_Y: (pool * 2)[:130]}
    LC._graph(S, rows, covis, children, {})
    LC._random_point_arrays(S, rng, pcap)
    fp = np.full((frames, cap), -1, i32)
    some_bad = bad_points[:9]
    a = rng.permutation(np.array(f0 + some_bad + [-1] * 20, i32))
    b = rng.permutation(np.array(f1 + bad_points[9:14] + [-1] * 7, i32))
    fp[0, :len(a)], fp[1, :len(b)] = a, b
    S["frame_point"], S["frame_n"] = fp, np.array([len(a), len(b)], i32)
    S["local_kf"], S["n_local_kf"] = np.full((frames, rows), -1, i32), np.zeros(frames, i32)
    return S


def _lm_cap4096():
    """40 rows of 4096 slots, 18000 points in arrays of 20000.  Row 7 is the second observer of exactly 4096 points, so all its
    slots are taken; frame 0 has 4096 key points, 3000 of them with a point."""
    rows, cap, npts, pcap, frames = 40, 4096, 18000, 20000, 2
    rng = np.random.default_rng(812)
    others = np.array([r for r in range(rows) if r != 7])
    point_rows = [[int(rng.choice(others))] for _ in range(npts)]
    for p in rng.choice(npts, cap, replace=False).tolist():
        point_rows[p].append(7)
    for p in range(0, npts, 3):
        r = int(rng.choice(others))
        if r not in point_rows[p]:
            point_rows[p].append(r)
    S = dict(frames=frames)
    LC._finish(S, rng, rows, cap, npts, pcap, point_rows, (3, 30), rng.choice(npts, npts // 10, replace=False))
    assert S["n"][7] == cap and (S["slot_point"][7] >= 0).all()
    LC._graph(S, rows, {r: [(r + 1) % rows, (r + 5) % rows] for r in range(rows)}, {}, {})
    LC._random_point_arrays(S, rng, pcap)
    fp = np.full((frames, cap), -1, i32)
    fp[0] = rng.permutation(np.concatenate([rng.choice(npts, 3000, replace=False), np.full(cap - 3000, -1)])).astype(i32)
    fp[1, :100] = rng.choice(npts, 100, replace=False)
    S["frame_point"], S["frame_n"] = fp, np.array([cap, 100], i32)
    S["local_kf"], S["n_local_kf"] = np.full((frames, rows), -1, i32), np.zeros(frames, i32)
    return S


LM_TOP = dict(voted=(65504, 65535), bad=65534, covisible=65520, parent=65530)


def _lm_rows65536():
    """65536 rows of 64 slots, 300 points seen by rows 10, 300, 5000, 40000, 65504, 65534 (bad) and 65535.  The walk of frame 0
    passes a bad and a voted covisible of row 10 and appends row 65520, then the parent 65530 of row 300 ends it: both in the
    last word of the stamp bitset.  Frame 1 votes the two top rows only."""
    rows, cap, npts, pcap, frames = LM_MAX_ROWS, 64, 300, 320, 2
    rng = np.random.default_rng(813)
    seen = np.array([10, 300, 5000, 40000, 65504, 65534, 65535])
    point_rows = [rng.choice(seen, int(rng.integers(1, 5)), replace=False).tolist() for _ in range(200)]
    point_rows += [rng.choice(seen[4:], int(rng.integers(1, 4)), replace=False).tolist() for _ in range(100)]
    S = dict(frames=frames)
    per_row = {int(r): [] for r in seen}
    for p, rs in enumerate(point_rows):
        for r in rs:
            if len(per_row[r]) < cap - 3:
                per_row[r].append(p)
    S["slot_point"], S["n"] = np.full((rows, cap), -1, i32), np.zeros(rows, i32)
    for r, s in per_row.items():
        s = np.array(s + [-1] * 3, i32)
        S["slot_point"][r, :len(s)], S["n"][r] = rng.permutation(s), len(s)
    S["obs_start"] = np.concatenate([[0], np.cumsum([len(rs) for rs in point_rows])]).astype(i32)
    S["obs_kf"] = np.array([r for rs in point_rows for r in rs] + [0], i32)
    S["kf_bad"] = np.zeros(rows, u8)
    S["kf_bad"][[LM_TOP["bad"], 77]] = 1
    S["flags"] = np.zeros(pcap, u8)
    S["flags"][:npts] = LC.PRESENT | (rng.random(npts) < 0.85) * LC.OBSERVED
    S["flags"][rng.choice(npts, 30, replace=False)] &= ~np.uint8(LC.PRESENT)
    S.update(rows=rows, cap=cap, np=npts, pcap=pcap)
    S["covis"] = np.full((rows, 10), -1, i32)
    S["covis"][10, :3] = [LM_TOP["bad"], 65535, LM_TOP["covisible"]]
    S["covis"][65504, :2] = [65535, 65505]
    S["child_start"], S["child"] = np.zeros(rows + 1, i32), np.zeros(1, i32)
    S["parent"] = np.full(rows, -1, i32)
    S["parent"][300] = LM_TOP["parent"]
    LC._random_point_arrays(S, rng, pcap)
    fp = np.full((frames, cap), -1, i32)
    fp[0, :50] = rng.choice(200, 50, replace=False)
    fp[1, :30] = 200 + rng.choice(100, 30, replace=False)
    S["frame_point"], S["frame_n"] = fp, np.array([50, 30], i32)
    S["local_kf"], S["n_local_kf"] = np.full((frames, rows), -1, i32), np.zeros(frames, i32)
    return S


LM_SCENES = dict(lm_rows1100=_lm_rows1100, lm_cap4096=_lm_cap4096, lm_rows65536=_lm_rows65536)


@functools.lru_cache(maxsize=None)
def lm_case(name):
    """(S, R): the layout of LC.scene_and_reference."""
    S = LM_SCENES[name]()
    R = LM.update_local_map(S, S["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"], pcap=S["pcap"])
    _freeze(S, dict(a=R["frame_point"], b=R["votes"], c=R["taken"], d=R["report"]))
    return S, R


def lm_add_track_arrays(S, seed=814):
    """What TrackLocalMapDevice reads on top of a local-map scene: a camera, a pose, key points and descriptors per frame."""
    import test_seqref_projection_cpu as PC
    rng = np.random.default_rng(seed)
    frames, cap = S["frames"], S["cap"]
    cam, scam = PC.make_cam()
    keys = np.zeros((frames, cap), LC.KEY_DTYPE)
    keys["x"], keys["y"] = rng.uniform(10, PC.W - 10, (frames, cap)), rng.uniform(10, PC.H - 10, (frames, cap))
    keys["octave"], keys["angle"], keys["size"] = rng.integers(0, 8, (frames, cap)), rng.uniform(0, 360, (frames, cap)), 31
    return dict(S, cam=cam, scam=scam, T=[PC.pose(rng, small=False) for _ in range(frames)], keys=keys,
                desc=rng.integers(0, 256, (frames, cap, 32), dtype=np.uint8))


def lm_owners(S, local_kf):
    """first[p] = (list position, slot) of the first slot of the list's rows that holds good point p."""
    first = {}
    for pos, row in enumerate(np.asarray(local_kf).tolist()):
        sp = S["slot_point"][row, :S["n"][row]]
        for i in np.nonzero(sp >= 0)[0].tolist():
            p = int(sp[i])
            if (S["flags"][p] & LC.PRESENT) and p not in first:
                first[p] = (pos, i)
    return first


# ---------------------------------------------------------------------------------------------------------------------
# culling
CU_SCENES = {                     # name: (keywords of cull_scene, candidate list)
    "cu_rows1100": (dict(rows=1100, seed=826, stereo=True, npts=5000, big=True, cap=1536, big_at=1000),
                    [1098, 3, 0, 6, 9, 12, 15, 18, 21, 7, 8, -1, 1000]),
    "cu_full4096": (dict(rows=4096, seed=822, stereo=True, npts=1500, big=True, cap=512, big_at=4010, hub_row=30), [4094, 6, 12]),
}
CU_RECENT = 3000


@functools.lru_cache(maxsize=None)
def cu_case(name):
    """The layout of KC.scene_and_reference; map-point culling (mp) on the mid-size case only."""
    kw, cand = CU_SCENES[name]
    T, state = KC.cull_scene(**kw)
    info = {}
    kf = KC.reference_key_frames(T, state, cand, 0, False, KC.TH_DEPTH, info)
    mp = {}
    if name == "cu_rows1100":
        rec = KC.recent_list(T, CU_RECENT, 823)
        mp[CU_RECENT] = dict(recent=rec, out=KC.reference_map_points(T, rec, 100, 3, info))
    _freeze(T, state, kf, *[m["out"] for m in mp.values()])
    return dict(T=T, state=state, cand=np.array(cand, i32), id0=0, mono=False, th_obs=3, kf=kf, mp=mp, info=info, kw=kw)


# ---------------------------------------------------------------------------------------------------------------------
# map-point refresh: more long points than k_update_points_long has workgroups
UPD_COUNTS = [17, 17, 17, 5, 17, 17, 17, 17, 17, 17, 17, 0] * 100 + [65] * 6 + [17] * 94


@functools.lru_cache(maxsize=None)
def upd_case():
    """The bank of test_mappoint_cpu's random scene with a table of 1300 points: 1094 lists of 17 and 6 of 65 (1057 of them present), some short ones."""
    import test_mappoint_cpu as MC
    from seqref import mappoint as MP
    S = MC.scene_and_reference(MC.BOTH)[0]
    rng = np.random.default_rng(831)
    n = len(UPD_COUNTS)
    slots = [rng.choice(MC.FAMILY_SLOTS, N, replace=N > MC.FAMILY_SLOTS) + (p % MC.FAMILIES) * MC.FAMILY_SLOTS
             for p, N in enumerate(UPD_COUNTS)]
    okf = np.concatenate([s % MC.ROWS for s in slots]).astype(i32)
    oidx = np.concatenate([s // MC.ROWS for s in slots]).astype(i32)
    start = np.concatenate([[0], np.cumsum(UPD_COUNTS)]).astype(i32)
    ref_obs = (rng.integers(0, 1 << 30, n) % np.maximum(np.array(UPD_COUNTS), 1)).astype(i32)
    world = rng.normal(0, 8, (n, 3)).astype(f32)
    flags = np.where(rng.random(n) < 0.05, 0, 1).astype(u8)
    ref = MP.update_map_points(S["scam"], MC.BOTH, S["T"], S["keys"], S["desc"], S["kf_bad"], start, okf, oidx, ref_obs, world, flags,
                               *MC.sentinels(n))
    for a in ref:
        a.setflags(write=False)
    return dict(n=n, start=start, okf=okf, oidx=oidx, ref_obs=ref_obs, world=world, flags=flags, ref=ref)


# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)                                               # a case that passed is not checked again
def preconditions(name):
    """Raises AssertionError naming the precondition that the reference's report, info or arrays do not meet."""
    if name == "cv_blocks2":
        S = cv_case(name)
        T = S["T"]
        assert cv_slot_blocks(T["cap"]) == 2 and T["rows"] == 65
        ok = 0
        for r in set(S["upd"].tolist()):
            a, b = _voters_by_block(T, r, 2)
            ok += _filled(T, r) > 2 * GROUP and len(a & b) > 3         # rows 1 and 64 hold a few points only
        assert ok >= 4 and (S["report"][:, 0] == CV.OK).sum() >= 5 and (S["report"][:, 4] >= CV_TH).any()
    elif name == "cv_blocks8":
        S = cv_case(name)
        T = S["T"]
        assert cv_slot_blocks(T["cap"]) == CV_MAX_BLOCKS and (T["cap"] + CV_BLOCK_SLOTS - 1) // CV_BLOCK_SLOTS > CV_MAX_BLOCKS
        assert sort_size(T["rows"]) == 2048 and T["rows"] > 4 * WG
        for r in (B8["A"], B8["B"], B8["C"], B8["H"]):
            assert _filled(T, r) > 1024, "%s: row %d has %d filled slots" % (name, r, _filled(T, r))
            sets = _voters_by_block(T, r, CV_MAX_BLOCKS)
            spread = max(sum(k in s for s in sets) for k in set.union(*sets))
            assert all(sets) and spread >= (CV_MAX_BLOCKS if r in (B8["A"], B8["B"]) else 4), \
                "%s: the votes of row %d for one row come from %d workgroups" % (name, r, spread)
        _tied_maximum(S, 0, B8["A"], B8["A_TIE"], 0)
        a, b = (where(r) for r in B8["A_TIE"])
        assert a[1] > b[1] and B8["A_TIE"][0] < B8["A_TIE"][1], "%s: the lower row is not in the higher wavefront" % name
        _tied_maximum(S, 1, B8["B"], B8["B_TIE"], 0)
        lo, other, late = (where(r) for r in B8["B_TIE"])
        assert lo[1:] == late[1:] and lo[0] < late[0], "%s: no tie between two passes of one thread" % name
        assert other[1] == lo[1] and other[2] < lo[2] and B8["B_TIE"][1] > B8["B_TIE"][0], \
            "%s: no tie between lanes with the higher row in the lower lane" % name
        _tied_maximum(S, 2, B8["C"], B8["C_TIE"], 1)
        a, b = (where(r) for r in B8["C_TIE"])
        assert a[1] > b[1], "%s: the fallback's lower row is not in the higher wavefront" % name
        rep = _report(S, 0)
        assert rep["n_ordered"] > WG and rep["n_resorted"] > WG, rep
        assert S["out"]["n_ord"][B8["A"]] > WG and (S["report"][:, 0] == CV.EMPTY).any()
        assert S["info"].get("equal_weight_return", 0) > 0 and S["info"].get("resort", 0) > 1000
        H = cv_case("cv_blocks8_host")
        res = cv_resident_rows(T, H["upd"])
        assert 24 < len(res) < 100 and max(res) > 1024 and (H["report"][:, 0] == CV.OK).all(), "%s: %d resident rows" % (name, len(res))
        assert H["touched"] <= res and len(H["touched"]) > 24
    elif name == "cv_wide":
        S = cv_case(name)
        rep = _report(S, 0)
        assert rep["n_ordered"] == 319 > WG and rep["n_resorted"] == 319 > WG and rep["fallback"] == 0, rep
        assert cv_slot_blocks(S["T"]["cap"]) == 6 and _filled(S["T"], W_HUB) > 5 * CV_BLOCK_SLOTS
        assert (S["out"]["conn_w"][W_HUB] == 14).sum() == 10
    elif name == "cv_full4096":
        S = cv_case(name)
        T, out = S["T"], S["out"]
        assert T["rows"] == CV_MAX_ROWS == sort_size(T["rows"]) and T["cap"] >= 897 and cv_slot_blocks(T["cap"]) == CV_MAX_BLOCKS
        assert F_HUB in S["touched"] and F_HUB not in S["upd"] and out["n_ord"][F_HUB] == 4095
        w = out["ord_w"][F_HUB, :4095]
        assert (np.diff(w) == 0).sum() > 2000 and (np.diff(w) <= 0).all()
        assert 4095 in S["upd"] and out["conn_w"][10, 4095] >= CV_TH and (S["report"][:, 0] == CV.OK).all()
        assert out["conn_w"][10, F_HUB] >= CV_TH
    elif name == "children":
        C = children_case("rows4096")
        kids = C["child"][C["start"][CHILD_P]:C["start"][CHILD_P + 1]]
        assert C["rows"] == CV_MAX_ROWS and len(kids) >= 700 and len(set((kids // WG).tolist())) >= 3
        between = C["parent"][kids[0]:kids[-1]]
        assert len(set(between.tolist())) > 20 and C["bad"][100:4050:5].sum() > 20, "children: nothing between the children of %d" % CHILD_P
        last = C["child"][C["start"][CHILD_LAST]:C["start"][CHILD_LAST + 1]]
        assert CHILD_LAST // WG == (C["rows"] - 1) // WG and len(last) > 100
        C = children_case("rows1025")
        assert C["start"][1] == 1024 and C["rows"] > 4 * WG
    elif name == "lm_rows1100":
        S, R = lm_case(name)
        rep0, rep1 = LC.report(R, 0), LC.report(R, 1)
        assert rep0["n_local_kf"] > LM_POS_BLOCKS and rep0["n_local_kf"] > WG and rep0["status"] == LM.OK
        v = np.where(S["kf_bad"] != 0, 0, R["votes"][0])
        assert tuple(np.nonzero(v == v.max())[0].tolist()) == LM_TIE
        assert rep0["ref_row"] == LM_TIE[0] and rep0["ref_votes"] == v.max()
        lo, lane_hi, lane_lo, late, wave0 = (where(r) for r in LM_TIE)
        assert lo[1:] == late[1:] and lo[0] < late[0], "%s: no tie between two passes of one thread" % name
        assert lane_hi[1] == lo[1] and lane_hi[2] != lo[2], "%s: no tie between two lanes of the reference row's wavefront" % name
        assert lane_lo[1] == lo[1] and lane_lo[2] < lo[2] and LM_TIE[2] > LM_TIE[0], \
            "%s: no tie between lanes with the higher row in the lower lane" % name
        assert wave0[1] < lo[1] and LM_TIE[4] > LM_TIE[0], "%s: the lower row is not in the higher wavefront" % name
        assert R["votes"][0].max() > v.max() and not S["kf_bad"][list(LM_TIE)].any()
        bad = np.nonzero(S["kf_bad"])[0]
        assert set((bad // WG).tolist()) == set(range((S["rows"] + WG - 1) // WG)) and (R["votes"][0][bad] > 0).all()
        held = R["frame_point"][0][R["frame_point"][0] >= 0]
        assert {17, 33} <= set(np.diff(S["obs_start"])[held].tolist())
        first = lm_owners(S, R["local_kf"][0])
        lk = R["local_kf"][0].tolist()
        for fat, least in zip(LM_FAT, (WG, 2 * WG)):
            assert _filled(S, fat) > least and fat in lk
            pos, sp = lk.index(fat), S["slot_point"][fat, :S["n"][fat]]
            for b in range(0, len(sp), WG):
                good = [(i, int(sp[i])) for i in range(b, min(b + WG, len(sp))) if sp[i] >= 0 and S["flags"][sp[i]] & LC.PRESENT]
                win = sum(first[p] == (pos, i) for i, p in good)
                assert 0 < win < len(good), "%s: row %d, slots from %d: %d winners of %d" % (name, fat, b, win, len(good))
        assert rep0["n_local_points"] > 7000
        assert rep1["n_voted"] < LM_MAX_KF and rep1["walk_end"] == LM.WALK_LIMIT and rep1["n_local_kf"] == LM_MAX_KF + 1
        lk1 = R["local_kf"][1].tolist()
        n_first = rep1["n_voted"] - int((S["kf_bad"][np.nonzero(R["votes"][1])[0]] != 0).sum())
        visits = LM_MAX_KF + 1 - n_first - 1                      # every visit appends a covisible, one of them a child too
        assert lk1.index(LM_X) < visits and lk1.index(LM_Y) < visits and 1090 in lk1 and 1091 not in lk1
        for r, k in ((LM_X, 100), (LM_Y, 130)):
            ch = S["child"][S["child_start"][r]:S["child_start"][r + 1]]
            assert len(ch) == k and all(S["kf_bad"][c] or c in lk1[:n_first] for c in ch[:WAVE]), \
                "%s: an acceptable child among the first 64 of row %d" % (name, r)
        ch = S["child"][S["child_start"][LM_Y]:S["child_start"][LM_Y + 1]]
        assert all(S["kf_bad"][c] or c in lk1[:n_first] for c in ch)
    elif name == "lm_cap4096":
        S, R = lm_case(name)
        rep = LC.report(R, 0)
        assert S["cap"] == 4096 and S["n"][7] == 4096 and S["frame_n"][0] == 4096 and 7 in R["local_kf"][0]
        assert rep["n_local_points"] > 4096 and S["pcap"] >= 20000 and rep["status"] == LM.OK
        first, pos = lm_owners(S, R["local_kf"][0]), R["local_kf"][0].tolist().index(7)
        wins = [first[int(p)] == (pos, i) for i, p in enumerate(S["slot_point"][7]) if S["flags"][p] & LC.PRESENT]
        assert 0 < sum(wins[-200:]) and 0 < sum(wins) < len(wins)
    elif name == "lm_rows65536":
        S, R = lm_case(name)
        rep = LC.report(R, 0)
        assert S["rows"] == LM_MAX_ROWS and all(R["votes"][0][r] > 0 for r in LM_TOP["voted"]) and R["votes"][0][LM_TOP["bad"]] > 0
        lk = R["local_kf"][0].tolist()
        assert LM_TOP["covisible"] in lk and lk[-1] == LM_TOP["parent"] and rep["walk_end"] == LM.WALK_PARENT and LM_TOP["bad"] not in lk
        assert all(r >> 5 == LM_MAX_ROWS // 32 - 1 for r in (LM_TOP["covisible"], LM_TOP["parent"], LM_TOP["bad"], 65535, 65504))
        assert R["local_kf"][1].tolist() == [65504, 65535, 65505]
    elif name == "cu_rows1100":
        S = cu_case(name)
        T, rep = S["T"], S["kf"]["report"]
        assert cu_slot_blocks(T["cap"]) == 6 and sort_size(T["rows"]) == 2048 and T["rows"] == 1100
        assert set(rep[:, 0].tolist()) == {CU.NOT_CULLED, CU.CULLED, CU.SKIPPED_ID0, CU.SKIPPED_ENTRY, CU.NOT_ERASE}
        culled = [u for u in range(len(rep)) if rep[u, 0] == CU.CULLED]
        heavy = [u for u in culled if rep[u, 1] > WG and rep[u, 3] > WG and _filled(T, int(S["cand"][u])) > 1024]
        assert len(heavy) >= 3, "%s: %d culled candidates with n_mps and n_erased above %d" % (name, len(heavy), WG)
        assert any(rep[u, 4] > 0 for u in heavy) and any(rep[u, 5] > WAVE for u in culled)
        assert S["info"].get("child_adopted", 0) > 0 and S["info"].get("child_fell_back", 0) > 0
        par = S["kf"]["parent"][1025:1071]
        assert rep[0, 0] == CU.CULLED and rep[0, 6] > WAVE and ((par >= 1000) & (par < 1071)).sum() > 5 and (par == 3).sum() > 0
        out = S["mp"][CU_RECENT]["out"]
        assert set(out["status"].tolist()) == {CU.KEPT, CU.ALREADY_BAD, CU.BAD_RATIO, CU.BAD_OBS, CU.DROPPED_OLD}
    elif name == "cu_full4096":
        S = cu_case(name)
        T, rep, hub = S["T"], S["kf"]["report"], S["kw"]["hub_row"]
        assert T["rows"] == CU_MAX_ROWS == sort_size(T["rows"]) and S["state"]["n_ord"][hub] == 4095
        assert (rep[:, 0] == CU.CULLED).all() and S["kf"]["n_ord"][hub] == 4095 - len(rep) > 2048
        par0, par = S["state"]["parent"], S["kf"]["parent"]
        kids = np.nonzero(par0 == 4094)[0]
        assert (kids >= 4064).sum() > 10 and ((par[kids] >= 4064) & (par[kids] != 4094)).sum() > 0, \
            "%s: no adoption in the last bitset word" % name
        assert rep[0, 6] > WAVE and S["info"].get("child_adopted", 0) > 0
    elif name == "upd_long":
        C = upd_case()
        long_points = int(((np.diff(C["start"]) > UPD_GROUP) & (C["flags"] & 1 != 0)).sum())
        assert long_points > UPD_LONG_BLOCKS and {17, 65} <= set(np.diff(C["start"]).tolist()), "%d long points" % long_points
    else:
        raise KeyError(name)
