"""tests/seqref/culling.py (LocalMapping::MapPointCulling and KeyFrameCulling with both SetBadFlags, EraseObservation and
EraseConnection restated from the reference text) against cases worked by hand, one per rule; the scenes
tests/test_culling_gpu.py and tests/test_cpp_culling_gpu.py run the kernels on, with a non-vacuity check computed from seqref
alone; the two integer forms the kernels use; the declarations and the argument checks of the C-ABI entries.  No device."""
import ctypes as C
import os

import numpy as np

from seqref import covisibility as CV
from seqref import culling as CU
from test_covisibility_cpu import SENTINEL, random_scene

i32, u8, f32 = np.int32, np.uint8, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT, OBSERVED = CU.POINT_PRESENT, CU.POINT_OBSERVED
TABLE_KEYS = ("kps", "u_right", "depth", "n", "obs_start", "obs_kf", "obs_idx", "ref_obs", "not_erase")
IO_KEYS = ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child", "obs_start_out", "obs_kf_out", "obs_idx_out",
           "ref_obs_out")
STATE_KEYS = ("conn_w", "ord_kf", "ord_w", "n_ord", "covis", "first_conn", "parent")


# ---- small scenes by hand -----------------------------------------------------------------------------------------------------
def scene(rows, cap, obs, stereo=False):
    """obs[p] = the rows observing point p, in list order; every observing row holds the point in its next free slot.
    Octaves 0, depths 0, u_right -1 (stereo) or absent, every point present with reference observation 0, found == visible,
    first_kf_id 0."""
    n_pts = len(obs)
    T = dict(rows=rows, cap=cap, np=n_pts, pcap=n_pts, slot_point=np.full((rows, cap), -1, i32), n=np.zeros(rows, i32),
             octave=np.zeros((rows, cap), i32), depth=np.zeros((rows, cap), f32),
             u_right=np.full((rows, cap), -1, f32) if stereo else None, flags=np.full(n_pts, PRESENT | OBSERVED, u8),
             ref_obs=np.zeros(n_pts, i32), kf_bad=np.zeros(rows, u8), to_be_erased=np.zeros(rows, u8), not_erase=None,
             found=np.ones(n_pts, i32), visible=np.ones(n_pts, i32), first_kf_id=np.zeros(n_pts, i32))
    kf, idx = [], []
    for p, rs in enumerate(obs):
        for r in rs:
            i = int(T["n"][r])
            assert i < cap
            T["slot_point"][r, i] = p
            T["n"][r] = i + 1
            kf.append(r)
            idx.append(i)
    T["obs_start"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(i32)
    T["obs_kf"], T["obs_idx"] = np.array(kf, i32), np.array(idx, i32)
    return T


def make_map(T):
    return CU.Map(T["slot_point"], T["n"], T["u_right"], T["flags"], T["obs_start"], T["obs_kf"], T["obs_idx"], T["ref_obs"],
                  T["kf_bad"], T["to_be_erased"])


def connect(G, a, b, w):
    G.conn[a][b] = w
    G.conn[b][a] = w
    CV.update_best_covisibles(G, a)
    CV.update_best_covisibles(G, b)


def cull_mp(T, recent, cur_kf_id, th_obs, info=None):
    M = make_map(T)
    kept, status = CU.map_point_culling(M, recent, T["found"], T["visible"], T["first_kf_id"], cur_kf_id, th_obs, info)
    return M, kept, status.tolist()


def cull_kf(T, G, cand, id0_row=-1, mono=True, th_depth=0.0, info=None, M=None):
    M = make_map(T) if M is None else M
    rep = CU.key_frame_culling(M, G, cand, T["octave"], T["depth"], T["not_erase"], id0_row, mono, th_depth, info)
    return M, [dict(zip(CU.REPORT_FIELDS, r.tolist())) for r in rep]


def test_map_point_branches_and_their_precedence():
    #            p0      p1      p2      p3         p4   p5
    T = scene(4, 8, [[0, 1], [0, 1], [0, 1], [0, 1, 2], [0], [0, 1, 2]])
    T["flags"][0] = 0
    T["found"][1], T["visible"][1] = 1, 5                        # fails the ratio AND the observation test: the ratio is reported
    T["first_kf_id"][:] = [0, 0, 8, 7, 9, 8]
    M, kept, status = cull_mp(T, [0, 1, 2, 3, 4, 5], 10, 2)
    assert status == [CU.ALREADY_BAD, CU.BAD_RATIO, CU.BAD_OBS, CU.DROPPED_OLD, CU.KEPT, CU.KEPT]
    assert kept == [4, 5]
    assert [f & PRESENT for f in M.flags] == [0, 0, 0, 1, 1, 1] and M.flags[1] & OBSERVED      # nObs is not reset
    assert M.obs[1] == [] and M.obs[2] == [] and M.obs[3] == [(0, 3), (1, 3), (2, 0)]
    assert M.slot_point[0].tolist()[:6] == [0, -1, -1, 3, 4, 5] and M.slot_point[1].tolist()[:5] == [0, -1, -1, 3, 5]


def test_found_ratio_at_exactly_a_quarter_and_with_zero_visible():
    T = scene(1, 8, [[0]] * 5)
    T["found"][:] = [1, 1, 0, 3, 0]
    T["visible"][:] = [4, 5, 0, 0, 1]
    T["first_kf_id"][:] = 10
    _, kept, status = cull_mp(T, range(5), 10, 2)
    assert status == [CU.KEPT, CU.BAD_RATIO, CU.KEPT, CU.KEPT, CU.BAD_RATIO]


def test_th_obs_2_against_3_with_a_stereo_observation_counting_2():
    T = scene(2, 4, [[0, 1]], stereo=True)
    T["u_right"][0, 0] = 31.5
    T["first_kf_id"][0] = 8
    M, _, status = cull_mp(T, [0], 10, 3)
    assert M.nobs[0] == 3 and status == [CU.BAD_OBS]
    assert cull_mp(T, [0], 10, 2)[2] == [CU.KEPT]
    T["u_right"] = None
    M, _, status = cull_mp(T, [0], 10, 2)
    assert M.nobs[0] == 2 and status == [CU.BAD_OBS]


def test_erase_map_point_match_is_by_index():
    T = scene(2, 4, [[0, 1], [0]])
    T["slot_point"][1, 0] = 1                                    # the slot point 0's observation names holds point 1
    T["found"][0], T["visible"][0] = 0, 9
    info = {}
    M, _, _ = cull_mp(T, [0], 0, 2, info)
    assert M.slot_point[1, 0] == -1 and M.slot_point[0, 0] == -1 and M.slot_point[0, 1] == 1
    assert info["erase_match_other_point"] == 1


def test_a_point_listed_twice_is_already_bad_the_second_time():
    T = scene(1, 4, [[0], [0], [0]])
    T["found"][0], T["visible"][0] = 0, 9
    T["first_kf_id"][:] = [0, 7, 9]
    _, kept, status = cull_mp(T, [0, 1, 2, 0, 1, 2], 10, 0)
    assert status == [CU.BAD_RATIO, CU.DROPPED_OLD, CU.KEPT, CU.ALREADY_BAD, CU.DROPPED_OLD, CU.KEPT] and kept == [2, 2]


def redundant_row(n_red, n_other, observers=(1, 2, 3), rows=6):
    """Row 0 holds n_red points that `observers` see too, and n_other points only row 1 sees besides."""
    return scene(rows, 16, [[0] + list(observers)] * n_red + [[0, 1]] * n_other)


def test_nine_tenths_at_ten_points():
    for n_red, status in ((9, CU.NOT_CULLED), (10, CU.CULLED)):
        T = redundant_row(n_red, 10 - n_red)
        M, rep = cull_kf(T, CV.Graph(6), [0])
        assert (rep[0]["status"], rep[0]["n_mps"], rep[0]["n_redundant"]) == (status, 10, n_red)
        assert M.kf_bad[0] == (status == CU.CULLED)


def test_a_row_without_points_is_not_culled():
    T = scene(2, 4, [[1]])
    _, rep = cull_kf(T, CV.Graph(2), [0])
    assert rep[0]["status"] == CU.NOT_CULLED and rep[0]["n_mps"] == 0


def test_octave_level_plus_1_against_level_plus_2():
    T = redundant_row(10, 0)
    T["octave"][0, :] = 2
    T["octave"][1:4, :] = 3
    assert cull_kf(T, CV.Graph(6), [0])[1][0]["status"] == CU.CULLED
    T["octave"][3, :] = 4                                          # one of the three others is two levels coarser
    info = {}
    _, rep = cull_kf(T, CV.Graph(6), [0], info=info)
    assert rep[0]["status"] == CU.NOT_CULLED and rep[0]["n_redundant"] == 0 and info["decide_coarser_scale"] == 10


def test_depth_gates_and_mono():
    T = redundant_row(8, 2)
    T["depth"][0, 8], T["depth"][0, 9] = 40.5, -1.0                # the two points that are not redundant: too far, no depth
    T["depth"][0, 0] = 40.0                                        # at the threshold: counted
    _, rep = cull_kf(T, CV.Graph(6), [0], mono=False, th_depth=40.0)
    assert (rep[0]["status"], rep[0]["n_mps"], rep[0]["n_redundant"]) == (CU.CULLED, 8, 8)
    _, rep = cull_kf(T, CV.Graph(6), [0], mono=True, th_depth=40.0)
    assert (rep[0]["status"], rep[0]["n_mps"], rep[0]["n_redundant"]) == (CU.NOT_CULLED, 10, 8)


def test_observations_3_against_4():
    """Row 0 holds the points in its slots without being in their lists, so Observations() is what the others add up to."""
    for others, status in (((1, 2, 3), CU.NOT_CULLED), ((1, 2, 3, 4), CU.CULLED)):
        T = scene(6, 16, [list(others)] * 4)
        T["slot_point"][0, :4], T["n"][0] = [0, 1, 2, 3], 4
        info = {}
        M, rep = cull_kf(T, CV.Graph(6), [0], info=info)
        assert rep[0]["status"] == status and M.nobs[0] == len(others)
        assert rep[0]["n_erased"] == 0 and (status == CU.NOT_CULLED or info["erase_not_observed"] == 4)


def flip_scene():
    """Rows 1 and 2 hold the same ten points, which rows 3 and 4 see too: each is redundant until the other is culled.  An
    eleventh point of row 1 is seen by rows 5 and 6 only."""
    T = scene(7, 16, [[1, 2, 3, 4]] * 10 + [[5, 1, 6]])
    T["ref_obs"][:] = [0, 1, 2] + [0] * 8
    return T


def test_culling_the_first_of_a_pair_flips_the_verdict_of_the_second_in_either_order():
    M, rep = cull_kf(flip_scene(), CV.Graph(7), [1, 2])
    assert [r["status"] for r in rep] == [CU.CULLED, CU.NOT_CULLED] and M.kf_bad == [0, 1, 0, 0, 0, 0, 0]
    assert (rep[0]["n_mps"], rep[0]["n_redundant"], rep[1]["n_mps"], rep[1]["n_redundant"]) == (11, 10, 10, 0)
    M, rep = cull_kf(flip_scene(), CV.Graph(7), [2, 1])
    assert [r["status"] for r in rep] == [CU.CULLED, CU.NOT_CULLED] and M.kf_bad == [0, 0, 1, 0, 0, 0, 0]
    assert (rep[1]["n_mps"], rep[1]["n_redundant"]) == (11, 0)


def test_reference_observation_moves_to_the_first_entry_left():
    M, rep = cull_kf(flip_scene(), CV.Graph(7), [1])
    start, kf, idx, ref = M.table()
    assert kf[start[0]:start[1]].tolist() == [2, 3, 4] and idx[start[0]:start[1]].tolist() == [0, 0, 0]
    assert ref[:3].tolist() == [0, 0, 1]        # it was row 1: now row 2; it was row 2, second of four: now first; row 3 moved up
    assert M.ref[0] == 2 and M.ref[1] == 2 and M.ref[2] == 3


def test_a_point_falling_to_two_observations_goes_bad_and_leaves_third_key_frames():
    info = {}
    M, rep = cull_kf(flip_scene(), CV.Graph(7), [1], info=info)
    assert rep[0]["n_erased"] == 11 and rep[0]["n_bad"] == 1 and info["erase_turned_bad"] == 1
    assert not M.flags[10] & PRESENT and M.flags[10] & OBSERVED and M.nobs[10] == 2 and M.obs[10] == []
    assert M.slot_point[5, 0] == -1 and M.slot_point[6, 0] == -1
    assert M.slot_point[1].tolist()[:11] == list(range(11))       # mvpMapPoints of the bad key frame is not cleared
    assert M.table()[3][10] == -1 and all(M.flags[p] == PRESENT | OBSERVED and M.nobs[p] == 3 for p in range(10))


def test_the_same_point_in_two_slots_of_the_culled_row():
    T = flip_scene()
    T["slot_point"][1, 11], T["n"][1] = 4, 12
    info = {}
    M, rep = cull_kf(T, CV.Graph(7), [1], info=info)
    assert rep[0]["n_mps"] == 12 and rep[0]["n_redundant"] == 11 and rep[0]["n_erased"] == 11 and info["erase_not_observed"] == 1
    assert M.nobs[4] == 3 and M.obs[4] == [(2, 4), (3, 4), (4, 4)]


def test_connections_are_erased_on_the_other_side_and_the_asymmetric_one_is_left_alone():
    T = redundant_row(10, 0)
    G = CV.Graph(6)
    connect(G, 0, 1, 20)
    connect(G, 0, 2, 17)
    connect(G, 1, 2, 30)
    G.conn[0][3] = 4                                               # the own row names row 3, row 3 does not name row 0
    connect(G, 3, 4, 16)
    G.mirror = {k: G.dense()[k].copy() for k in ("ord_kf", "ord_w", "covis")}
    info = {}
    _, rep = cull_kf(T, G, [0], info=info)
    assert rep[0]["n_resorted"] == 2 and info["asymmetric_connection"] == 1
    assert G.conn[0] == {} and G.ord_kf[0] == [] and G.conn[1] == {2: 30} and G.ord_kf[1] == [2] and G.ord_kf[2] == [1]
    assert G.conn[3] == {4: 16} and G.ord_kf[3] == [4]
    D = G.dense()
    assert D["n_ord"][0] == 0 and (D["covis"][0] == -1).all() and D["ord_kf"][0, :2].tolist() == [1, 2]      # the bytes stay
    assert D["ord_kf"][1, :2].tolist() == [2, 0] and D["n_ord"][1] == 1      # a rewrite stores nothing behind the list


def test_not_erase_sets_to_be_erased_and_nothing_else():
    T = redundant_row(10, 0)
    T["not_erase"] = np.array([1, 0, 0, 0, 0, 0], u8)
    G = CV.Graph(6)
    connect(G, 0, 1, 20)
    M, rep = cull_kf(T, G, [0])
    assert rep[0] == dict(status=CU.NOT_ERASE, n_mps=10, n_redundant=10, n_erased=0, n_bad=0, n_resorted=0, n_children=0, fallback=0)
    assert M.to_be_erased == [1, 0, 0, 0, 0, 0] and M.kf_bad[0] == 0 and G.conn[1] == {0: 20} and M.nobs[0] == 4


def test_the_id0_row_and_a_gap_in_the_list_are_skipped():
    T = redundant_row(10, 0)
    M, rep = cull_kf(T, CV.Graph(6), [-1, 0], id0_row=0)
    assert [r["status"] for r in rep] == [CU.SKIPPED_ENTRY, CU.SKIPPED_ID0] and M.kf_bad[0] == 0 and rep[1]["n_mps"] == 0


def test_a_bad_candidate_is_visited_again_and_changes_nothing():
    T = redundant_row(10, 0, observers=(1, 2, 3, 4, 5))
    G = CV.Graph(6)
    connect(G, 0, 1, 20)
    G.parent[0], G.parent[2] = 1, 0
    info = {}
    M, rep = cull_kf(T, G, [0, 0], info=info)
    assert rep[0] == dict(status=CU.CULLED, n_mps=10, n_redundant=10, n_erased=10, n_bad=0, n_resorted=1, n_children=1, fallback=1)
    assert rep[1] == dict(status=CU.CULLED, n_mps=10, n_redundant=10, n_erased=0, n_bad=0, n_resorted=0, n_children=0, fallback=0)
    assert info["bad_candidate_culled_again"] == 1 and G.parent[2] == 1 and M.nobs[0] == 5


def test_the_candidate_list_is_a_snapshot():
    """The candidates are the covisibles of row 5 when the call starts.  Culling row 1 re-sorts row 5, whose list then no
    longer names row 1 and starts with row 2; row 2 is still the second candidate and is visited once."""
    T = flip_scene()
    G = CV.Graph(7)
    connect(G, 5, 1, 30)
    connect(G, 5, 2, 20)
    cand = G.ord_kf[5]
    assert cand == [1, 2]
    M, rep = cull_kf(T, G, cand)
    assert G.ord_kf[5] == [2] and cand == [1, 2] and [r["status"] for r in rep] == [CU.CULLED, CU.NOT_CULLED]
    assert rep[1]["n_mps"] == 10


def reparent_scene():
    """Row 1 is culled.  Its parent is row 0; rows 2, 3, 4, 5 and 6 name it as their parent, row 6 is bad."""
    T = redundant_row(10, 0, rows=8)
    T["slot_point"][[0, 1]] = T["slot_point"][[1, 0]]              # row 1 is the redundant one
    T["n"][[0, 1]] = T["n"][[1, 0]]
    T["obs_kf"] = np.where(T["obs_kf"] == 0, 1, np.where(T["obs_kf"] == 1, 0, T["obs_kf"])).astype(i32)
    T["kf_bad"][6] = 1
    G = CV.Graph(8)
    G.parent = [-1, 0, 1, 1, 1, 1, 1, 0]
    return T, G


def test_reparenting():
    T, G = reparent_scene()
    connect(G, 2, 0, 7)             # child 2 knows the grandparent
    connect(G, 3, 2, 9)             # child 3 knows only child 2, a candidate once it is adopted
    connect(G, 4, 7, 50)            # child 4 knows no candidate
    connect(G, 6, 0, 99)            # bad: not a child any more
    info = {}
    M, rep = cull_kf(T, G, [1], info=info)
    assert rep[0]["status"] == CU.CULLED and rep[0]["n_children"] == 4 and rep[0]["fallback"] == 1
    assert G.parent == [-1, 0, 0, 2, 0, 0, 1, 0] and info["child_adopted"] == 2 and info["child_fell_back"] == 2
    assert M.kf_bad[1] == 1 and G.parent[1] == 0                   # mpParent of the bad key frame stays


def test_reparenting_ties_go_by_child_order_then_list_order():
    T, G = reparent_scene()
    connect(G, 2, 0, 7)
    connect(G, 3, 0, 7)             # the same weight as child 2: the lower row is adopted first ...
    connect(G, 3, 2, 7)             # ... and then child 3 finds row 2 before row 0 in its list
    connect(G, 4, 0, 3)
    connect(G, 5, 0, 8)             # the strictly largest weight wins the first round
    assert G.ord_kf[3] == [2, 0]
    M, rep = cull_kf(T, G, [1])
    assert G.parent == [-1, 0, 0, 2, 0, 0, 1, 0] and rep[0]["fallback"] == 0 and rep[0]["n_children"] == 4


def test_a_culled_row_without_a_parent():
    T, G = reparent_scene()
    G.parent[1] = -1
    connect(G, 2, 0, 7)
    connect(G, 3, 2, 7)
    info = {}
    _, rep = cull_kf(T, G, [1], info=info)
    assert rep[0]["fallback"] == 1 and info["no_parent"] == 1 and G.parent[:6] == [-1, -1, -1, -1, -1, -1]


# ---- the integer forms the kernels use ----------------------------------------------------------------------------------------
def test_four_times_found_below_visible_equals_the_float_ratio_below_a_quarter():
    """(float)found / visible < 0.25f against 4 * found < visible for every visible below 2^24 at the found values around the
    boundary (the float quotient is monotonic in found), at the ends of the range, and on a random sample."""
    v = np.arange(1 << 24, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for f in (v // 4 - 1, v // 4, v // 4 + 1, np.zeros_like(v), np.full_like(v, (1 << 24) - 1), v):
            f = np.clip(f, 0, (1 << 24) - 1)
            assert np.array_equal(f.astype(f32) / v.astype(f32) < f32(0.25), 4 * f < v)
        rng = np.random.default_rng(5)
        f, v = rng.integers(0, 1 << 24, 1 << 22), rng.integers(0, 1 << 24, 1 << 22)
        assert np.array_equal(f.astype(f32) / v.astype(f32) < f32(0.25), 4 * f < v)


def test_ten_redundant_above_nine_points_equals_the_double_comparison():
    n = np.arange(4097, dtype=np.int64)[:, None]
    r = np.arange(4097, dtype=np.int64)[None, :]
    assert np.array_equal(r > 0.9 * n.astype(np.float64), 10 * r > 9 * n)


# ---- random scenes ------------------------------------------------------------------------------------------------------------
def cull_scene(rows, seed, stereo=True, npts=300, big=False, cap=64, big_at=100, hub_row=None):
    """A scene of test_covisibility_cpu.random_scene with what culling reads on top.  The lists are made maps (a row once)
    and get the key-point index of the slot that holds the point; the graph is what UpdateConnections of every row gives.
    Every third row sees its points at a coarse octave, so it is redundant while enough finer rows see them too.  big: a
    hub point seen by 70 rows, and row rows - 2 with 76 connections and 71 children that is culled; those rows start at big_at.
    cap: the slots of a bank row.  hub_row: a row every other row is connected with, both ways, weights 1-4."""
    T, state, G = random_scene(rows, seed, npts=npts, cap=cap, obs_lo=4, obs_hi=9)
    rng = np.random.default_rng(seed + 1000)
    cap, n_pts, pcap = T["cap"], T["np"], T["pcap"]
    where = {}
    for r in range(rows):
        for i in range(int(T["n"][r])):
            p = int(T["slot_point"][r, i])
            if p >= 0:
                where[(p, r)] = i
    lists = []
    for p in range(n_pts):
        rs = dict.fromkeys(int(k) for k in T["obs_kf"][T["obs_start"][p]:T["obs_start"][p + 1]])
        lists.append([(r, where[(p, r)]) for r in rs if (p, r) in where])
    big_row = rows - 2
    if big:
        assert rows >= 200 and 24 <= big_at and big_at + 76 <= big_row
        hub_pt = 7
        for r in range(big_at, big_at + 70):                        # the hub point: a list that crosses a wavefront
            i = int(T["n"][r])
            T["slot_point"][r, i], T["n"][r] = hub_pt, i + 1
            lists[hub_pt].append((r, i))
        T["flags"][hub_pt] = PRESENT
        T["n"][big_row] = 0
        T["slot_point"][big_row] = -1
        for p in range(20, 32):                                     # the big row sees twelve well observed points, coarsely
            lists[p] = [e for e in lists[p] if e[0] != big_row]
            i = int(T["n"][big_row])
            T["slot_point"][big_row, i], T["n"][big_row] = p, i + 1
            lists[p].append((big_row, i))
            T["flags"][p] = PRESENT
    for p in range(5, n_pts, 13):                                   # a slot an observation names holds another point
        q = (p + 1) % n_pts
        if lists[p] and (q, lists[p][0][0]) not in where:
            T["slot_point"][lists[p][0]] = q
    T["obs_start"] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(i32)
    T["obs_kf"] = np.array([k for x in lists for k, _ in x], i32)
    T["obs_idx"] = np.array([i for x in lists for _, i in x], i32)
    T["ref_obs"] = np.array([int(rng.integers(0, len(x))) if x else -1 for x in lists] + [0] * 0, i32)
    T["ref_obs"][::37] = -1
    T["flags"] = (T["flags"] | (OBSERVED * (np.arange(pcap) % 5 != 0)) | 4).astype(u8)       # bit 2: not the call's business
    base = np.where(np.arange(rows) % 3 == 0, 4, rng.integers(0, 3, rows))
    T["octave"] = (base[:, None] + rng.integers(0, 2, (rows, cap))).astype(i32)
    if big:
        T["octave"][big_row] = 7
    T["depth"] = rng.uniform(1.0, 44.0, (rows, cap)).astype(f32)
    T["depth"][rng.random((rows, cap)) < 0.05] = -1.0
    T["u_right"] = np.where(rng.random((rows, cap)) < 0.5, rng.uniform(0, 600, (rows, cap)), -1.0).astype(f32) if stereo else None
    T["found"] = rng.integers(0, 40, pcap).astype(i32)
    T["visible"] = (T["found"] * rng.choice([1, 2, 4, 5, 8], pcap) + rng.integers(0, 2, pcap)).astype(i32)
    T["visible"][::41] = 0
    T["first_kf_id"] = rng.integers(95, 101, pcap).astype(i32)
    T["kf_bad"] = np.zeros(rows, u8)
    T["to_be_erased"] = np.zeros(rows, u8)
    T["not_erase"] = np.zeros(rows, u8)
    # the graph: UpdateConnections of every row, then a few rows that are bad already
    CV.update_connections_list(G, list(range(rows)), T["slot_point"], T["n"], T["obs_start"], T["obs_kf"], T["flags"], 0)
    for r in (3, 6, 9):                                             # a connection only the own row holds
        if r < rows and G.conn[r]:
            c = min(G.conn[r], key=lambda k: (G.conn[r][k], k))
            G.conn[c].pop(r, None)
            CV.update_best_covisibles(G, c)
    if rows > 12:
        T["kf_bad"][[5, 11]] = 1
        T["not_erase"][[3, 9]] = 1
    if big:
        for c in range(big_at, big_at + 76):
            G.conn[big_row][c] = G.conn[c][big_row] = 1 + (c * 7) % 5
        G.conn[big_row][3] = G.conn[3][big_row] = 40
        for c in range(big_at, big_at + 71):
            G.parent[c] = big_row
            if c % 3 == 0:
                G.conn[c][3] = G.conn[3][c] = 2 + c % 4
            if c % 3 == 1:
                G.conn[c][c - 1] = G.conn[c - 1][c] = 5 + c % 2
        G.parent[big_row] = 3
        T["kf_bad"][big_at + 30] = 1
        for c in [3, big_row] + list(range(big_at - 1, big_at + 76)):
            CV.update_best_covisibles(G, c)
    if hub_row is not None:
        for c in range(rows):
            if c != hub_row:
                G.conn[hub_row][c] = G.conn[c][hub_row] = 1 + (c * 5) % 4
        for c in range(rows):
            CV.update_best_covisibles(G, c)
    fill = dict(ord_kf=np.full((rows, rows), SENTINEL, i32), ord_w=np.full((rows, rows), SENTINEL, i32),
                covis=np.full((rows, 10), SENTINEL, i32))
    state = G.dense(fill)
    start, child = CV.children_from_parents(state["parent"], T["kf_bad"])
    T["child_start"], T["child"] = start, np.concatenate([child, np.full(rows - len(child), SENTINEL, i32)]).astype(i32)
    T["obs_cap"] = len(T["obs_kf"]) + 3
    T["obs_kf"] = np.concatenate([T["obs_kf"], [0, 0, 0]]).astype(i32)
    T["obs_idx"] = np.concatenate([T["obs_idx"], [0, 0, 0]]).astype(i32)
    return T, state


def reference_key_frames(T, state, cand, id0_row, mono, th_depth, info=None):
    """seqref on the arrays of a scene: every in/out and output array of orbhip_cull_key_frames as it must come back.
    Entries behind a count hold SENTINEL (the table out, child) or what they held (the dense lists)."""
    M = make_map(T)
    G = CV.Graph.from_dense(state)
    G.mirror = {k: np.array(state[k], i32).copy() for k in ("ord_kf", "ord_w", "covis")}
    rep = CU.key_frame_culling(M, G, cand, T["octave"], T["depth"], T["not_erase"], id0_row, mono, th_depth, info)
    out = G.dense()
    out.update(table_out(M, T), report=rep, slot_point=M.slot_point, flags=np.array(M.flags, u8), kf_bad=np.array(M.kf_bad, u8),
               to_be_erased=np.array(M.to_be_erased, u8))
    start, child = CV.children_from_parents(out["parent"], out["kf_bad"])
    out["child_start"] = start
    out["child"] = np.concatenate([child, np.array(T["child"])[len(child):]]).astype(i32)
    return out


def table_out(M, T):
    start, kf, idx, ref = M.table()
    pad = np.full(T["obs_cap"] - len(kf), SENTINEL, i32)
    return dict(obs_start_out=start, obs_kf_out=np.concatenate([kf, pad]).astype(i32),
                obs_idx_out=np.concatenate([idx, pad]).astype(i32), ref_obs_out=ref)


def reference_map_points(T, recent, cur_kf_id, th_obs, info=None):
    M = make_map(T)
    kept, status = CU.map_point_culling(M, recent, T["found"], T["visible"], T["first_kf_id"], cur_kf_id, th_obs, info)
    out = table_out(M, T)
    out.update(slot_point=M.slot_point, flags=np.array(M.flags, u8), status=status, n_recent_out=np.array([len(kept)], i32),
               recent_out=np.concatenate([kept, np.full(len(recent) - len(kept), SENTINEL, i32)]).astype(i32))
    return out


def recent_list(T, R, seed):
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, T["np"], R).astype(i32)
    if R >= 2:
        rec[R - 1] = rec[0]                                        # a point listed twice
    return rec


GPU_SCENES = {                     # name: (rows, seed, stereo, big, candidate list)
    "r2": (2, 3, True, False, [1, 0]),
    "r12": (12, 21, True, False, [3, -1, 0, 6, 9, 1, 6, -1, 2]),       # gaps, and row 6 twice
    "r65": (65, 5, False, False, [0, 3, 6, 9, 12, 15, 18, 21, 5, 1, 2, 64]),
    "r257": (257, 6, True, True, [255, 3, 0, 6, 9, 12, 15, 18, 21, 7, 8, 11, 100]),
}
TH_DEPTH = 40.0
_CACHE = {}


def scene_and_reference(name):
    """The named scene and seqref's answers to both calls, computed once and shared; nobody writes to them."""
    if name not in _CACHE:
        rows, seed, stereo, big, cand = GPU_SCENES[name]
        T, state = cull_scene(rows, seed, stereo, big=big)
        id0 = 0 if rows > 2 else -1
        info = {}
        kf = reference_key_frames(T, state, cand, id0, not stereo, TH_DEPTH, info)
        mp = {}
        for R in (0, 1, 63, 64, 65, 1000):
            rec = recent_list(T, R, seed + R)
            mp[R] = dict(recent=rec, out=reference_map_points(T, rec, 100, 3 if stereo else 2, info))
        S = dict(T=T, state=state, cand=np.array(cand, i32), id0=id0, mono=not stereo, th_obs=3 if stereo else 2, kf=kf, mp=mp,
                 info=info)
        for d in (T, state, kf) + tuple(m["out"] for m in mp.values()):
            for a in d.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _CACHE[name] = S
    return _CACHE[name]


def test_gpu_scenes_are_not_vacuous():
    seen_kf, seen_mp, info = set(), set(), {}
    for name in GPU_SCENES:
        S = scene_and_reference(name)
        st = S["kf"]["report"][:, 0].tolist()
        seen_kf |= set(st)
        if S["T"]["rows"] >= 12:
            assert st.count(CU.CULLED) > 1, (name, st)
        for R, m in S["mp"].items():
            seen_mp |= set(m["out"]["status"].tolist())
        for k, v in S["info"].items():
            info[k] = info.get(k, 0) + v
        assert (S["kf"]["obs_start_out"][-1] < S["T"]["obs_start"][-1])
    assert seen_kf == {CU.NOT_CULLED, CU.CULLED, CU.SKIPPED_ID0, CU.SKIPPED_ENTRY, CU.NOT_ERASE}
    assert seen_mp == {CU.KEPT, CU.ALREADY_BAD, CU.BAD_RATIO, CU.BAD_OBS, CU.DROPPED_OLD}
    for key in ("erase_match_other_point", "erase_not_observed", "ref_moved", "erase_turned_bad", "asymmetric_connection",
                "not_erase", "child_adopted", "child_fell_back", "decide_bad_point", "decide_depth_gate", "decide_coarser_scale",
                "decide_few_observations", "bad_candidate_culled_again"):
        assert info.get(key, 0) > 0, (key, info)
    S = scene_and_reference("r257")
    big_row = 255
    rep = dict(zip(CU.REPORT_FIELDS, S["kf"]["report"][0].tolist()))
    assert rep["status"] == CU.CULLED and rep["n_resorted"] > 64 and rep["n_children"] > 64 and rep["fallback"] == 1
    assert S["state"]["n_ord"][big_row] > 64 and np.diff(S["T"]["obs_start"]).max() > 64
    par = S["kf"]["parent"][100:171]
    assert (par == 3).sum() > 5 and ((par >= 100) & (par < 171)).sum() > 5      # adopted by the grandparent, and by each other
    S = scene_and_reference("r12")
    assert S["kf"]["report"][6, 0] == S["kf"]["report"][3, 0] == CU.CULLED and S["cand"][6] == S["cand"][3]


# ---- C ABI without a device ---------------------------------------------------------------------------------------------------
def kp_array(octave):
    from orb_slam2_comment_amd import capi
    kps = np.zeros(octave.shape, capi.KP_DTYPE)
    kps["octave"] = octave
    return kps


def c_records(capi, T, S, out):
    rt, rio, rs = capi.CullTables(), capi.CullIO(), capi.CovisState()
    for k in TABLE_KEYS:
        if T.get(k) is not None:
            setattr(rt, k, capi.ptr(T[k]).value)
    for k in IO_KEYS:
        a = out[k] if k in out else T.get(k)
        if a is not None:
            setattr(rio, k, capi.ptr(a).value)
    for k in STATE_KEYS:
        setattr(rs, k, capi.ptr(S[k]).value)
    return rt, rio, rs


def test_culling_entries_exist_and_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device.  The entries are exported with the declared signatures and check counts,
    pointers, aliasing and (the host forms) every range before they look at the handle: with a null handle each violation is
    ORBHIP_E_ARG, named by orbhip_last_error, and valid arguments reach the handle check.  Nothing is written."""
    from orb_slam2_comment_amd import capi
    names = [s[0] for s in capi.SYMBOLS]
    for name in ("orbhip_cull_map_points", "orbhip_cull_map_points_device", "orbhip_cull_key_frames", "orbhip_cull_key_frames_device"):
        assert name in names
    assert (capi.CULLPOINT_KEPT, capi.CULLPOINT_ALREADY_BAD, capi.CULLPOINT_BAD_RATIO, capi.CULLPOINT_BAD_OBS,
            capi.CULLPOINT_DROPPED_OLD) == (CU.KEPT, CU.ALREADY_BAD, CU.BAD_RATIO, CU.BAD_OBS, CU.DROPPED_OLD)
    assert (capi.CULLKF_NOT_CULLED, capi.CULLKF_CULLED, capi.CULLKF_SKIPPED_ID0, capi.CULLKF_SKIPPED_ENTRY,
            capi.CULLKF_NOT_ERASE) == (CU.NOT_CULLED, CU.CULLED, CU.SKIPPED_ID0, CU.SKIPPED_ENTRY, CU.NOT_ERASE)
    assert capi.CULLKF_REPORT == CU.REPORT_FIELDS
    assert tuple(k for k, _ in capi.CullTables._fields_) == TABLE_KEYS and tuple(k for k, _ in capi.CullIO._fields_) == IO_KEYS
    L = capi.lib()
    T0 = flip_scene()
    T0.update(kps=kp_array(T0["octave"]), child_start=np.zeros(8, i32), child=np.zeros(7, i32), not_erase=np.zeros(7, u8))
    G = CV.Graph(7)
    connect(G, 1, 2, 20)
    S0 = G.dense()
    total = len(T0["obs_kf"])
    out0 = dict(obs_start_out=np.full(12, SENTINEL, i32), obs_kf_out=np.full(total, SENTINEL, i32),
                obs_idx_out=np.full(total, SENTINEL, i32), ref_obs_out=np.full(11, SENTINEL, i32))
    cand0, rep0 = np.array([1, -1, 2], i32), np.full((3, 8), SENTINEL, i32)
    rec0, rout0, nout0, st0 = np.array([0, 10], i32), np.full(2, SENTINEL, i32), np.full(1, SENTINEL, i32), np.full(2, 77, u8)

    def kf(m=None, rows=7, cap=16, n=11, pcap=11, obs_cap=total, id0=-1, U=3, cand=cand0, mono=1, T=T0, S=S0, out=out0, device=False,
           rep=rep0):
        rt, rio, rs = c_records(capi, T, S, out)
        fn = L.orbhip_cull_key_frames_device if device else L.orbhip_cull_key_frames
        return fn(m, rows, cap, n, pcap, obs_cap, C.byref(rt), C.byref(rio), C.byref(rs), id0, U, capi.ptr(cand), mono, 40.0,
                  capi.ptr(rep))

    def mp(m=None, rows=7, cap=16, n=11, pcap=11, obs_cap=total, R=2, rec=rec0, th_obs=2, T=T0, out=out0, device=False, found=True):
        rt, rio, _ = c_records(capi, T, S0, out)
        fn = L.orbhip_cull_map_points_device if device else L.orbhip_cull_map_points
        return fn(m, rows, cap, n, pcap, obs_cap, C.byref(rt), C.byref(rio), R, capi.ptr(rec), capi.ptr(T["found"]) if found else None,
                  capi.ptr(T["visible"]), capi.ptr(T["first_kf_id"]), 10, th_obs, capi.ptr(rout0), capi.ptr(nout0), capi.ptr(st0))

    def last():
        return (L.orbhip_last_error() or b"").decode()

    def changed(A, key, index, value):
        B = dict(A)
        if index is None:
            B[key] = value
        else:
            B[key] = np.array(A[key]).copy()
            B[key][index] = value
        return B
    before = {k: np.array(a).copy() for k, a in list(T0.items()) + list(S0.items()) if isinstance(a, np.ndarray)}
    alias = dict(out0, obs_kf_out=T0["obs_kf"])
    for device in (False, True):
        for kw in (dict(rows=-1), dict(n=-1), dict(n=12, pcap=11), dict(cap=0), dict(obs_cap=-1), dict(U=-1), dict(id0=7), dict(id0=-2),
                   dict(cand=None), dict(rep=None), dict(out=alias), dict(out=dict(out0, ref_obs_out=T0["ref_obs"])),
                   dict(out=dict(out0, obs_start_out=T0["obs_start"])), dict(out=dict(out0, obs_idx_out=T0["obs_idx"])),
                   dict(T=changed(T0, "kps", None, None)), dict(T=changed(T0, "obs_idx", None, None)),
                   dict(T=changed(T0, "kf_bad", None, None)), dict(T=changed(T0, "slot_point", None, None)),
                   dict(T=changed(T0, "to_be_erased", None, None)), dict(T=changed(T0, "depth", None, None), mono=0),
                   {}):
            assert kf(device=device, **kw) == capi.E_ARG, (device, kw)
        assert kf(device=device, T=changed(T0, "depth", None, None), mono=1, m=None) == capi.E_ARG        # reaches the handle check
        assert kf(device=device, rows=4097) == capi.E_CAPACITY and "4096" in last()
        assert kf(device=device, cap=4097) == capi.E_CAPACITY
        for kw in (dict(rows=-1), dict(n=-1), dict(n=12, pcap=11), dict(cap=0), dict(obs_cap=-1), dict(R=-1), dict(th_obs=-1),
                   dict(rec=None), dict(found=False), dict(out=alias), dict(T=changed(T0, "ref_obs", None, None)),
                   dict(T=changed(T0, "flags", None, None)), {}):
            assert mp(device=device, **kw) == capi.E_ARG, (device, kw)
        assert mp(device=device, rows=4097) == capi.E_CAPACITY and mp(device=device, cap=4097) == capi.E_CAPACITY
    twice = changed(T0, "obs_kf", 1, 1)
    for case, word in ((dict(cand=np.array([1, 7, 2], i32)), "candidate 1"), (dict(cand=np.array([1, 2, 1], i32)), "bank row 1 twice"),
                       (dict(cand=np.array([-2, 2, 1], i32)), "candidate 0"),
                       (dict(T=changed(T0, "obs_kf", 1, 7)), "observation 1"), (dict(T=changed(T0, "obs_idx", 2, 16)), "observation 2"),
                       (dict(T=twice), "names bank row 1 twice"),
                       (dict(T=changed(T0, "slot_point", (1, 0), 11)), "point index"),
                       (dict(T=changed(T0, "slot_point", (0, 1), -2)), "point index"),
                       (dict(T=changed(T0, "obs_start", 1, 9)), "non-decreasing"), (dict(T=changed(T0, "obs_start", 0, 1)), "start at 0"),
                       (dict(obs_cap=total - 1), "obs_cap"),
                       (dict(T=changed(T0, "n", 2, 17)), "bank row 2"), (dict(T=changed(T0, "n", 0, -1)), "bank row 0"),
                       (dict(S=changed(S0, "n_ord", 1, 8)), "n_ord of bank row 1"), (dict(S=changed(S0, "parent", 4, 7)), "parent of bank row 4"),
                       (dict(S=changed(S0, "ord_kf", (1, 0), 9)), "ordered list of bank row 1")):
        assert kf(**case) == capi.E_ARG and word in last(), (list(case), word, last())
    for case, word in ((dict(rec=np.array([0, 11], i32)), "list entry 1"), (dict(rec=np.array([-1, 3], i32)), "list entry 0"),
                       (dict(T=twice), "names bank row 1 twice"), (dict(T=changed(T0, "obs_start", 3, 1)), "non-decreasing")):
        assert mp(**case) == capi.E_ARG and word in last(), (list(case), word, last())
    assert (rep0 == SENTINEL).all() and (rout0 == SENTINEL).all() and (nout0 == SENTINEL).all() and (st0 == 77).all()
    assert all((a == SENTINEL).all() for a in out0.values())
    assert all(np.array_equal(before[k], a) for k, a in list(T0.items()) + list(S0.items()) if isinstance(a, np.ndarray))


def test_mirrors_declare_the_culling_interface():
    import orb_slam2_comment_amd as pkg
    methods = ("CullMapPoints", "CullMapPointsDevice", "CullKeyFrames", "CullKeyFramesDevice")
    for name in methods:
        assert callable(getattr(pkg.ORBmatcher, name))
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for sym in ("ORBHIP_CULLPOINT_KEPT        0", "ORBHIP_CULLPOINT_DROPPED_OLD 4", "ORBHIP_CULLKF_CULLED        1",
                "ORBHIP_CULLKF_NOT_ERASE     4"):
        assert "#define " + sym in hdr
    for name in ("orbhip_cull_map_points_device", "orbhip_cull_map_points", "orbhip_cull_key_frames_device", "orbhip_cull_key_frames"):
        assert "int %s(" % name in hdr
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for name in methods:
        assert "void %s(" % name in hpp
    mk = open(os.path.join(ROOT, "orb_slam2_comment_amd", "csrc", "Makefile")).read()
    assert "orbhip_culling.hip" in mk


if __name__ == "__main__":
    for name_ in GPU_SCENES:
        S_ = scene_and_reference(name_)
        print(name_, S_["kf"]["report"].tolist(), {R: np.bincount(m["out"]["status"], minlength=5).tolist() for R, m in S_["mp"].items()})
        print("  ", S_["info"])
