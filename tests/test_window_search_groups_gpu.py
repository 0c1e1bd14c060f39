"""k_window_search<L>: 16 lanes per query (four queries per wavefront) for the SearchByProjection family, the whole
wavefront for SearchForInitialization.  Hand-built frames aimed at what the lane groups changed:
  * list lengths around the group chunk (16 / 17), the second .. fourth owned key of the rank sort (31 .. 63) and the
    move from the LDS-only list to `cand` (64 / 65),
  * windows wider than 16 grid columns (2, 3 and 4 trips of the column loop, whose carry of total / b1 / b2 / nb is dead
    code with 64 lanes),
  * groups of one wavefront with very different work (80 candidates beside 0 and 1; 1 .. 33 queries),
  * every gate of the candidate test, the image borders, invalid queries inside a group (device entries),
  * both widths forced on the development build (child process; a process can load one build only).
Every case first asserts ON THE CPU, with seqref.features_in_area and its own arithmetic, that the construction gives
the list lengths / column counts it claims.  Results are compared for equality (counts and whole assignment arrays) with
tests/seqref/matcher.py."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from seqref import matcher as SM  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 1241, 376
BOUNDS = (0.0, 0.0, float(W), float(H))
SF = np.cumprod(np.concatenate([[f32(1)], np.full(7, f32(1.2))])).astype(f32)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80)
NNRATIO = 0.8
_BITS = [(3, 1), (11, 4), (19, 16), (27, 64)]


# ---- construction ------------------------------------------------------------------------------------------------
def _keys(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), SM.KP_DTYPE)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = octave, angle, 31.0, 20.0, -1
    return k


def _family(rng, n, base, flips=(0, 1, 2, 3)):
    """n descriptors at small, heavily TIED distances from `base` (0 .. 3 of four fixed bits set), as in
    test_resolve_adversarial_gpu.py: the (distance, visiting order) sort is what decides."""
    d = np.repeat(base[None, :], n, 0).copy()
    for i in range(n):
        for j in range(int(rng.choice(flips))):
            d[i, _BITS[j][0]] ^= np.uint8(_BITS[j][1])
    return d


def _far(rng, n, base):
    """n descriptors more than TH_HIGH away from every member of base's family: 140 bits flipped in the bytes the
    family leaves alone."""
    d = np.repeat(base[None, :], n, 0).copy()
    free = [b for b in range(256) if b // 8 not in [byte for byte, _ in _BITS]]
    for i in range(n):
        for b in rng.choice(free, 140, replace=False):
            d[i, b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _queries(uv, radius, lmin=-1, lmax=-1, angle=0.0, observed=1, ur=-1.0):
    uv = np.asarray(uv, f32).reshape(-1, 2)
    q = np.zeros(len(uv), SM.QUERY_DTYPE)
    q["valid"] = 1
    q["u"], q["v"] = uv[:, 0], uv[:, 1]
    q["radius"], q["min_level"], q["max_level"], q["ur"], q["angle"], q["observed"] = radius, lmin, lmax, ur, angle, observed
    return q


def _case(k, d, q, qd, ur=None, taken=None):
    return {"k": k, "d": np.ascontiguousarray(d), "q": q, "qd": np.ascontiguousarray(qd),
            "ur": None if ur is None else np.asarray(ur, f32), "taken": None if taken is None else np.asarray(taken, np.uint8)}


def _frame(c):
    return SM.Frame(c["k"], c["d"], c["ur"], BOUNDS, SF)


def _window(S, c, i):
    """indices the window + level tests of query i keep, in visiting order"""
    q = c["q"]
    return SM.features_in_area(S, q["u"][i], q["v"][i], f32(q["radius"][i]), int(q["min_level"][i]), int(q["max_level"][i]))


def _listed(S, c, i, cut):
    """what k_window_search lists for query i: window, levels, the stereo gate and (cut = True: the frame search) the
    acceptance distance.  Slots taken on entry stay listed."""
    idx = _window(S, c, i)
    if len(idx) == 0:
        return idx
    keep = np.ones(len(idx), bool)
    urt = S.u_right[idx]
    keep &= ~((urt > 0) & (np.abs((f32(c["q"]["ur"][i]) - urt).astype(f32)) > f32(c["q"]["radius"][i])))
    if cut:
        keep &= SM.descriptor_distance(c["qd"][i], S.desc[idx]) <= SM.TH_HIGH
    return idx[keep]


def _columns(S, q, i):
    """(first, last) grid column of query i's window (src/Frame.cc:332-346), None when it is empty"""
    x, r = f32(q["u"][i]), f32(q["radius"][i])
    lo = max(0, int(math.floor(f32(f32(f32(x - S.min_x) - r) * S.inv_w))))
    hi = min(SM.FRAME_GRID_COLS - 1, int(math.ceil(f32(f32(f32(x - S.min_x) + r) * S.inv_w))))
    return None if lo >= SM.FRAME_GRID_COLS or hi < 0 or hi < lo else (lo, hi)


def case_lengths():
    """One cluster per target length, three queries on each (so the sorted row is walked past its first entry)."""
    rng = np.random.default_rng(101)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    xy, uv = [], []
    for i, n in enumerate(LENGTHS):
        centre = np.array([90.0 + 160.0 * (i % 7), 100.0 + 170.0 * (i // 7)])
        xy.append(centre + rng.uniform(-8, 8, (n, 2)))
        uv.append(centre + rng.uniform(-1, 1, (3, 2)))
    xy.append(np.array([1180.0, 5.0]) + rng.uniform(0, 1, (20, 2)) * np.array([55.0, 35.0]))   # the rest: far away
    xy, uv = np.concatenate(xy), np.concatenate(uv)
    n = len(xy)
    k = _keys(xy, rng.integers(0, 3, n), rng.choice([10.0, 10.0, 10.0, 200.0], n).astype(f32))
    c = _case(k, _family(rng, n, base), _queries(uv, 20.0, 0, 2, 10.0, (rng.random(len(uv)) < 0.8).astype(np.int32)),
              _family(rng, len(uv), base, (0, 0, 1, 2)))
    S = _frame(c)
    for i, n in enumerate(LENGTHS):
        for j in range(3):
            assert len(_listed(S, c, 3 * i + j, True)) == n == len(_listed(S, c, 3 * i + j, False)), (n, j)
    return c


def case_wide(ntrain):
    """Radius 200 / 700 at the image centre and at two corners: 12 .. 64 window columns = 1 .. 4 trips of 16."""
    rng = np.random.default_rng(200 + ntrain)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    xy = rng.uniform(0, 1, (ntrain, 2)) * np.array([W - 4.0, H - 4.0]) + 2.0
    uv, rad = [], []
    for pos in ((W / 2.0, H / 2.0), (0.0, 0.0), (float(W), float(H))):
        for r in (200.0, 700.0):
            uv += [pos, pos]
            rad += [r, r]
    k = _keys(xy, rng.integers(0, 3, ntrain), rng.choice([10.0, 10.0, 200.0], ntrain).astype(f32))
    c = _case(k, _family(rng, ntrain, base), _queries(uv, np.array(rad, f32), angle=10.0,
                                                      observed=(rng.random(len(uv)) < 0.7).astype(np.int32)),
              _family(rng, len(uv), base, (0, 1, 2)))
    S = _frame(c)
    trips, lens = set(), []
    for i in range(len(uv)):
        lo, hi = _columns(S, c["q"], i)
        nt = (hi - lo + 1 + 15) // 16
        trips.add(nt)
        got = _listed(S, c, i, True)
        lens.append(len(got))
        col = np.array([S.pos_in_grid(j)[0] for j in got]) - lo
        assert col.min() >= 0 and col.max() <= hi - lo
        if nt > 1:   # candidates in the first and in the last trip of the column loop
            assert (col // 16 == 0).any() and (col // 16 == nt - 1).any(), (i, nt)
    assert trips == {1, 2, 3, 4}, trips
    if ntrain <= 64:
        assert 0 < min(lens) and max(lens) <= 64, lens
    else:
        assert max(lens) > 250 and sorted(lens)[len(lens) // 2] > 64 and min(lens) <= 64, lens
    return c


def case_uneven(nq):
    """Queries 0, 1, 2, 3, ... sit on a cluster of 80, on nothing, on a single keypoint, on the 80 again, ..."""
    rng = np.random.default_rng(300 + nq)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    spots = np.array([[300.0, 150.0], [1000.0, 300.0], [700.0, 150.0]])
    xy = np.concatenate([spots[0] + rng.uniform(-8, 8, (80, 2)), spots[2][None, :],
                         np.array([60.0, 340.0]) + rng.uniform(0, 20, (10, 2))])
    uv = np.stack([spots[i % 3] + rng.uniform(-1, 1, 2) for i in range(nq)])
    k = _keys(xy, rng.integers(0, 3, len(xy)), 10.0)
    c = _case(k, _family(rng, len(xy), base), _queries(uv, 20.0, 0, 2, 10.0, (rng.random(nq) < 0.8).astype(np.int32)),
              _family(rng, nq, base, (0, 0, 1, 2)))
    S = _frame(c)
    for i in range(nq):
        assert len(_listed(S, c, i, True)) == (80, 0, 1)[i % 3], i
    return c


def case_levels():
    rng = np.random.default_rng(401)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    centre = np.array([500.0, 200.0])
    xy = centre + rng.uniform(-8, 8, (42, 2))
    k = _keys(xy, np.arange(42) % 6, 10.0)
    q = _queries(centre + rng.uniform(-1, 1, (4, 2)), 20.0, np.array([1, 2, 0, -1]), np.array([3, -1, 0, -1]), 10.0)
    c = _case(k, _family(rng, 42, base), q, _family(rng, 4, base, (0, 1)))
    S = _frame(c)
    assert [len(_listed(S, c, i, True)) for i in range(4)] == [21, 28, 7, 42]
    return c


def case_acceptance_cut():
    """12 of a window's 30 keypoints are beyond TH_HIGH: the frame search (mode 0) does not list them, the map-point
    search (mode 1) does."""
    rng = np.random.default_rng(402)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    centre = np.array([500.0, 200.0])
    xy = centre + rng.uniform(-8, 8, (30, 2))
    d = _family(rng, 30, base)
    far = rng.choice(30, 12, replace=False)
    d[far] = _far(rng, 12, base)
    c = _case(_keys(xy, 0, 10.0), d, _queries(centre + rng.uniform(-1, 1, (5, 2)), 20.0, angle=10.0), _family(rng, 5, base, (0, 1)))
    S = _frame(c)
    for i in range(5):
        assert len(_window(S, c, i)) == 30 and len(_listed(S, c, i, True)) == 18 and len(_listed(S, c, i, False)) == 30
    return c


def case_taken_best():
    """Two clusters (40 and 70 keypoints); every keypoint at the smallest distance of some query is taken on entry."""
    rng = np.random.default_rng(403)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    c1, c2 = np.array([400.0, 150.0]), np.array([800.0, 250.0])
    xy = np.concatenate([c1 + rng.uniform(-8, 8, (40, 2)), c2 + rng.uniform(-8, 8, (70, 2))])
    uv = np.concatenate([c1 + rng.uniform(-1, 1, (6, 2)), c2 + rng.uniform(-1, 1, (6, 2))])
    c = _case(_keys(xy, 0, 10.0), _family(rng, 110, base, (0, 1, 1, 2, 2, 3)), _queries(uv, 20.0, angle=10.0),
              _family(rng, 12, base, (0, 1)))
    S = _frame(c)
    taken = np.zeros(110, np.uint8)
    for i in range(12):
        idx = _listed(S, c, i, True)
        dist = SM.descriptor_distance(c["qd"][i], S.desc[idx])
        taken[idx[dist == dist.min()]] = 1
    c["taken"] = taken
    for i in range(12):
        idx = _listed(S, c, i, True)
        assert len(idx) == (40 if i < 6 else 70) and taken[idx].any() and not taken[idx].all()
    return c


def case_stereo_gate():
    rng = np.random.default_rng(404)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    centre = np.array([600.0, 180.0])
    xy = (centre + rng.uniform(-8, 8, (45, 2))).astype(f32)
    ur = np.where(np.arange(45) % 3 == 0, xy[:, 0] - f32(20), np.where(np.arange(45) % 3 == 1, xy[:, 0] - f32(80), f32(-1)))
    uv = (centre + rng.uniform(-1, 1, (5, 2))).astype(f32)
    c = _case(_keys(xy, 0, 10.0), _family(rng, 45, base), _queries(uv, 20.0, angle=10.0, ur=uv[:, 0] - f32(20)),
              _family(rng, 5, base, (0, 1)), ur=ur)
    S = _frame(c)
    for i in range(5):
        assert len(_window(S, c, i)) == 45 and len(_listed(S, c, i, True)) == 30
    return c


def case_borders():
    """Windows clipped by the left / right / top / bottom border, and four windows entirely outside the grid."""
    rng = np.random.default_rng(405)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    inside = np.array([[5.0, 188.0], [1225.0, 188.0], [620.0, 3.0], [620.0, 366.0]])   # PosInGrid rejects x > 1231, y > 372
    outside = np.array([[-100.0, 188.0], [1400.0, 188.0], [620.0, -50.0], [620.0, 500.0]])
    xy = np.concatenate([np.clip(p + rng.uniform(-4, 4, (6, 2)), [0.5, 0.5], [W - 0.5, H - 0.5]) for p in inside])
    uv = np.concatenate([inside, outside, inside + 0.5])
    c = _case(_keys(xy, 0, 10.0), _family(rng, len(xy), base), _queries(uv, 20.0, angle=10.0), _family(rng, len(uv), base, (0, 1)))
    S = _frame(c)
    assert [len(_listed(S, c, i, True)) for i in range(12)] == [6] * 4 + [0] * 4 + [6] * 4
    assert [_columns(S, c["q"], i) for i in (4, 5)] == [None, None]
    return c


def case_init():
    """SearchForInitialization with level-0 keypoints in a 300 x 60 px band and 100-px windows: lists of 53 .. 128
    candidates that differ from query to query; F2's descriptors at untied distances so that the ratio test passes."""
    rng = np.random.default_rng(406)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    centre, spread = np.array([500.0, 180.0]), np.array([150.0, 30.0])
    k1 = _keys(centre + rng.uniform(-1, 1, (120, 2)) * spread, np.where(rng.random(120) < 0.9, 0, 1),
               rng.choice([30.0, 30.0, 31.0, 250.0], 120).astype(f32))
    k2 = _keys(centre + rng.uniform(-1, 1, (200, 2)) * spread, np.where(rng.random(200) < 0.9, 0, 2),
               rng.choice([30.0, 31.0, 100.0], 200).astype(f32))
    # descending distances along the query index: later queries come closer and steal
    d1 = np.repeat(base[None, :], 120, 0).copy()
    for i in range(120):
        for b in range(max(0, 6 - (7 * i) // 120) + int(rng.integers(0, 2))):
            d1[i, 5 + b] ^= np.uint8(1 << (b % 8))
    d2 = np.repeat(base[None, :], 200, 0).copy()
    flips = (rng.permutation(200) * 4) // 5                 # 0 .. 159, at most two keypoints per value
    for j in range(200):
        for b in rng.choice(np.arange(96, 256), int(flips[j]), replace=False):
            d2[j, b // 8] ^= np.uint8(1 << (b % 8))
    F1, F2 = SM.Frame(k1, d1, None, BOUNDS, SF), SM.Frame(k2, d2, None, BOUNDS, SF)
    lens = [len(SM.features_in_area(F2, k1["x"][i], k1["y"][i], 100.0, 0, 0)) for i in range(120) if k1["octave"][i] == 0]
    assert 0 < min(lens) <= 64 < max(lens) and len(set(lens)) > 10      # short and long lists, different per query
    assert SM.search_for_initialization(F1, F2, np.stack([k1["x"], k1["y"]], 1), 100, 0.9, True)[0] >= 3
    return k1, d1, k2, d2


GATES = {"levels": case_levels, "acceptance_cut": case_acceptance_cut, "taken_best": case_taken_best,
         "stereo_gate": case_stereo_gate, "borders": case_borders}


# ---- running -------------------------------------------------------------------------------------------------------
def run_case(pkg, c):
    """[(n, assign)] of the frame search with and without the rotation cull and of the map-point search"""
    view = pkg.FrameView(c["k"], c["d"], SF, BOUNDS, c["ur"])
    out = [pkg.ORBmatcher(0.9, ori).SearchByProjectionFrame(view, c["q"], c["qd"], c["taken"]) for ori in (True, False)]
    out.append(pkg.ORBmatcher(NNRATIO, True).SearchByProjectionPoints(view, c["q"], c["qd"], c["taken"]))
    return out


_want = {}


def want_case(name, c):
    """the sequential reference's results, computed once per case"""
    if name not in _want:
        S = _frame(c)
        _want[name] = [SM.search_by_projection_frame(S, c["q"], c["qd"], c["taken"], ori) for ori in (True, False)] + \
                      [SM.search_by_projection_points(S, c["q"], c["qd"], c["taken"], NNRATIO)]
    return _want[name]


def same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and np.array_equal(g[1], w[1]), (what, i, g[0], w[0])


def run_init(pkg):
    k1, d1, k2, d2 = case_init()
    prev = np.stack([k1["x"], k1["y"]], 1).astype(f32)
    return pkg.ORBmatcher(0.9, True).SearchForInitialization(pkg.FrameView(k1, d1, SF, BOUNDS), pkg.FrameView(k2, d2, SF, BOUNDS),
                                                             prev, 100)


def shared_cases():
    """the cases that run on the product build and, with the width forced, on the development build"""
    return [("lengths", case_lengths())] + [("wide%d" % n, case_wide(n)) for n in (50, 300)]


@pytest.fixture(scope="module")
def pkg():
    import orb_slam2_comment_amd as p
    return p


def test_list_length_boundaries(pkg):
    c = case_lengths()
    want = want_case("lengths", c)
    same(run_case(pkg, c), want, "lengths")
    assert want[1][0] >= len(LENGTHS) - 1 and want[2][0] > 0     # every non-empty cluster gives the frame search a match


@pytest.mark.parametrize("ntrain", [50, 300])
def test_windows_wider_than_16_columns(pkg, ntrain):
    c = case_wide(ntrain)
    want = want_case("wide%d" % ntrain, c)
    same(run_case(pkg, c), want, "wide")
    assert want[1][0] >= 6


@pytest.mark.parametrize("nq", [1, 3, 5, 15, 16, 17, 33])
def test_uneven_groups(pkg, nq):
    c = case_uneven(nq)
    want = want_case("uneven%d" % nq, c)
    same(run_case(pkg, c), want, "uneven")
    assert want[1][0] >= (nq + 2) // 3 and (nq < 3 or want[1][1][80] % 3 == 2)   # the single keypoint goes to one of its queries


@pytest.mark.parametrize("gate", sorted(GATES))
def test_gates(pkg, gate):
    c = GATES[gate]()
    want = want_case(gate, c)
    same(run_case(pkg, c), want, gate)
    assert want[1][0] > 0


def _device_pairs():
    """three pairs of different n and nq; every fifth and seventh query invalid, so valid and invalid ones share groups"""
    cs = [case_lengths(), case_uneven(17), case_stereo_gate()]
    for p, c in enumerate(cs):
        c["q"]["valid"] = (np.arange(len(c["q"])) % 5 != 2) & (np.arange(len(c["q"])) % 7 != p)
        if c["ur"] is None:
            c["ur"] = np.full(len(c["k"]), -1, f32)
        if c["taken"] is None:
            c["taken"] = (np.arange(len(c["k"])) % 11 == 3).astype(np.uint8)
    return cs


def test_device_entries_equal_host_entries(pkg):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    cs = _device_pairs()
    pairs = len(cs)
    cap = max(len(c["k"]) for c in cs) + 5
    qcap = max(len(c["q"]) for c in cs) + 6
    assert qcap % 16 != 0 and len({len(c["k"]) for c in cs}) == 3 and len({len(c["q"]) for c in cs}) == 3
    kps = np.zeros((pairs, cap), pkg.KP_DTYPE); desc = np.zeros((pairs, cap, 32), np.uint8)
    ur = np.full((pairs, cap), -1, f32); taken = np.zeros((pairs, cap), np.uint8)
    q = np.zeros((pairs, qcap), pkg.QUERY_DTYPE); qd = np.zeros((pairs, qcap, 32), np.uint8)
    n = np.array([len(c["k"]) for c in cs], np.int32); nq = np.array([len(c["q"]) for c in cs], np.int32)
    q["valid"] = 1                                     # beyond nq: never looked at
    for p, c in enumerate(cs):
        kps[p, :n[p]], desc[p, :n[p]], ur[p, :n[p]], taken[p, :n[p]] = c["k"], c["d"], c["ur"], c["taken"]
        q[p, :nq[p]], qd[p, :nq[p]] = c["q"], c["qd"]
        assert 0 < c["q"]["valid"][:16].sum() < 16
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)).copy()).to(dev)  # noqa: E731
    t_k, t_d, t_ur, t_tk, t_q, t_qd = t(kps), torch.from_numpy(desc).to(dev), torch.from_numpy(ur).to(dev), \
        torch.from_numpy(taken).to(dev), t(q), torch.from_numpy(qd).to(dev)
    t_n, t_nq = torch.from_numpy(n).to(dev), torch.from_numpy(nq).to(dev)
    t_a = torch.zeros((pairs, cap), dtype=torch.int32, device=dev); t_nm = torch.zeros(pairs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for mode in ("frame", "points"):
        m = pkg.ORBmatcher(NNRATIO, True)
        fn = m.SearchByProjectionFrameDevice if mode == "frame" else m.SearchByProjectionPointsDevice
        fn(pairs, t_k.data_ptr(), t_d.data_ptr(), t_n.data_ptr(), cap, BOUNDS, t_q.data_ptr(), t_qd.data_ptr(), t_nq.data_ptr(),
           qcap, t_a.data_ptr(), t_nm.data_ptr(), d_u_right=t_ur.data_ptr(), d_taken=t_tk.data_ptr())
        m.sync()
        assign, nm = t_a.cpu().numpy(), t_nm.cpu().numpy()
        for p, c in enumerate(cs):
            host = m.SearchByProjectionFrame if mode == "frame" else m.SearchByProjectionPoints
            hn, ha = host(pkg.FrameView(c["k"], c["d"], SF, BOUNDS, c["ur"]), c["q"], c["qd"], c["taken"])
            assert hn == nm[p] and np.array_equal(ha, assign[p, :n[p]]), (mode, p)
            S = _frame(c)
            sn, sa = SM.search_by_projection_frame(S, c["q"], c["qd"], c["taken"], True) if mode == "frame" else \
                SM.search_by_projection_points(S, c["q"], c["qd"], c["taken"], NNRATIO)
            assert hn == sn and np.array_equal(ha, sa) and hn > 0, (mode, p)


def test_track_last_frame_device_narrow_and_wide(pkg):
    """The shape of test_fused_track_last_frame_equals_seqref at 200 keypoints, th 15 and th 100 (radius 100 .. 358 px:
    windows of two and three column trips), against ProjectLastFrame + seqref per pair.  The product build takes the
    wavefront form above th 20; the child of test_both_widths_equal_the_product_build repeats th 100 with 16 lanes."""
    pytest.importorskip("torch")
    check_track(pkg, (15.0, 100.0))


def check_track(pkg, ths):
    import torch
    from helpers import frame_bounds, synth_frame
    from orb_slam2_comment_amd import matcher as M
    FX, CX, CY, BF = 718.856, 607.1928, 185.2157, 386.1448
    rng = np.random.default_rng(7)
    dev = torch.device("cuda", 0)
    ext = pkg.ORBextractor(200, 1.2, 8, 20, 7)
    frames = np.stack([synth_frame(1 + (i // 2) % 3, shift_xy=(3 * (i % 2), 0)) for i in range(6)])
    B, Hh, Ww = frames.shape
    cap = ext.capacity(Hh, Ww)
    d_img = torch.from_numpy(frames).to(dev)
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ext.set_stream(st)
    ext.extract_batch_device(d_img.data_ptr(), B, Hh, Ww, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr())
    torch.cuda.synchronize()
    kps = d_k.cpu().numpy().view(np.uint8).reshape(B, cap, 28).copy().view(pkg.KP_DTYPE).reshape(B, cap)
    desc, n = d_d.cpu().numpy(), d_n.cpu().numpy()
    assert 150 <= n.min() and n.max() <= 260
    sf = ext.GetScaleFactors()
    bounds = frame_bounds(frames[0])
    cam = M.make_camera(FX, FX, CX, CY, bounds, sf, mbf=BF, mb=BF / FX)
    pairs = B // 2
    zc = f32(12.0)
    Tlw = np.stack([np.eye(4, dtype=f32) for _ in range(pairs)])
    Tcw = Tlw.copy()
    Tcw[:, 0, 3] = f32(3.0) * zc / f32(FX)
    world = np.zeros((B, cap, 3), f32)
    flags = np.zeros((B, cap), np.uint8)
    for p in range(pairs):
        kl = kps[2 * p, :n[2 * p]]
        world[2 * p, :n[2 * p], 0] = (kl["x"] - f32(CX)) * zc / f32(FX)
        world[2 * p, :n[2 * p], 1] = (kl["y"] - f32(CY)) * zc / f32(FX)
        world[2 * p, :n[2 * p], 2] = zc
        flags[2 * p, :n[2 * p]] = (rng.random(n[2 * p]) < 0.9) * pkg.capi.POINT_PRESENT + \
            (rng.random(n[2 * p]) < 0.7) * pkg.capi.POINT_OBSERVED
    taken = (rng.random((pairs, cap)) < 0.05).astype(np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_Tcw, d_Tlw = t(Tcw[:, :3, :].reshape(pairs, 12)), t(Tlw[:, :3, :].reshape(pairs, 12))
    d_world, d_flags, d_taken = t(world), t(flags), t(taken)
    d_assign = torch.zeros((pairs, cap), dtype=torch.int32, device=dev)
    d_nm = torch.zeros(pairs, dtype=torch.int32, device=dev)
    for th in ths:
        m = pkg.ORBmatcher(0.9, True)
        m.set_stream(st)
        m.TrackLastFrameDevice(pairs, cam, d_Tcw.data_ptr(), d_Tlw.data_ptr(), d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(),
                               cap, 1, 2, 0, 2, d_world.data_ptr(), d_flags.data_ptr(), th, True, d_assign.data_ptr(),
                               d_nm.data_ptr(), d_taken=d_taken.data_ptr())
        torch.cuda.synchronize()
        assign, nm = d_assign.cpu().numpy(), d_nm.cpu().numpy()
        for p in range(pairs):
            fl, fc = 2 * p, 2 * p + 1
            q = m.ProjectLastFrame(cam, Tcw[p], Tlw[p], world[fl, :n[fl]], flags[fl, :n[fl]], kps[fl, :n[fl]], th, True)
            c = _case(kps[fc, :n[fc]], desc[fc, :n[fc]], q, desc[fl, :n[fl]], taken=taken[p, :n[fc]])
            S = SM.Frame(c["k"], c["d"], None, bounds, sf)
            lens = [len(_listed(S, c, i, True)) for i in range(len(q)) if q["valid"][i]]
            cols = [hi - lo + 1 for lo, hi in (_columns(S, q, i) for i in range(len(q)) if q["valid"][i])]
            print("th %g pair %d: longest list %d, widest window %d columns" % (th, p, max(lens), max(cols)))
            assert max(cols) > 16 if th == 100.0 else (0 < max(lens) <= 64 and max(cols) <= 16), (th, p)
            sn, sa = SM.search_by_projection_frame(S, q, c["qd"], c["taken"], True)
            assert nm[p] == sn and np.array_equal(assign[p, :n[fc]], sa), (th, p)
            assert sn > 20, (th, p, sn)


# ---- both widths on the development build ------------------------------------------------------------------------------
def _flat(results):
    return {"%s/%d/%s" % (name, i, f): np.asarray(r[j]) for name, res in results for i, r in enumerate(res)
            for j, f in enumerate(("n", "a", "p")[:len(r)])}


def _expected_lists(c, cut):
    """per query: the keys dist << 32 | cell << 20 | index of its listed candidates in sorted order, and those among them
    whose slot is not taken on entry"""
    S = _frame(c)
    out = []
    for i in range(len(c["q"])):
        idx = _listed(S, c, i, cut)
        dist = SM.descriptor_distance(c["qd"][i], S.desc[idx]) if len(idx) else []
        keys = sorted((int(d) << 32) | ((S.pos_in_grid(j)[0] * SM.FRAME_GRID_ROWS + S.pos_in_grid(j)[1]) << 20) | int(j)
                      for j, d in zip(idx.tolist(), list(dist)))
        free = [k for k in keys if c["taken"] is None or not c["taken"][k & 0xfffff]]
        out.append((keys, free))
    return out


def check_lists(pkg, L, name, c, width):
    """What the window search hands to the resolve, read back from the development build: cnt and the sorted compact row
    of every list of at most 64 entries must be exactly the CPU's; a longer list has cnt = -length and, in its row, an
    exact prefix (1 .. 8 keys) of the sorted order of its free candidates with the count | complete << 8 word behind."""
    assert c["q"]["valid"].all()                 # the host entries compact invalid queries away
    view = pkg.FrameView(c["k"], c["d"], SF, BOUNDS, c["ur"])
    nq, nlong = len(c["q"]), 0
    for cut in (True, False):
        m = pkg.ORBmatcher(NNRATIO, False)
        (m.SearchByProjectionFrame if cut else m.SearchByProjectionPoints)(view, c["q"], c["qd"], c["taken"])
        cnt, rows = np.zeros(nq, np.int32), np.zeros((nq, 64), np.uint64)
        pkg.capi.check(L.orbhip_dev_window_lists(m._h, nq, pkg.capi.ptr(cnt), pkg.capi.ptr(rows)), "orbhip_dev_window_lists")
        for i, (keys, free) in enumerate(_expected_lists(c, cut)):
            if len(keys) <= 64:
                assert cnt[i] == len(keys) and rows[i, :len(keys)].tolist() == keys, (name, width, cut, i, cnt[i], len(keys))
                continue
            nlong += 1
            hl, complete = int(rows[i, 8]) & 0xff, (int(rows[i, 8]) >> 8) & 1
            assert cnt[i] == -len(keys) and 1 <= hl <= 8 and int(rows[i, 8]) >> 9 == 0, (name, width, cut, i, cnt[i], hl)
            assert rows[i, :hl].tolist() == free[:hl], (name, width, cut, i)
            assert not complete or hl == len(free), (name, width, cut, i)
    return nlong


def test_both_widths_equal_the_product_build(pkg, tmp_path):
    """In a child process on the development build, with the width forced to 16 and to 64: the boundary and the wide-window
    cases (and SearchForInitialization at 16) equal what the product build gives here; cnt and the compact rows equal
    the CPU's lists; the fused tracking entry at th 100 with 16 lanes equals seqref."""
    results = [(name, run_case(pkg, c)) for name, c in shared_cases()] + [("init", [run_init(pkg)])]
    path = str(tmp_path / "product.npz")
    np.savez(path, **_flat(results))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:], file=sys.stderr)
    assert r.returncode == 0, "child failed with status %d" % r.returncode
    assert "widths 16 and 64: all cases equal the product build" in r.stdout


def _child(path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), "dev"], check=True)
    from orb_slam2_comment_amd import capi
    capi.use_library(os.path.join(ROOT, "tools", "_dev", "liborbhip_dev.so"))
    import orb_slam2_comment_amd as pkg
    L = capi.lib()
    want = dict(np.load(path))
    real_init = pkg.ORBmatcher.__init__
    lanes = [0]

    def init(self, *a, **k):                    # every handle the cases create gets the width
        real_init(self, *a, **k)
        capi.check(L.orbhip_dev_set_window_lanes(self._h, lanes[0]), "orbhip_dev_set_window_lanes")
    pkg.ORBmatcher.__init__ = init
    assert L.orbhip_dev_set_window_lanes(pkg.ORBmatcher()._h, 32) != 0     # only 0 / 16 / 64
    cases = shared_cases()
    for width in (16, 64, 0):
        lanes[0] = width
        got = _flat([(name, run_case(pkg, c)) for name, c in cases] + ([("init", [run_init(pkg)])] if width != 64 else []))
        assert set(got) == {k for k in want if width != 64 or not k.startswith("init/")}
        for key, v in got.items():
            assert np.array_equal(v, want[key]), (width, key)
        print("width %d: %d arrays equal" % (width, len(got)))
        if width:
            nlong = sum(check_lists(pkg, L, name, c, width) for name, c in cases + [("taken_best", case_taken_best())])
            assert nlong > 20
            print("width %d: cnt and compact rows equal the CPU's lists (%d long lists)" % (width, nlong))
    lanes[0] = 16
    check_track(pkg, (100.0,))
    print("width 16: TrackLastFrameDevice at th 100 equals seqref")
    print("widths 16 and 64: all cases equal the product build")


if __name__ == "__main__":
    _child(sys.argv[1])
