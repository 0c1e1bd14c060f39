"""One small scene aimed at the frame-grid rules themselves -- Frame::PosInGrid (`round`), the cell window of
Frame::GetFeaturesInArea (floor / ceil, clamped), the strict |dx| < r and Fuse's chi-square gate -- for every consumer of
those rules: test_grid_rules_cpu.py (sequential reference against the C oracle) and test_grid_rules_gpu.py (the kernels
against the sequential reference).

Bounds (-8, -8, 504, 376): the grid element inverse is 0.125 exactly in float32, a cell is 8 px, cell px holds
x in [8 px - 12, 8 px - 4), and rounding ties are hit exactly.  Scale factor 2, fx = fy = 1, cx = cy = 0, identity pose
and map points (u, v, 1): the Fuse prologue lands on the pixel (u, v) with radius th * 2^level without a rounding.

Every situation the scene claims is asserted here on tests/seqref: a case that lost its property fails in the builder."""
import math

import numpy as np

from orb_slam2_comment_amd import matcher as M
from seqref import matcher as SM
from seqref import projection as P

f32 = np.float32
BOUNDS = (-8.0, -8.0, 504.0, 376.0)
BOUNDS_OTHER = (-8.0, -8.0, 1016.0, 760.0)          # a key frame with another grid: FuseBatch sends it down the single-frame path
SF = (f32(2) ** np.arange(8)).astype(f32)
INV_SIGMA2 = (f32(1) / (SF * SF)).astype(f32)
TH, MBF = 4.0, 2.0
NNRATIO = 0.8
COLS, ROWS = SM.FRAME_GRID_COLS, SM.FRAME_GRID_ROWS
N_WHOLE = 12                                         # whole-grid queries with one and the same descriptor


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def columns(S, u, r, axis=0):
    """(first, last) cell of the window along one axis (src/Frame.cc:332-346), or the name of the exit the reference takes"""
    lo_b, inv, n = (S.min_x, S.inv_w, COLS) if axis == 0 else (S.min_y, S.inv_h, ROWS)
    u, r = f32(u), f32(r)
    lo = max(0, int(math.floor(f32(f32(f32(u - lo_b) - r) * inv))))
    if lo >= n:
        return "min>=n"
    hi = min(n - 1, int(math.ceil(f32(f32(f32(u - lo_b) + r) * inv))))
    return "max<0" if hi < 0 else (lo, hi)


def grid_csr(S):
    """(cell_of[n], cell_start[3073], cell_items) of AssignFeaturesToGrid from the reference's mGrid: push_back order"""
    cell_of = np.full(S.N, -1, np.int32)
    for i in range(S.N):
        p = S.pos_in_grid(i)
        if p is not None:
            cell_of[i] = p[0] * ROWS + p[1]
    sizes = [len(S.grid[x][y]) for x in range(COLS) for y in range(ROWS)]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    items = np.concatenate([S.grid[x][y] for x in range(COLS) for y in range(ROWS)]).astype(np.int32)
    return cell_of, start, items


_SCENE = {}


def scene():
    """The scene, built and checked once: dict with the train frame (k, d, ur, taken), the queries (q, qd), the names of
    the special key points / queries (`kp`, `qi`), the Fuse inputs (cam, scam, T, X, nrm, max_d, min_d, flags) and S /
    S_other, the reference frames on the two grids."""
    if _SCENE:
        return _SCENE
    rng = np.random.default_rng(2026)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    xy, lvl, nflip, kp = [], [], [], {}

    def add(name, x, y, level, k):
        if name:
            kp[name] = len(xy)
        xy.append((x, y)); lvl.append(level); nflip.append(k)

    # rounding ties (x - min_x) * inv_w = k + 0.5, k = -1, 0, 62, 63: round() gives -1 (rejected), 1, 63, 64 (rejected); the
    # rejected ones are the closest descriptors of the scene, the accepted ones tie with a companion in the cell that rint /
    # floor would send them to, and the companion has the HIGHER index: only the visiting order lets it win
    add("tie_x-12", -12.0, 96.0, 0, 0); add("tie_x-4", -4.0, 96.0, 0, 2)
    add("tie_x492", 492.0, 96.0, 0, 2); add("tie_x500", 500.0, 96.0, 0, 0)
    add("tie_y-12", 96.0, -12.0, 0, 0); add("tie_y-4", 96.0, -4.0, 0, 2)
    add("tie_y364", 96.0, 364.0, 0, 2); add("tie_y372", 96.0, 372.0, 0, 0)
    add("on_max_x", 504.0, 96.0, 0, 0); add("on_max_y", 96.0, 376.0, 0, 0)
    keep_clear = [(-20, 76, 20, 116), (470, 76, 520, 116), (76, -20, 116, 20), (76, 340, 116, 390),     # the border queries,
                  (140, 136, 172, 168), (300, 220, 340, 260)]                                            # the edges, the cluster
    inner = []
    while len(inner) < 340:                              # quarter-pixel positions away from the hand-placed key points
        x, y = rng.integers(0, 4 * 496) / 4.0, rng.integers(0, 4 * 368) / 4.0
        if not any(x0 <= x <= x1 and y0 <= y <= y1 for x0, y0, x1, y1 in keep_clear):
            inner.append((x, y))
    for i, (x, y) in enumerate(inner[:170]):
        add(None, x, y, int(rng.integers(0, 4)), int(rng.integers(4, 41)))
    add("comp_x-7", -7.0, 96.0, 0, 2); add("comp_x486", 486.0, 96.0, 0, 2)
    add("comp_y-7", 96.0, -7.0, 0, 2); add("comp_y358", 96.0, 358.0, 0, 2)
    # |dx| == r exactly (excluded by the strict <) and just inside; the one visited first has the higher index
    add("edge_hi_in", 159.5, 152.0, 0, 6); add("edge_lo_out", 152.0, 152.0, 0, 6)
    add("edge_hi_out", 160.0, 152.0, 0, 6); add("edge_lo_in", 152.5, 152.0, 0, 6)
    # several key points per cell in cells (40,30), (40,31), (41,30), dealt round robin: push_back order is not index order
    cells = [(40, 30), (40, 31), (41, 30)]
    for j in range(12):
        cx, cy = cells[j % 3]
        add("cell%d_%d" % (j % 3, j // 3), 8 * cx - 12 + 0.5 + (j * 5 % 7), 8 * cy - 12 + 0.5 + (j * 3 % 7), 1, 6)
    for x, y in inner[170:]:
        add(None, x, y, int(rng.integers(0, 4)), int(rng.integers(4, 41)))
    for j in range(8):                                   # coarse levels: what the whole-grid map point of Fuse can match
        add("coarse%d" % j, 40.0 + 55.0 * j, 30.0 + 40.0 * j, 6 + j % 2, 3 + j)
    n = len(xy)
    assert n <= 400
    k = np.zeros(n, SM.KP_DTYPE)
    k["x"], k["y"] = np.asarray(xy, f32).T
    k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = lvl, 10.0, 31.0, 20.0, -1
    d = np.stack([_flip(base, rng.choice(128, c, replace=False)) for c in nflip])        # flips in bytes 0 .. 15
    # mvuRight on half of the key points: consistent with a query at the same pixel (x - mbf), or 20 px off (the stereo gate)
    sel = rng.random(n)
    ur = np.where(sel < 0.25, k["x"] - f32(MBF), np.where(sel < 0.5, k["x"] - f32(MBF + 20), f32(-1))).astype(f32)
    named = np.array(sorted(kp.values()))
    taken = (rng.random(n) < 0.05).astype(np.uint8)
    taken[named] = 0

    # ---- queries: (u, v, level) with radius TH * 2^level and the level window [level - 1, level] = what Fuse's prologue gives
    uv, lev, qd, qi = [], [], [], {}

    def ask(name, u, v, level, desc=base, radius=None, levels=None):
        if name:
            qi[name] = len(uv)
        uv.append((u, v)); lev.append((level, radius, levels)); qd.append(desc)

    ask("left", -6.0, 96.0, 1); ask("right", 493.0, 96.0, 1); ask("top", 96.0, -6.0, 1); ask("bottom", 96.0, 365.0, 1)
    ask("out_left", -100.0, 96.0, 1); ask("invalid", 200.0, 200.0, 1); ask("out_right", 600.0, 96.0, 1)
    ask("out_top", 96.0, -100.0, 1); ask("out_bottom", 96.0, 500.0, 1)
    ask("on_boundaries", 156.0, 152.0, 0)
    ask("radius0", 152.0, 152.0, 0, radius=0.0, levels=(0, 3))
    ask("one_cell", 152.0, 152.0, 0, radius=2.0, levels=(0, 3))
    ask("cells", 316.0, 236.0, 1)
    ask("whole_coarse", 248.0, 184.0, 7)
    free = [i for i in range(n) if i not in set(named.tolist()) and 0 < xy[i][0] < 490 and 0 < xy[i][1] < 360]
    for j, t in enumerate(rng.choice(free, 48 - 14 - N_WHOLE, replace=False)):           # a target key point each
        level = lvl[t] + int(j % 2 and lvl[t] < 3)
        off = rng.integers(-3, 4, 2) / 2.0
        ask(None, xy[t][0] + off[0], xy[t][1] + off[1], level, _flip(d[t], [128 + int(rng.integers(0, 128))]))
    for j in range(N_WHOLE):                             # the same best candidates for all of them: list heads run out
        ask("whole%d" % j, 248.0, 184.0, 7, levels=(0, 7))
    nq = len(uv)
    assert nq == 48
    q = np.zeros(nq, SM.QUERY_DTYPE)
    q["valid"] = 1
    q["u"], q["v"] = np.asarray(uv, f32).T
    q["radius"] = [TH * 2.0 ** L if r is None else r for L, r, _ in lev]
    q["min_level"] = [L - 1 if lv is None else lv[0] for L, _, lv in lev]
    q["max_level"] = [L if lv is None else lv[1] for L, _, lv in lev]
    q["ur"], q["level_aux"], q["angle"], q["observed"] = q["u"] - f32(MBF), [L for L, _, _ in lev], 10.0, 1
    q["valid"][qi["invalid"]] = 0
    qd = np.stack(qd)

    # ---- Fuse: map points whose prologue gives exactly these records (where the pixel is in the image and r = TH * 2^level)
    cam = M.make_camera(1.0, 1.0, 0.0, 0.0, BOUNDS, SF, mbf=MBF, mb=MBF)
    scam = P.camera(cam)
    X = np.stack([q["u"], q["v"], np.ones(nq, f32)], 1).astype(f32)
    dist = np.sqrt((X.astype(np.float64) ** 2).sum(1))
    nrm = (X / dist[:, None]).astype(f32)
    max_d = (dist * 2.0 ** (np.array([L for L, _, _ in lev]) - 0.15)).astype(f32)
    min_d = (dist * 0.01).astype(f32)
    fusable = np.array([r is None and lv is None for _, r, lv in lev]) & (q["valid"] == 1)
    flags = fusable.astype(np.uint8) * P.POINT_PRESENT
    T = np.eye(4, dtype=f32)

    S = SM.Frame(k, d, ur, BOUNDS, SF)
    S_other = SM.Frame(k, d, ur, BOUNDS_OTHER, SF)
    _SCENE.update(k=k, d=d, ur=ur, taken=taken, q=q, qd=qd, kp=kp, qi=qi, cam=cam, scam=scam, T=T, X=X, nrm=nrm, max_d=max_d,
                  min_d=min_d, flags=flags, S=S, S_other=S_other, base=base)
    _check(_SCENE)
    return _SCENE


def _check(c):
    S, k, q, kp, qi = c["S"], c["k"], c["q"], c["kp"], c["qi"]
    assert S.inv_w == f32(0.125) and S.inv_h == f32(0.125)
    cell = lambda name: S.pos_in_grid(kp[name])  # noqa: E731
    # PosInGrid: ties go away from zero, the far borders are exclusive
    assert [cell("tie_x" + s) for s in ("-12", "-4", "492", "500")] == [None, (1, 13), (63, 13), None]
    assert [cell("tie_y" + s) for s in ("-12", "-4", "364", "372")] == [None, (13, 1), (13, 47), None]
    assert cell("on_max_x") is None and cell("on_max_y") is None
    for name, x in (("tie_x-12", -0.5), ("tie_x-4", 0.5), ("tie_x492", 62.5), ("tie_x500", 63.5)):      # exact ties
        assert f32(f32(k["x"][kp[name]] - S.min_x) * S.inv_w) == f32(x)
    for name, y in (("tie_y-12", -0.5), ("tie_y-4", 0.5), ("tie_y364", 46.5), ("tie_y372", 47.5)):
        assert f32(f32(k["y"][kp[name]] - S.min_y) * S.inv_h) == f32(y)
    # rint and floor would file the accepted ties in the companions' cells
    assert [cell(s) for s in ("comp_x-7", "comp_x486", "comp_y-7", "comp_y358")] == [(0, 13), (62, 13), (13, 0), (13, 46)]
    # push_back order inside the cells of the cluster differs from a sort by anything but the index, and cells interleave
    for j, (cx, cy) in enumerate([(40, 30), (40, 31), (41, 30)]):
        members = [kp["cell%d_%d" % (j, i)] for i in range(4)]
        got = S.grid[cx][cy].tolist()
        assert [g for g in got if g in members] == members and len(got) >= 4, (j, got)
    assert kp["cell1_0"] < kp["cell0_1"] < kp["cell1_1"]

    def area(name):
        i = qi[name]
        return SM.features_in_area(S, q["u"][i], q["v"][i], q["radius"][i], int(q["min_level"][i]), int(q["max_level"][i])).tolist()

    def cols(name, axis=0):
        i = qi[name]
        return columns(S, q["v" if axis else "u"][i], q["radius"][i], axis)

    # clipped at each border; the companion is visited before the tie although its index is higher; rejected ones stay out
    assert area("left") == [kp["comp_x-7"], kp["tie_x-4"]] and cols("left") == (0, 2)
    assert area("right") == [kp["comp_x486"], kp["tie_x492"]] and cols("right") == (61, 63)
    assert area("top") == [kp["comp_y-7"], kp["tie_y-4"]] and cols("top", 1) == (0, 2)
    assert area("bottom") == [kp["comp_y358"], kp["tie_y364"]] and cols("bottom", 1) == (45, 47)
    for name, rej in (("left", "tie_x-12"), ("right", "tie_x500"), ("top", "tie_y-12"), ("bottom", "tie_y372")):
        i, j = qi[name], kp[rej]                        # only the grid keeps the rejected key point out of the window
        assert abs(k["x"][j] - q["u"][i]) < q["radius"][i] and abs(k["y"][j] - q["v"][i]) < q["radius"][i]
        assert (c["d"][j] == c["qd"][i]).all()
    # wholly outside: both exits of the reference, on both axes
    assert [cols("out_left"), cols("out_right"), cols("out_top", 1), cols("out_bottom", 1)] == ["max<0", "min>=n", "max<0", "min>=n"]
    assert all(area(s) == [] for s in ("out_left", "out_right", "out_top", "out_bottom"))
    # window edges on cell boundaries: floor / ceil of integers, nothing wider; a key point exactly r away is out
    i = qi["on_boundaries"]
    assert f32(f32(f32(q["u"][i] - S.min_x) - q["radius"][i]) * S.inv_w) == 20 and cols("on_boundaries") == (20, 21)
    assert f32(f32(f32(q["v"][i] - S.min_y) - q["radius"][i]) * S.inv_h) == 19.5 and cols("on_boundaries", 1) == (19, 21)
    got = area("on_boundaries")
    assert got[:1] == [kp["edge_lo_in"]] and kp["edge_hi_in"] in got and kp["edge_lo_in"] > kp["edge_hi_in"]
    assert kp["edge_lo_out"] not in got and kp["edge_hi_out"] not in got
    assert abs(k["x"][kp["edge_lo_out"]] - q["u"][i]) == q["radius"][i] == abs(k["x"][kp["edge_hi_out"]] - q["u"][i])
    # radius 0: a window of cells, no candidate, not even the key point under the query
    assert cols("radius0") == (20, 20) and cols("radius0", 1) == (20, 20) and area("radius0") == []
    assert len(S.grid[20][20]) >= 2 and k["x"][kp["edge_lo_out"]] == q["u"][qi["radius0"]]
    # a window inside one cell (the reference still walks the neighbours: floor below, ceil above)
    assert cols("one_cell") == (19, 21) and set(area("one_cell")) >= {kp["edge_lo_out"], kp["edge_lo_in"]}
    i = qi["one_cell"]
    assert 8 * 20 - 12 <= q["u"][i] - q["radius"][i] and q["u"][i] + q["radius"][i] < 8 * 20 - 4
    assert len(area("cells")) >= 12
    # the whole grid: 64 columns = four trips of a 16-lane group, lists longer than 64, and for all N_WHOLE queries the same
    # eight nearest candidates, the rounding ties and their companions, which the border queries hold already
    assert cols("whole0") == (0, 63) and cols("whole0", 1) == (0, 47) and cols("whole_coarse") == (0, 63)
    whole = area("whole0")
    ingrid = [j for j in range(S.N) if S.pos_in_grid(j) is not None]
    assert whole == sorted(ingrid, key=lambda j: (S.pos_in_grid(j)[0] * ROWS + S.pos_in_grid(j)[1], j)) and len(whole) > 300
    dist = SM.descriptor_distance(c["qd"][qi["whole0"]], c["d"][whole])
    near = [whole[j] for j in np.argsort(dist, kind="stable")[:8]]
    assert sorted(near) == sorted(kp[s] for s in ("comp_x-7", "tie_x-4", "comp_y-7", "tie_y-4", "comp_y358", "tie_y364",
                                                  "comp_x486", "tie_x492")) and near[-1] == kp["tie_x492"]
    assert sorted(dist)[7] < sorted(dist)[8] and not c["taken"][near].any() and c["taken"].sum() >= 5
    assert len(area("whole_coarse")) == 8
    assert q["valid"][qi["invalid"]] == 0 and q["valid"].sum() == len(q) - 1
    assert ((c["ur"] >= 0).sum() > S.N // 3) and ((c["ur"] < 0).sum() > S.N // 3)
    # Fuse's prologue lands on the records: same pixel, radius, level window and ur, bit for bit
    f = c["flags"] != 0
    qf = P.keyframe_queries(c["scam"], 0, False, c["T"], None, c["X"], c["nrm"], c["max_d"], c["min_d"], c["flags"], TH)
    inside = (q["u"] >= BOUNDS[0]) & (q["u"] < BOUNDS[2]) & (q["v"] >= BOUNDS[1]) & (q["v"] < BOUNDS[3])
    assert np.array_equal(qf["valid"] == 1, f & inside) and (f & ~inside).sum() == 4 and (f & inside).sum() >= 28
    for name in ("valid", "u", "v", "radius", "min_level", "max_level", "ur", "level_aux"):
        assert np.array_equal(qf[name][f & inside], q[name][f & inside]), name
    assert all(qf["valid"][qi[s]] for s in ("left", "right", "top", "bottom", "on_boundaries", "cells", "whole_coarse"))


def expected():
    """The sequential reference's answers for every consumer, computed once: dict of tuples."""
    c = scene()
    if "want" in c:
        return c["want"]
    S, q, qd = c["S"], c["q"], c["qd"]
    w = {"grid": grid_csr(S), "grid_other": grid_csr(c["S_other"])}
    for ori in (True, False):
        w["frame", ori] = SM.search_by_projection_frame(S, q, qd, c["taken"], ori)
    w["points"] = SM.search_by_projection_points(S, q, qd, c["taken"], NNRATIO)
    F1 = init_frame(c)
    prev = np.stack([q["u"], q["v"]], 1).astype(f32)
    for window in (8, 600):
        w["init", window] = SM.search_for_initialization(F1, S, prev, window, 0.9, True)
    w["best", False] = P.best_in_window(S, q, qd, None)
    w["best", True] = P.best_in_window(S, q, qd, INV_SIGMA2)
    for sim3 in (False, True):
        for name, F in (("fuse", S), ("fuse_other", c["S_other"])):
            w[name, sim3] = P.fuse(F, c["scam"], c["T"], c["X"], c["nrm"], c["max_d"], c["min_d"], c["flags"], qd, TH, INV_SIGMA2, sim3)
    # the answers depend on the rules under test
    qi, kp = c["qi"], c["kp"]
    a = w["frame", False][1]
    assert a[kp["comp_x-7"]] == qi["left"] and a[kp["comp_x486"]] == qi["right"] and a[kp["edge_lo_in"]] == qi["on_boundaries"]
    assert a[kp["comp_y-7"]] == qi["top"] and a[kp["comp_y358"]] == qi["bottom"]
    whole = [qi["whole%d" % j] for j in range(N_WHOLE)]
    assert np.isin(whole, a).sum() >= 10 and w["frame", False][0] > 30 and w["points"][0] > 15
    # heads of 8 keys run out: a long list's head holds at most its eight nearest candidates not taken on entry; for the
    # later whole-grid queries every one of those is held by a query with a smaller index when their turn comes (a holder
    # is never displaced in the frame search), and they still find a match further down the list: the head must be refilled
    i0 = qi["whole0"]
    dist = SM.descriptor_distance(qd[i0], c["d"])
    order = sorted((j for j in SM.features_in_area(S, q["u"][i0], q["v"][i0], q["radius"][i0], 0, 7).tolist() if not c["taken"][j]),
                   key=lambda j: (dist[j], S.pos_in_grid(j)[0] * ROWS + S.pos_in_grid(j)[1], j))
    assert len(order) > 64 and order[7] == kp["tie_x492"] and dist[order[7]] < dist[order[8]]
    starved = [i for i in whole if (a[order[:8]] >= 0).all() and (a[order[:8]] < i).all() and (a == i).any()]
    assert len(starved) >= 6 and starved[-1] == whole[-1], starved
    assert w["init", 8][0] >= 5 and w["init", 600][0] >= 5
    for gate in (False, True):
        bi, bd = w["best", gate]
        assert bi[qi["left"]] == kp["comp_x-7"] and bd[qi["left"]] == 2
        assert bi[qi["bottom"]] == kp["tie_y364" if gate else "comp_y358"]       # 7 px off: 49 > 5.99 at level 0
        assert (bi[[qi[s] for s in ("out_left", "out_right", "out_top", "out_bottom", "radius0", "invalid")]] == -1).all()
        assert (bi >= 0).sum() > 25
    assert (w["best", False][0] != w["best", True][0]).sum() >= 3                                  # the chi-square gate bites
    assert w["fuse", True][0][qi["right"]] == kp["comp_x486"] and w["fuse", False][0][qi["right"]] == kp["tie_x492"]
    assert w["fuse", False][0][qi["left"]] == kp["comp_x-7"] and w["fuse", True][0][qi["whole_coarse"]] >= 0
    assert (w["fuse", False][0] != w["fuse", True][0]).any() and (w["fuse_other", False][0] >= 0).sum() > 15
    c["want"] = w
    return w


N_PAD = 700


def padded(c):
    """The train frame behind N_PAD more key points far outside the grid, all with the queries' own descriptor: above 1024
    key points the grid build takes its two-pass path, and PosInGrid must keep every one of them out.  Returns
    (k, d, ur, taken) and the reference's frame / points answers, which are the scene's own."""
    if "padded" not in c:
        n = len(c["k"])
        k = np.concatenate([c["k"], np.zeros(N_PAD, SM.KP_DTYPE)])
        k["x"][n:], k["y"][n:] = 5000.0 + np.arange(N_PAD), 96.0
        k["octave"][n:], k["angle"][n:], k["size"][n:], k["response"][n:], k["class_id"][n:] = 0, 10.0, 31.0, 20.0, -1
        d = np.concatenate([c["d"], np.repeat(c["base"][None, :], N_PAD, 0)])
        ur = np.concatenate([c["ur"], np.full(N_PAD, -1, f32)])
        taken = np.concatenate([c["taken"], np.zeros(N_PAD, np.uint8)])
        S = SM.Frame(k, d, ur, BOUNDS, SF)
        assert S.N > 1024 and all(S.pos_in_grid(j) is None for j in range(n, S.N))
        want = (SM.search_by_projection_frame(S, c["q"], c["qd"], taken, False),
                SM.search_by_projection_points(S, c["q"], c["qd"], taken, NNRATIO))
        w = expected()
        for got, ref in zip(want, (w["frame", False], w["points"])):
            assert got[0] == ref[0] and np.array_equal(got[1][:n], ref[1]) and (got[1][n:] == -1).all()
        c["padded"] = (k, d, ur, taken, want)
    return c["padded"]


def init_frame(c):
    """F1 of SearchForInitialization: a level-0 key point on every query centre, with the query's descriptor"""
    q = c["q"]
    k1 = np.zeros(len(q), SM.KP_DTYPE)
    k1["x"], k1["y"] = q["u"], q["v"]
    k1["octave"], k1["angle"], k1["size"], k1["response"], k1["class_id"] = 0, 10.0, 31.0, 20.0, -1
    c["k1"] = k1
    return SM.Frame(k1, c["qd"], None, BOUNDS, SF)
