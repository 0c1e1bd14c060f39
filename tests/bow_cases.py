"""Inputs shared by tests/test_seqref_bow_cpu.py (seqref against the oracle) and tests/test_seqref_bow_gpu.py (seqref
against the kernels): constructed edge cases and small random scenes for the vocabulary transform, both SearchByBoW
forms, SearchForTriangulation and ComputeDistinctiveDescriptors, plus the two float32 enumerations.  Imports seqref
only; the expected values of every case come from tests/seqref/bow.py, and the callers assert from `info` that a case
reached the branch it was built for."""
import numpy as np

from seqref import bow as B
from seqref.extractor import KP_DTYPE, tables

f32, f64 = np.float32, np.float64
NO_NODE = B.NO_NODE
SF = tables(1000, 1.2, 8)["scale"]                     # mvScaleFactors of an 8-level, 1.2 pyramid (float32)
SIGMA2 = np.array([f32(s * s) for s in SF], f32)       # mvLevelSigma2, src/ORBextractor.cc:422
BOUNDS = (0.0, 0.0, 640.0, 480.0)


def keys(n, x=0.0, y=0.0, octave=0, angle=0.0):
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["size"] = 31.0
    return k


def ones(d, first=0):
    """A descriptor with bits first .. first+d-1 set: distance d from zero."""
    bits = np.zeros(256, np.uint8)
    bits[first:first + d] = 1
    return np.packbits(bits, bitorder="little")


def far(rng, n):
    """n descriptors with bits 96..255 set and random bits below 40 only: at least 120 away from anything `ones` makes
    with fewer than 40 bits."""
    bits = np.zeros((n, 256), np.uint8)
    bits[:, 96:] = 1
    bits[:, :40] = rng.integers(0, 2, (n, 40))
    return np.packbits(bits, axis=1, bitorder="little")


# -- the two enumerations --------------------------------------------------------------------------------------

def ratio_pairs(nnratio):
    """Integer pairs (d1, d2) in 0..256 on which static_cast<float>(d1) < nnratio * static_cast<float>(d2) evaluated in
    float32 (the reference) differs from the same test with the float constant promoted to double.
    Returns [(d1, d2, accepted_in_float32)]."""
    r32 = f32(nnratio)
    out = []
    for d1 in range(257):
        for d2 in range(257):
            a32 = bool(f32(d1) < f32(r32 * f32(d2)))
            a64 = bool(f64(d1) < f64(r32) * f64(d2))
            if a32 != a64:
                out.append((d1, d2, a32))
    return out


def epipolar_edge(level, bs=tuple(range(1, 33))):
    """(b, y2), both float32, with dsqr = (b*y2)^2 / (b*b) below 3.84 * sigma2[level] in double but not below
    3.84f * sigma2[level] in float (CheckDistEpipolarLine with la = lc = 0, lb = b), or None.  For each b in turn the
    floats around sqrt(3.84 * sigma2) are tried; the first hit is returned."""
    s2 = SIGMA2[level]
    lim64 = f64(3.84) * f64(s2)
    lim32 = f32(f32(3.84) * s2)
    for b in bs:
        b = f32(b)
        y = f32(np.sqrt(lim64))
        for _ in range(8):
            y = np.nextafter(y, f32(0))
        for _ in range(16):
            num = f32(b * y)
            dsqr = f32(f32(num * num) / f32(b * b))
            if f64(dsqr) < lim64 and not dsqr < lim32:
                return b, y
            y = np.nextafter(y, f32(np.inf))
    return None


# -- vocabulary --------------------------------------------------------------------------------------------------

def chain_tree(k, L, seed, scoring=0, weighting=0, dup_at=None):
    """A full k-ary tree of depth L in breadth-first file order.  Child c of every node is its parent with 3*(c+1) bits
    flipped in a window that moves with the level, so the descent is decided by small distinct distances.  dup_at = (i, j):
    child j is an exact copy of child i everywhere (a distance tie the first must win)."""
    rng = np.random.default_rng(seed)
    parent, leaf, desc, weight = [], [], [], []
    level = [(0, rng.integers(0, 256, 32, dtype=np.uint8))]
    for depth in range(1, L + 1):
        nxt = []
        for pid, pdesc in level:
            for c in range(k):
                bits = np.unpackbits(pdesc, bitorder="little")
                src = dup_at[0] if (dup_at is not None and c == dup_at[1]) else c
                lo = (depth - 1) * 64
                bits[lo + 3 * src: lo + 3 * src + 3] ^= 1
                d = np.packbits(bits, bitorder="little")
                parent.append(pid)
                leaf.append(1 if depth == L else 0)
                desc.append(d)
                weight.append(float(rng.uniform(0.05, 12.0)) if depth == L else 0.0)
                nxt.append((len(parent), d))
        level = nxt
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=np.array(parent, np.int32),
                is_leaf=np.array(leaf, np.uint8), desc=np.stack(desc), weight=np.array(weight, f64))


def ragged_tree(scoring=0, weighting=0):
    """k = 3, L = 3, written by hand: leaves at depth 1, 2 and 3, one stopped word, interleaved file order.
    node: 1 = leaf A (depth 1), 2 = inner B, 3 = inner C, 4 = leaf of C (depth 2), 5 = inner child of B, 6 = leaf of B
    (depth 2, stopped), 7, 8 = leaves under 5 (depth 3), 9 = leaf of C."""
    d = {i: ones(0) for i in range(1, 10)}
    d[1] = ones(8, 0)
    d[2] = ones(8, 32)
    d[3] = ones(8, 64)
    d[4] = ones(8, 64) | ones(4, 100)
    d[5] = ones(8, 32) | ones(4, 120)
    d[6] = ones(8, 32) | ones(4, 140)
    d[7] = ones(8, 32) | ones(4, 120) | ones(4, 160)
    d[8] = ones(8, 32) | ones(4, 120) | ones(4, 180)
    d[9] = ones(8, 64) | ones(4, 200)
    parent = [0, 0, 0, 3, 2, 2, 5, 5, 3]
    leaf = [1, 0, 0, 1, 0, 1, 1, 1, 1]
    weight = [1.5, 0.0, 0.0, 0.25, 0.0, 0.0, 2.0, 1e-3, 7.0]
    voc = dict(k=3, L=3, scoring=scoring, weighting=weighting, parent=np.array(parent, np.int32),
               is_leaf=np.array(leaf, np.uint8), desc=np.stack([d[i] for i in range(1, 10)]), weight=np.array(weight, f64))
    # four features of one wavefront that stop at depth 1, 2 (stopped), 3, 2
    feats = np.stack([d[1], d[6], d[8], d[9], d[7], d[4], d[8]])
    return voc, feats


def tree_features(voc, rng, n):
    """n descriptors near nodes of the tree (few flipped bits), exact node copies and noise."""
    d = voc["desc"][rng.integers(0, len(voc["desc"]), n)].copy()
    flips = (rng.integers(0, 256, d.shape, dtype=np.uint8) & rng.integers(0, 256, d.shape, dtype=np.uint8)
             & rng.integers(0, 256, d.shape, dtype=np.uint8) & rng.integers(0, 256, d.shape, dtype=np.uint8))
    d ^= flips * (rng.random((n, 1)) < 0.6).astype(np.uint8)
    noise = rng.random(n) < 0.1
    d[noise] = rng.integers(0, 256, (int(noise.sum()), 32), dtype=np.uint8)
    return d


def seq_voc(voc):
    return B.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["parent"], voc["is_leaf"], voc["desc"],
                         voc["weight"])


# -- SearchByBoW ---------------------------------------------------------------------------------------------------

def bow_case(k1, d1, n1, k2, d2, n2, nnratio, good1=None, good2=None, check_ori=True, name=""):
    return dict(name=name, k1=k1, d1=np.ascontiguousarray(d1, np.uint8).reshape(-1, 32), n1=np.asarray(n1, np.uint32), k2=k2,
                d2=np.ascontiguousarray(d2, np.uint8).reshape(-1, 32), n2=np.asarray(n2, np.uint32), nnratio=nnratio,
                good1=good1, good2=good2, check_ori=check_ori)


def bow_expected(case, form, info=None):
    """(nmatches, matches12[n1]) of the product's single entry from the reference form `form`:
    "frame": SearchByBoW(KeyFrame*, Frame&) = max_dist 50, valid1 = good1, blocked2 = none; its vpMapPointMatches is the
             inverse of matches12.  "kf": SearchByBoW(KeyFrame*, KeyFrame*) = max_dist 49, blocked2 = !good2."""
    c = case
    if form == "frame":
        n, m = B.search_by_bow_kf_frame(c["k1"], c["d1"], c["n1"], c["good1"], c["k2"], c["d2"], c["n2"], c["nnratio"],
                                        c["check_ori"], info)
        m12 = np.full(len(c["d1"]), -1, np.int32)
        for iF, iKF in enumerate(m.tolist()):
            if iKF >= 0:
                assert m12[iKF] == -1
                m12[iKF] = iF
        return n, m12
    return B.search_by_bow_kf_kf(c["k1"], c["d1"], c["n1"], c["good1"], c["k2"], c["d2"], c["n2"], c["good2"], c["nnratio"],
                                 c["check_ori"], info)


def bow_entry_args(case, form):
    """(valid1, blocked2, max_dist) for the product's / the oracle's single entry."""
    v1 = None if case["good1"] is None else np.asarray(case["good1"], np.uint8)
    if form == "frame":
        return v1, None, 50
    return v1, (None if case["good2"] is None else (1 - np.asarray(case["good2"], np.uint8)).astype(np.uint8)), 49


def bow_list_case(L, p, seed=0):
    """One node; L candidates; the winner of query 0 (distance 5) sits at list position p, query 1 prefers the same slot
    (distance 6) and has to fall back to the runner-up (distance 20, at position 0 unless p == 0); query 2 sees only the
    far ones.  Expected: 0 -> p, 1 -> runner-up (or nothing when L == 1), 2 -> nothing."""
    rng = np.random.default_rng(seed + L)
    d2 = far(rng, L)
    d2[p] = ones(5)
    if L > 1:
        d2[0 if p else 1] = ones(20)
    d1 = np.stack([ones(0), ones(1, 250), far(rng, 1)[0] ^ ones(70, 150)])
    return bow_case(keys(3), d1, [7, 7, 7], keys(L), d2, [7] * L, 0.7, name="list%d@%d" % (L, p))


def bow_duplicate_case(nnratio):
    """Exact duplicate candidates at distance 10: the lower index is the best, bestDist2 == bestDist1."""
    d2 = np.stack([far(np.random.default_rng(1), 1)[0], ones(10), ones(10)])
    return bow_case(keys(1), [ones(0)], [3], keys(3), d2, [3, 3, 3], nnratio, name="dup%g" % nnratio)


def bow_threshold_case():
    """Three nodes, one query and one candidate each (bestDist2 = 256), at distances 49, 50, 51; a fourth node exists on
    side 1 only, a fifth on side 2 only, and one key point per side is in no list."""
    d1 = np.stack([ones(0)] * 5)
    d2 = np.stack([ones(49), ones(50), ones(51), ones(3), ones(2)])
    return bow_case(keys(5), d1, [10, 20, 30, 25, NO_NODE], keys(5), d2, [10, 20, 30, 35, NO_NODE], 0.9, name="th")


def bow_ratio_case(nnratio, max_d1=49):
    """One node per float32-deciding pair (d1, d2) with d1 <= max_d1: candidates at exactly d1 and d2.  case["pairs"] =
    [(d1, d2, accepted by the reference)], three pairs on which float32 and float64 agree included."""
    pairs = [(a, b, acc) for a, b, acc in ratio_pairs(nnratio) if a <= max_d1 and b <= 200]
    pairs += [(15, 25, True), (3, 6, True), (30, 31, False)]      # both precisions agree on these
    d1, d2, n1, n2 = [], [], [], []
    for j, (a, b, _) in enumerate(pairs):
        d1.append(ones(0))
        n1.append(100 + j)
        d2 += [ones(b, 40), ones(a)]          # the second best first
        n2 += [100 + j, 100 + j]
    c = bow_case(keys(len(d1)), d1, n1, keys(len(d2)), d2, n2, nnratio, name="ratio%g" % nnratio)
    c["pairs"] = pairs
    return c


def bow_cull_case():
    """12 matches in rotation bin 0 and one in bin 5 (150 degrees) that takes slot s = 12; the next query (bin 0) prefers
    s too and is left with its runner-up slot 13.  The cull then frees s: expected 12 -> -1, 13 -> 13, 14 matches - 1."""
    d1 = [ones(0) | ones(2, 8 * j + 64) for j in range(12)]
    d2 = [ones(0) | ones(2, 8 * j + 64) | ones(1, 8 * j + 66) for j in range(12)]
    n1 = [50 + j for j in range(12)]
    n2 = list(n1)
    d1 += [ones(4, 200), ones(5, 200)]
    n1 += [99, 99]
    d2 += [ones(4, 200), ones(5, 200) | ones(12, 220)]       # slot 12: distance 0 / 1; slot 13: 13 / 12
    n2 += [99, 99]
    k1 = keys(14)
    k1["angle"][12] = 150.0
    return bow_case(k1, d1, n1, keys(14), d2, n2, 0.95, name="cull")


def bow_random_case(rng, n1, n2, n_nodes, nnratio=0.75, flags=True, check_ori=True, name="random", big_ids=False):
    """Noisy copies of a few base descriptors pressed into n_nodes nodes (plus nodes on one side only and NO_NODE
    entries): distances from 0 to far beyond TH_LOW, exact duplicates, chains of blocked slots, every rotation bin."""
    base = rng.integers(0, 256, (max(4, (n1 + n2) // 6), 32), dtype=np.uint8)

    def side(n, only):
        bi = rng.integers(0, len(base), n)
        d = base[bi].copy()
        fl = (rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8)
              & rng.integers(0, 256, (n, 32), dtype=np.uint8))
        d ^= fl * (rng.random((n, 1)) < 0.7).astype(np.uint8)
        node = (np.where(rng.random(n) < 0.8, bi % n_nodes, rng.integers(0, n_nodes, n)) * 7 + 3).astype(np.uint32)
        node[rng.random(n) < 0.06] = only
        node[rng.random(n) < 0.05] = NO_NODE
        k = keys(n, rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.integers(0, 8, n),
                 rng.choice([0.0, 3.0, 15.0, 45.0, 135.0, 255.0, 359.5], n, p=[.45, .2, .1, .1, .05, .05, .05]))
        return k, d, node
    k1, d1, node1 = side(n1, 1)
    k2, d2, node2 = side(n2, 2)
    if big_ids:        # node ids above 2^31 (NodeId is unsigned); side 1 also ends on a node side 2 does not have
        node1[node1 == 3], node2[node2 == 3] = 0xF0000000, 0xF0000000
        node1[0] = 0xFFFFFFF0
    g1 = (rng.random(n1) < 0.85).astype(np.uint8) if flags else None
    g2 = (rng.random(n2) < 0.8).astype(np.uint8) if flags else None
    return bow_case(k1, d1, node1, k2, d2, node2, nnratio, g1, g2, check_ori, name)


def bow_group_case(N, seed=40):
    """One node whose query group has exactly N surviving queries (a real node id and valid1 set), next to four queries that
    do not survive (two without a map point, two in no list).  Query j is a random descriptor of its own and candidate
    perm[j] copies it with three bits flipped (random descriptors lie about 128 apart), so every query has one decisive
    match: expected matches12[j] = perm[j] for the survivors, -1 for the others.  case["group"] = N."""
    rng = np.random.default_rng(seed + N)
    n1, n2 = N + 4, N + 6
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    node1 = np.full(n1, 7, np.uint32)
    good1 = np.ones(n1, np.uint8)
    out = [3, N // 2, N + 1, N + 3]                  # scattered, so the survivors are not a prefix of the frame
    good1[out[:2]] = 0
    node1[out[2:]] = NO_NODE
    alive = [j for j in range(n1) if j not in out]
    perm = rng.permutation(n2)
    d2 = far(rng, n2)
    expected = np.full(n1, -1, np.int32)
    for j, slot in zip(alive, perm):
        d2[slot] = d1[j] ^ ones(3, 100)
        expected[j] = slot
    c = bow_case(keys(n1), d1, node1, keys(n2), d2, [7] * n2, 0.7, good1=good1, name="exact%d" % N)
    c["group"], c["expected_m12"] = N, expected
    return c


def bow_flags_case():
    """The map-point flags, by hand.  Query 0 has no good map point and is skipped although candidate 0 equals it; query 1 is
    2 away from candidate 0, 8 from candidate 1 and 30 from candidate 2.  SearchByBoW(KeyFrame*, Frame&) has no side-2 flag:
    query 1 takes candidate 0 (2 < 0.7 * 8).  In SearchByBoW(KeyFrame*, KeyFrame*) candidate 0 has no good map point, so the
    runner-up wins: candidate 1 (8 < 0.7 * 30)."""
    d1 = [ones(0), ones(2, 60)]
    d2 = [ones(0), ones(2, 60) | ones(8, 70), ones(2, 60) | ones(30, 80)]
    c = bow_case(keys(2), d1, [9, 9], keys(3), d2, [9, 9, 9], 0.7, good1=np.array([0, 1], np.uint8),
                 good2=np.array([0, 1, 1], np.uint8), name="flags")
    return c


def bow_constructed_cases():
    cs = [bow_list_case(L, p) for L, p in ((1, 0), (63, 62), (64, 63), (65, 64), (128, 63), (129, 64), (129, 128))]
    cs += [bow_duplicate_case(r) for r in (0.6, 1.0, 1.5)]
    cs += [bow_threshold_case(), bow_ratio_case(0.6), bow_ratio_case(0.8), bow_cull_case(), bow_flags_case()]
    cs += [bow_group_case(N) for N in (64, 65, 129)]
    return cs


def bow_random_cases():
    rng = np.random.default_rng(2024)
    return [bow_random_case(rng, 64, 70, 1, name="crowded_a"), bow_random_case(rng, 65, 70, 1, name="crowded_b"),
            bow_random_case(rng, 129, 140, 1, name="crowded_c"), bow_random_case(rng, 300, 280, 40, name="nodes40"),
            bow_random_case(rng, 200, 220, 5, 0.9, flags=False, check_ori=False, name="noflags"),
            bow_random_case(rng, 300, 300, 150, 0.8, name="sparse", big_ids=True)]


# -- SearchForTriangulation ------------------------------------------------------------------------------------------

F_HORIZONTAL = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)     # la = 0, lb = 1, lc = -y1: the line y2 = y1
F_EDGE = np.array([[0, 1, 0], [0, 0, 0], [0, 0, 0]], f32)            # la = lc = 0, lb = x1: num = x1 * y2


def tri_case(k1, d1, n1, k2, d2, n2, F12, epipole=(1e4, 1e4), free1=None, free2=None, ur1=None, ur2=None,
             only_stereo=False, check_ori=False, name="", pose=None):
    """pose: the camera pair that produces this geometry, "side" (camera 2 moved sideways: horizontal lines, epipole at
    infinity) or "ahead" (moved straight ahead: lines through the epipole = the principal point), None where no pair does."""
    return dict(name=name, pose=pose, k1=k1, d1=np.ascontiguousarray(d1, np.uint8).reshape(-1, 32), n1=np.asarray(n1, np.uint32), k2=k2,
                d2=np.ascontiguousarray(d2, np.uint8).reshape(-1, 32), n2=np.asarray(n2, np.uint32),
                F12=np.asarray(F12, f32).reshape(3, 3), ex=f32(epipole[0]), ey=f32(epipole[1]), free1=free1, free2=free2,
                ur1=None if ur1 is None else np.asarray(ur1, f32), ur2=None if ur2 is None else np.asarray(ur2, f32),
                only_stereo=only_stereo, check_ori=check_ori)


def tri_expected(c, info=None):
    return B.search_for_triangulation(c["k1"], c["d1"], c["n1"], c["free1"], c["ur1"], c["k2"], c["d2"], c["n2"], c["free2"],
                                      c["ur2"], c["F12"], c["ex"], c["ey"], SIGMA2, SF, c["only_stereo"], c["check_ori"], info)


def tri_count_case(L, seed=3):
    """L >= 3 candidates in the query's node, all on the line y2 = y1 = 100: far ones, then distances 40, 30, 30 at the last
    three positions.  The tie at 30: the later passes the gates, so the last wins (index L - 1); the second query is a copy
    of the first and takes the same candidate."""
    rng = np.random.default_rng(seed + L)
    d2 = far(rng, L)
    d2[L - 3], d2[L - 2], d2[L - 1] = ones(40), ones(30, 1), ones(30)
    k2 = keys(L, 50.0 + np.arange(L), 100.0)
    c = tri_case(keys(2, 300.0, 100.0), [ones(0), ones(0)], [5, 5], k2, d2, [5] * L, F_HORIZONTAL, name="count%d" % L, pose="side")
    c["expected_m12"] = np.array([L - 1, L - 1])
    return c


def tri_tie_case():
    """Equal distances 20, 20.  Query 0 (y1 = 100): the later candidate is on the line, so the last wins (index 1).
    Query 1 (y1 = 200): the later one (y2 = 100) fails the epipolar gate, the earlier (y2 = 200) stays (index 2).
    Query 2 (y1 = 300, node 8): the later equal candidate is inside the epipole gate, the earlier stays (index 4)."""
    k1 = keys(3, 300.0, [100.0, 200.0, 300.0])
    k2 = keys(6, [10.0, 20.0, 30.0, 40.0, 50.0, 500.0], [100.0, 100.0, 200.0, 100.0, 300.0, 300.0])
    d2 = [ones(20, 0), ones(20, 1), ones(20, 2), ones(20, 3), ones(20, 4), ones(20, 5)]
    return tri_case(k1, [ones(0)] * 3, [6, 7, 8], k2, d2, [6, 6, 7, 7, 8, 8], F_HORIZONTAL, epipole=(503.0, 304.0), name="tie", pose="side")


def tri_threshold_case():
    """bestDist starts at TH_LOW and the skip is dist > TH_LOW || dist > bestDist, by hand; everything lies on the line.
    Query 0: candidates at 51 (skipped) and 50 (kept): index 1.  Query 1: one candidate at 51: nothing.  Query 2: 50 and 50:
    the second equals bestDist and replaces it: index 4."""
    k2 = keys(5, [10.0, 20.0, 30.0, 40.0, 50.0], 100.0)
    d2 = [ones(51), ones(50), ones(51), ones(50), ones(50, 3)]
    c = tri_case(keys(3, 300.0, 100.0), [ones(0)] * 3, [1, 2, 3], k2, d2, [1, 1, 2, 3, 3], F_HORIZONTAL, name="th_low", pose="side")
    c["expected_m12"] = np.array([1, -1, 4])
    return c


def tri_epipole_case(stereo):
    """The epipole gate distex^2 + distey^2 < 100 * sf[level] is strict.  Level 0: the candidate at x = 330 is at squared
    distance exactly 100 = 100 * sf[0] and is kept, the next float32 towards the epipole is skipped; only this level sits
    exactly on the limit.  Level 2: 100 * sf[2] is no square of a float32 difference, so the smallest x whose squared
    distance is not below the limit is searched for (kept) and paired with the float32 below it (skipped).
    stereo: None, 1 or 2 = which side carries u_right >= 0 (gate off: all four match)."""
    ex, ey = f32(320.0), f32(100.0)
    xs, octs = [], []
    for level in (0, 2):
        lim = f32(f32(100) * SF[level])
        x = f32(ex + f32(np.sqrt(f64(lim))))
        # walk to the smallest x whose squared distance is not below the limit
        def sq(v):
            dx = f32(ex - v)
            return f32(dx * dx)
        while sq(x) < lim:
            x = np.nextafter(x, f32(np.inf))
        while not sq(np.nextafter(x, f32(0))) < lim:
            x = np.nextafter(x, f32(0))
        xs += [x, np.nextafter(x, f32(0))]
        octs += [level, level]
    n = len(xs)
    k1 = keys(n, 20.0, 100.0)
    k2 = keys(n, xs, 100.0, octs)
    ur1 = np.full(n, -1.0, f32)
    ur2 = np.full(n, -1.0, f32)
    if stereo == 1:
        ur1[:] = 5.0
    if stereo == 2:
        ur2[:] = 5.0
    node = np.arange(n) + 40
    c = tri_case(k1, [ones(0)] * n, node, k2, [ones(7)] * n, node, F_HORIZONTAL, epipole=(ex, ey), ur1=ur1, ur2=ur2,
                 name="epipole%s" % stereo, pose="ahead")
    c["expected_m12"] = np.arange(n) if stereo else np.array([0, -1, 2, -1])
    return c


def tri_uright_case(only_stereo):
    """mvuRight >= 0 decides bStereo: -0.0 and 0.0 are stereo, the largest negative float32 is monocular.  Every candidate
    lies inside the epipole gate, so only pairs with a stereo side survive; with only_stereo both sides must be stereo."""
    vals = np.array([-0.0, 0.0, -np.finfo(f32).smallest_subnormal, -1.0], f32)
    n = len(vals)
    k1 = keys(n * n, 20.0, 100.0)
    k2 = keys(n * n, 321.0, 100.0)
    ur1 = np.repeat(vals, n)
    ur2 = np.tile(vals, n)
    node = np.arange(n * n) + 60
    return tri_case(k1, [ones(0)] * (n * n), node, k2, [ones(3)] * (n * n), node, F_HORIZONTAL, epipole=(320.0, 100.0), ur1=ur1,
                    ur2=ur2, only_stereo=only_stereo, name="uright%d" % only_stereo, pose="ahead")


EDGE_LEVELS = (0, 1, 2, 4, 5, 6, 7)


def tri_epipolar_edge_case():
    """Per level in EDGE_LEVELS one node with three candidates at equal descriptor distance, in list order: the next float32
    below the y2 of epipolar_edge (passes), that y2 (passes the reference's double comparison, fails a float one) and the
    next float32 above (fails).  Equal distances: the last that passes wins, so the reference answers the middle one and a
    float gate the first."""
    k1x, k2y, octs, n1, n2 = [], [], [], [], []
    for j, level in enumerate(EDGE_LEVELS):
        b, y = epipolar_edge(level)
        k1x.append(b)
        k2y += [np.nextafter(y, f32(0)), y, np.nextafter(y, f32(np.inf))]
        octs += [level] * 3
        n1.append(80 + j)
        n2 += [80 + j] * 3
    n = len(EDGE_LEVELS)
    k1 = keys(n, np.array(k1x, f32), 44.0)
    k2 = keys(3 * n, 10.0, np.array(k2y, f32), octs)
    c = tri_case(k1, [ones(0)] * n, n1, k2, [ones(9)] * (3 * n), n2, F_EDGE, name="epipolar_edge")
    c["expected_m12"] = 3 * np.arange(n) + 1
    return c


def tri_epipolar_edge_pose_case(level):
    """The same edge for one level, in a geometry a camera pair produces: camera 2 moved sideways by tx = b * fy with
    fy = 256 (1 / fy exact) gives F12 = [[0, 0, 0], [0, 0, b], [0, -b, 0]] exactly, so a query at y1 = 0 has la = 0, lb = -b,
    lc = 0 and num = -b * y2, whose square is that of b * y2.  Three candidates as above: expected index 1."""
    b, y = epipolar_edge(level)
    k2 = keys(3, 10.0, np.array([np.nextafter(y, f32(0)), y, np.nextafter(y, f32(np.inf))], f32), level)
    F = np.array([[0, 0, 0], [0, 0, b], [0, -b, 0]], f32)
    c = tri_case(keys(1, 33.0, 0.0), [ones(0)], [80], k2, [ones(9)] * 3, [80] * 3, F, name="edge_pose%d" % level, pose="side")
    c["tx"], c["fy"], c["expected_m12"] = float(b) * 256.0, 256.0, np.array([1])
    return c


def tri_zero_f_case():
    """F12 of zeros: den == 0 rejects every candidate."""
    return tri_case(keys(2, 5.0, 5.0), [ones(0)] * 2, [1, 1], keys(3, 9.0, 9.0), [ones(1)] * 3, [1, 1, 1], np.zeros((3, 3), f32),
                    name="zeroF")


F_FORWARD = np.array([[0, 1, -240], [-1, 0, 320], [240, -320, 0]], f32)   # forward motion: lines through (320, 240)


def tri_random_case(rng, n1, per, n_nodes, only_stereo=False, check_ori=True, name="tri_random", tail=False):
    """Forward motion, epipole (320, 240) in image 2: the epipolar line of a query passes through the epipole and the query's
    own position.  Each candidate copies a query's descriptor with exactly 0 .. 60 flipped bits (so equal distances occur)
    and lies on that query's line at a random fraction of its distance from the epipole (the small fractions fall inside the
    epipole gate), pushed sideways by about the width of the epipolar gate.  Three queries sit on the epipole: den == 0."""
    n2 = n1 * per
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    x1, y1 = rng.uniform(20, 620, n1).round(1), rng.uniform(20, 460, n1).round(1)
    x1[:3], y1[:3] = 320.0, 240.0
    node1 = (rng.integers(0, n_nodes, n1) * 7 + 3).astype(np.uint32)
    d1[5], x1[5], y1[5], node1[5] = d1[4], x1[4], y1[4], node1[4]      # a twin query: both may take the same candidate
    k1 = keys(n1, x1, y1, rng.integers(0, 8, n1), rng.choice([0.0, 3.0, 45.0, 135.0, 359.5], n1, p=[.5, .2, .1, .1, .1]))
    src = rng.integers(0, n1, n2)
    src[:6] = [0, 0, 1, 1, 2, 2]
    bits = np.unpackbits(d1[src], axis=1)
    for j, nb in enumerate(rng.choice([0, 0, 5, 20, 20, 45, 50, 51, 60], n2)):
        bits[j, rng.permutation(256)[:nb]] ^= 1
    d2 = np.packbits(bits, axis=1)
    oct2 = rng.integers(0, 8, n2)
    s = rng.choice([0.01, 0.03, 0.5, 0.9, 1.2], n2)
    dx, dy = x1[src] - 320.0, y1[src] - 240.0
    nrm = np.maximum(np.hypot(dx, dy), 1e-9)
    side = rng.normal(0, 1.5, n2) * SF[oct2]
    x2 = 320.0 + s * dx - dy / nrm * side
    y2 = 240.0 + s * dy + dx / nrm * side
    k2 = keys(n2, x2, y2, oct2, rng.choice([0.0, 3.0, 45.0], n2, p=[.7, .2, .1]))
    node2 = node1[src].copy()
    other = rng.random(n2) < 0.1
    node2[other] = (rng.integers(0, n_nodes, int(other.sum())) * 7 + 3).astype(np.uint32)
    node1[rng.random(n1) < 0.05], node2[rng.random(n2) < 0.05] = 1, 2
    node1[rng.random(n1) < 0.05], node2[rng.random(n2) < 0.05] = NO_NODE, NO_NODE
    if tail:
        node1[6] = 0xFFFFFFF0                    # side 1 ends on a node (above 2^31) that side 2 does not have
    ur1 = np.where(rng.random(n1) < 0.35, x1 - 10, -1).astype(f32)
    ur2 = np.where(rng.random(n2) < 0.35, x2 - 10, -1).astype(f32)
    return tri_case(k1, d1, node1, k2, d2, node2, F_FORWARD, epipole=(320.0, 240.0),
                    free1=(rng.random(n1) < 0.85).astype(np.uint8), free2=(rng.random(n2) < 0.85).astype(np.uint8), ur1=ur1,
                    ur2=ur2, only_stereo=only_stereo, check_ori=check_ori, name=name, pose="ahead")


def tri_constructed_cases():
    return ([tri_count_case(L) for L in (63, 64, 65, 129)] + [tri_tie_case()] +
            [tri_epipole_case(s) for s in (None, 1, 2)] + [tri_uright_case(False), tri_uright_case(True),
                                                           tri_epipolar_edge_case(), tri_zero_f_case(), tri_threshold_case()] +
            [tri_epipolar_edge_pose_case(level) for level in EDGE_LEVELS])


def tri_random_cases():
    rng = np.random.default_rng(77)
    return [tri_random_case(rng, 120, 4, 6, name="tri_a"), tri_random_case(rng, 120, 4, 6, only_stereo=True, name="tri_os"),
            tri_random_case(rng, 40, 8, 2, check_ori=False, name="tri_b", tail=True)]


# -- ComputeDistinctiveDescriptors -----------------------------------------------------------------------------------

def distinctive_lists():
    """Lists of 1, 2, 3, 4, 63, 64, 65, 129 and 2048 descriptors drawn from few base descriptors, so that exact duplicates
    and equal medians occur."""
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    lists = []
    for N in (1, 2, 3, 4, 63, 64, 65, 129, 2048):
        d = base[rng.integers(0, len(base), N)].copy()
        fl = (rng.integers(0, 256, (N, 32), dtype=np.uint8) & rng.integers(0, 256, (N, 32), dtype=np.uint8)
              & rng.integers(0, 256, (N, 32), dtype=np.uint8))
        d ^= fl * (rng.random((N, 1)) < 0.3).astype(np.uint8)
        lists.append(d)
    # equal medians written by hand: rows 1 and 2 are the same descriptor, both have the least median; the first wins
    lists.append(np.stack([ones(40), ones(4), ones(4), ones(0)]))
    return lists


# -- transform cases ---------------------------------------------------------------------------------------------------

def transform_cases():
    """[(name, voc, features, levelsups)] for ORBVocabulary.transform: the trees, feature counts and weights at which the
    descent and the BowVector assembly take another path."""
    rng = np.random.default_rng(99)
    cases = []
    for k, L, dup in ((1, 4, None), (2, 4, None), (16, 2, None), (17, 2, (15, 16)), (20, 2, (15, 16))):
        voc = chain_tree(k, L, seed=10 * k + L, dup_at=dup)
        feats = tree_features(voc, rng, 150)
        if k > 16:          # exact copies of the leaves under children 15 .. k-1: the duplicate pair and minima in round two
            kids = np.nonzero(voc["parent"] == 1)[0][15:]
            feats = np.concatenate([feats, voc["desc"][kids], voc["desc"][15:k]])
        cases.append(("k%d_L%d" % (k, L), voc, feats, (0, 1, L - 1, L, L + 3)))
    voc, feats = ragged_tree()
    cases.append(("ragged", voc, feats, (0, 1, 2, 3, 6)))
    voc = chain_tree(4, 3, seed=5)
    pool = tree_features(voc, rng, 2049)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049):
        cases.append(("n%d" % n, voc, pool[:n], (1,)))
    # more than 1500 features in one word, weights over six decades: the order of the fp64 sums decides the bits
    voc = chain_tree(4, 2, seed=6)
    voc["weight"] = np.where(voc["is_leaf"] == 1, 10.0 ** rng.uniform(-3, 3, len(voc["weight"])), 0.0)
    leaf = voc["desc"][len(voc["desc"]) - 7]
    feats = np.concatenate([np.repeat(leaf[None], 1600, 0), tree_features(voc, rng, 300)])
    feats = feats[rng.permutation(len(feats))]
    for scoring in (0, 1, 5):
        cases.append(("heavy_word_s%d" % scoring, dict(voc, scoring=scoring), feats, (1,)))
    # every reached word is stopped
    voc = chain_tree(2, 2, seed=7)
    voc["weight"][:] = 0.0
    cases.append(("all_stopped", voc, tree_features(voc, rng, 40), (0, 1)))
    return cases


def typed_vocabulary(scoring, weighting):
    """One small ragged tree (helpers.make_vocabulary) for the scoring x weighting sweep."""
    from helpers import make_vocabulary
    return make_vocabulary(4, 3, seed=17, scoring=scoring, weighting=weighting, irregular=True, order="interleaved", stop_frac=0.15)


def typed_features():
    voc = typed_vocabulary(0, 0)
    return tree_features(voc, np.random.default_rng(3), 300)
