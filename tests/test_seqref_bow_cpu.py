"""tests/seqref/bow.py (the vocabulary transform, both SearchByBoW forms, SearchForTriangulation) on the CPU:

1. against cases worked by hand from the reference text: the expected values are written out here,
2. against the oracle, bit for bit, on the constructed cases of tests/bow_cases.py and on random scenes that are asserted
   (from the `info` counters) to take every way out of every loop,
3. the two enumerations that decide where float32 and float64 evaluation of a gate part: the ratio test
   (src/ORBmatcher.cc:230, :600) and the epipolar gate (src/ORBmatcher.cc:156).

A disagreement between seqref and the oracle means that one of them misreads the reference."""
import numpy as np
import pytest

import bow_cases as Cs
from helpers import write_vocabulary
from seqref import bow as B

f32, f64 = np.float32, np.float64
NO = B.NO_NODE
KEYS = ("word_id", "word_weight", "node_id", "bow_ids", "bow_vals")
DTYPES = dict(word_id=np.uint32, word_weight=np.float64, node_id=np.uint32, bow_ids=np.uint32, bow_vals=np.float64)


def same(a, b, what=""):
    for key in KEYS:
        assert a[key].dtype == b[key].dtype == DTYPES[key], (what, key, a[key].dtype, b[key].dtype)
        assert np.array_equal(a[key].view(np.uint64) if key in ("word_weight", "bow_vals") else a[key],
                              b[key].view(np.uint64) if key in ("word_weight", "bow_vals") else b[key]), (what, key)


# -- 1. hand-worked ----------------------------------------------------------------------------------------------------

def test_load_text_header_limits_children_order_and_word_ids(tmp_path):
    voc, _ = Cs.ragged_tree()
    path = write_vocabulary(tmp_path / "v.txt", voc)
    text = open(path).read().split("\n")
    # a blank line in the middle and two at the end: skipped
    open(path, "w").write("\n".join(text[:4] + [""] + text[4:]) + "\n\n")
    v = B.load_text(path)
    assert (v.k, v.L, v.scoring, v.weighting) == (3, 3, 0, 0)
    assert v.children == [[1, 2, 3], [], [5, 6], [4, 9], [], [7, 8], [], [], [], []]     # order of appearance, not id order
    assert v.words == [1, 4, 6, 7, 8, 9]                                                  # order of leaf appearance
    assert v.word_id == [None, 0, None, None, 1, None, 2, 3, 4, 5]
    assert v.weight[8] == 1e-3 and v.weight[9] == 7.0 and np.array_equal(v.desc[7], voc["desc"][6])
    p = tmp_path / "h.txt"
    for head, ok in (("21 3 0 0", False), ("-1 3 0 0", False), ("10 11 0 0", False), ("10 0 0 0", False), ("10 3 6 0", False),
                     ("10 3 -1 0", False), ("10 3 0 4", False), ("10 3 0 -1", False), ("20 10 5 3", True), ("0 1 0 0", True)):
        p.write_text(head + "\n")
        got = B.load_text(p)
        assert (got is not None) == ok, head                                              # :1359
        if ok:
            assert got.empty() and len(B.transform(got, np.zeros((3, 32), np.uint8))["bow_ids"]) == 0   # :1134
    # a descriptor element is cast to unsigned char (FORB.cpp:132)
    p.write_text("2 1 0 0\n0 1 " + " ".join(["257"] * 32) + " 0.5\n")
    assert np.array_equal(B.load_text(p).desc[1], np.ones(32, np.uint8))


def test_transform_hand_worked():
    voc, feats = Cs.ragged_tree()
    v = Cs.seq_voc(voc)
    # features: leaf 1 (depth 1), leaf 6 (stopped), leaf 8 (depth 3), leaf 9 (depth 2), leaf 7, leaf 4, leaf 8 again
    words = [0, 2, 4, 5, 3, 1, 4]
    weights = [1.5, 0.0, 1e-3, 7.0, 2.0, 0.25, 1e-3]
    nodes = {0: [1, NO, 8, 9, 7, 4, 8],       # nid_level 3: the leaves at depth 1 and 2 report themselves (DESIGN.md choice)
             1: [1, NO, 5, 9, 5, 4, 5],       # nid_level 2
             2: [1, NO, 2, 3, 2, 3, 2],       # nid_level 1
             3: [0, NO, 0, 0, 0, 0, 0],       # nid_level 0: the root
             6: [0, NO, 0, 0, 0, 0, 0]}       # nid_level < 0
    s = (((1.5 + 0.25) + 2.0) + (1e-3 + 1e-3)) + 7.0                  # L1 norm in ascending word order
    for levelsup, nd in nodes.items():
        r = B.transform(v, feats, levelsup)
        assert r["word_id"].tolist() == words and r["word_weight"].tolist() == weights
        assert r["node_id"].tolist() == nd, levelsup
        assert r["bow_ids"].tolist() == [0, 1, 3, 4, 5]                # word 2 is stopped: in neither vector
        assert r["bow_vals"].tolist() == [1.5 / s, 0.25 / s, 2.0 / s, (1e-3 + 1e-3) / s, 7.0 / s]
        for key in KEYS:
            assert r[key].dtype == DTYPES[key]
    # dot product: divided by v.size() = 5 entries, not normalised (:1164-1170)
    r = B.transform(Cs.seq_voc(dict(voc, scoring=B.DOT_PRODUCT)), feats, 1)
    assert r["bow_vals"].tolist() == [1.5 / 5.0, 0.25 / 5.0, 2.0 / 5.0, (1e-3 + 1e-3) / 5.0, 7.0 / 5.0]
    # TF with L1: the same accumulation; with a normalising score there is no division by v.size()
    r = B.transform(Cs.seq_voc(dict(voc, weighting=B.TF)), feats, 1)
    assert r["bow_vals"].tolist() == [1.5 / s, 0.25 / s, 2.0 / s, (1e-3 + 1e-3) / s, 7.0 / s]
    # IDF and BINARY: addIfNotExist keeps the first value of word 4; dot product does not divide here (:1173-1191)
    s1 = (((1.5 + 0.25) + 2.0) + 1e-3) + 7.0
    for weighting in (B.IDF, B.BINARY):
        r = B.transform(Cs.seq_voc(dict(voc, weighting=weighting)), feats, 1)
        assert r["bow_vals"].tolist() == [1.5 / s1, 0.25 / s1, 2.0 / s1, 1e-3 / s1, 7.0 / s1]
        r = B.transform(Cs.seq_voc(dict(voc, weighting=weighting, scoring=B.DOT_PRODUCT)), feats, 1)
        assert r["bow_vals"].tolist() == [1.5, 0.25, 2.0, 1e-3, 7.0]
    # L2: the square root of the squares summed in ascending word order
    s2 = float(np.sqrt((((1.5 * 1.5 + 0.25 * 0.25) + 2.0 * 2.0) + 2e-3 * 2e-3) + 7.0 * 7.0))
    r = B.transform(Cs.seq_voc(dict(voc, scoring=B.L2_NORM)), feats, 1)
    assert r["bow_vals"].tolist() == [1.5 / s2, 0.25 / s2, 2.0 / s2, 2e-3 / s2, 7.0 / s2]
    # every reached word stopped
    r = B.transform(v, feats[[1, 1]], 1)
    assert r["bow_ids"].size == 0 and r["node_id"].tolist() == [NO, NO] and r["word_id"].tolist() == [2, 2]


def test_descent_takes_the_first_of_equal_children():
    d = Cs.ones(9)
    v = B.from_arrays(3, 1, 0, 0, [0, 0, 0], [1, 1, 1], [Cs.ones(12), d, d], [1.0, 2.0, 3.0])
    assert B.transform_feature(v, Cs.ones(9) | Cs.ones(1, 100), 0) == (1, 2.0, 2)      # distances 5, 1, 1: strict "<"
    assert B.transform_feature(v, Cs.ones(12), 1) == (0, 1.0, 0)


@pytest.mark.parametrize("case", Cs.bow_constructed_cases(), ids=lambda c: c["name"])
def test_search_by_bow_hand_worked(case):
    name = case["name"]
    for form in ("frame", "kf"):
        info = {}
        n, m12 = Cs.bow_expected(case, form, info)
        m12 = m12.tolist()
        if name.startswith("list"):
            L, p = (int(t) for t in name[4:].split("@"))
            assert m12 == [p, (0 if p else 1) if L > 1 else -1, -1] and n == (2 if L > 1 else 1)
            assert info["blocked2"] >= 2                      # query 1 met the taken slot, query 2 both of them
            assert info.get("over_th", 0) + info.get("no_candidate", 0) >= 1
        elif name.startswith("dup"):
            assert m12 == ([1] if case["nnratio"] == 1.5 else [-1])        # the lower index of the pair; 10 < r * 10
            assert info["new_second"] == 1                                  # bestDist2 == bestDist1 came from the twin
        elif name == "th":
            assert m12 == ([0, 1, -1, -1, -1] if form == "frame" else [0, -1, -1, -1, -1])     # <= 50 against < 50
            assert info["common_node"] == 3 and info["skip_side1"] == 1
        elif name.startswith("ratio"):
            deciding = {(a, b) for a, b, _ in Cs.ratio_pairs(case["nnratio"])}
            assert len([p for p in case["pairs"] if p[0] <= 50 and (p[0], p[1]) in deciding]) >= 6
            for j, (d1, d2, accepted) in enumerate(case["pairs"]):
                assert m12[j] == (2 * j + 1 if accepted else -1), (d1, d2)
        elif name == "flags":
            assert m12 == ([-1, 0] if form == "frame" else [-1, 1]) and n == 1
            assert info["no_point1"] == 1 and info.get("no_point2", 0) == (0 if form == "frame" else 1)
        elif name.startswith("exact"):
            N = case["group"]
            alive = (case["n1"] == 7) & (case["good1"] == 1)
            assert alive.sum() == N == info["accepted"] == n and info["no_point1"] == 2 and not alive[:N].all()
            assert m12 == case["expected_m12"].tolist() and (case["expected_m12"][alive] >= 0).all()
        elif name == "cull":
            assert m12 == list(range(12)) + [-1, 13] and n == 13
            assert info["culled"] == 1 and info["blocked2"] == 1          # the culled match blocked query 13 during the walk


def _tri_by_rule(case):
    if "expected_m12" in case:
        return list(case["expected_m12"])
    if case["name"] == "tie":
        return [1, 2, 4]
    if case["name"].startswith("uright"):
        s = [True, True, False, False]                        # -0.0 >= 0, 0.0 >= 0, -1.4e-45 < 0, -1 < 0
        both = case["only_stereo"]
        return [(4 * i + j) if ((s[i] and s[j]) if both else (s[i] or s[j])) else -1 for i in range(4) for j in range(4)]
    if case["name"] == "zeroF":
        return [-1, -1]
    raise AssertionError(case["name"])


@pytest.mark.parametrize("case", Cs.tri_constructed_cases(), ids=lambda c: c["name"])
def test_search_for_triangulation_hand_worked(case):
    info = {}
    n, m12 = Cs.tri_expected(case, info)
    want = _tri_by_rule(case)
    assert m12.tolist() == [int(w) for w in want] and n == sum(1 for w in want if w >= 0)
    name = case["name"]
    if name.startswith("count"):
        assert info["shared_candidate"] == 1 and info["tie_replaces"] == 2      # vbMatched2 is never written
    if name == "tie":
        assert info["tie_replaces"] == 1 and info["epipolar_reject"] == 1 and info["epipole_skip"] == 1
    if name == "epipoleNone":
        assert info["epipole_skip"] == 2
    if name in ("epipole1", "epipole2"):
        assert "epipole_skip" not in info
    if name == "epipolar_edge":
        assert info["tie_replaces"] == len(Cs.EDGE_LEVELS) and info["epipolar_reject"] == len(Cs.EDGE_LEVELS)
    if name == "zeroF":
        assert info["den_zero"] == 6
    if name == "th_low":
        assert info["dist_skip"] == 2 and info["tie_replaces"] == 1 and info["unmatched"] == 1
    if name.startswith("edge_pose"):
        assert info["tie_replaces"] == 1 and info["epipolar_reject"] == 1


def test_epipolar_gate_is_float_dsqr_against_a_double_product():
    """CheckDistEpipolarLine by hand at level 0: y2 = 1.9595917463302612f squares to the float 3.8399999141693115, which
    is (float)3.84 and lies below the double 3.84."""
    y = f32(1.9595917463302612)
    assert float(f32(y * y)) == float(f32(3.84)) < 3.84
    F = Cs.F_EDGE
    assert B.check_dist_epipolar_line(1.0, 44.0, 10.0, y, 0, F, Cs.SIGMA2)
    assert not B.check_dist_epipolar_line(1.0, 44.0, 10.0, np.nextafter(y, f32(9)), 0, F, Cs.SIGMA2)
    assert not B.check_dist_epipolar_line(1.0, 44.0, 10.0, y, 0, np.zeros((3, 3), f32), Cs.SIGMA2)       # den == 0


# -- 3. the enumerations -----------------------------------------------------------------------------------------------

def test_ratio_test_enumeration():
    for r in (0.7, 0.75, 0.9):
        assert Cs.ratio_pairs(r) == []
    p6, p8 = Cs.ratio_pairs(0.6), Cs.ratio_pairs(0.8)
    # every deciding pair is a multiple of (3, 5) / (4, 5), rejected by the reference and accepted in double
    assert all(5 * a == 3 * b and not acc for a, b, acc in p6) and all(5 * a == 4 * b and not acc for a, b, acc in p8)
    assert len(p8) == 51                                        # every multiple up to (204, 255)
    s6 = {(a, b) for a, b, _ in p6}
    assert (3, 5) in s6 and (24, 40) in s6 and (15, 25) not in s6
    assert {(4, 5), (8, 10)} <= {(a, b) for a, b, _ in p8}
    # (15, 25): 0.6f * 25 rounds up to the next float above 15, so both precisions accept
    assert f32(15) < f32(f32(0.6) * f32(25)) and 15.0 < float(f32(0.6)) * 25.0
    # of the 51 multiples of (3, 5), those whose float product rounds up are accepted either way and do not separate
    assert len(p6) == sum(1 for k in range(1, 52) if not f32(3 * k) < f32(f32(0.6) * f32(5 * k))) == 33
    assert sum(1 for a, _, _ in p6 if a <= 50) >= 6 and sum(1 for a, _, _ in p8 if a <= 50) >= 6


def test_epipolar_gate_enumeration():
    found = {level: Cs.epipolar_edge(level) for level in range(8)}
    assert [level for level in range(8) if found[level] is not None] == list(Cs.EDGE_LEVELS)
    assert Cs.epipolar_edge(3, tuple(range(1, 200))) is None
    b, y = found[0]
    assert b == 1 and float(y) == 1.9595917463302612
    for level in Cs.EDGE_LEVELS:
        b, y = found[level]
        num = f32(b * y)
        dsqr = f32(f32(num * num) / f32(b * b))
        s2 = Cs.SIGMA2[level]
        assert f64(dsqr) < 3.84 * f64(s2) and not dsqr < f32(f32(3.84) * s2)


# -- 2. seqref against the oracle --------------------------------------------------------------------------------------

def _oracle_voc(O, tmp_path, voc, name="voc.txt"):
    return O.OracleVocabulary(write_vocabulary(tmp_path / name, voc))


def test_transform_equals_the_oracle_on_every_type(oracle, tmp_path):
    feats = Cs.typed_features()
    reached = set()
    for scoring in range(6):
        for weighting in range(4):
            voc = Cs.typed_vocabulary(scoring, weighting)
            path = write_vocabulary(tmp_path / "t.txt", voc)
            ov = oracle.OracleVocabulary(path)
            sv = B.load_text(path)
            for levelsup in (0, 1, 2, 5):
                r = B.transform(sv, feats, levelsup)
                same(r, ov.transform(feats, levelsup), (scoring, weighting, levelsup))
            reached.add((len(r["bow_ids"]) > 3, bool((r["node_id"] == NO).any())))
            same(B.transform(Cs.seq_voc(voc), feats, 1), B.transform(sv, feats, 1))          # arrays == text file
    assert reached == {(True, True)}                          # stopped words occur, and so do real ones


@pytest.mark.parametrize("case", Cs.transform_cases(), ids=lambda c: c[0])
def test_transform_cases_equal_the_oracle(oracle, tmp_path, case):
    name, voc, feats, levelsups = case
    ov = _oracle_voc(oracle, tmp_path, voc)
    sv = Cs.seq_voc(voc)
    for levelsup in levelsups:
        r = B.transform(sv, feats, levelsup)
        same(r, ov.transform(feats, levelsup), (name, levelsup))
    if name == "all_stopped":
        assert r["bow_ids"].size == 0 and (r["node_id"] == NO).all()
    if name.startswith("heavy_word"):
        assert np.bincount(r["word_id"]).max() > 1500
        w = voc["weight"][voc["is_leaf"] == 1]
        assert w.max() / w.min() > 1e4
    if name == "k20_L2":
        kid = (r["word_id"] // 20)                            # the level-1 child each feature went through
        assert (kid >= 17).any() and (kid == 15).any() and not (kid == 16).any()     # the twin of child 15 never wins


def _oracle_frames(O, c, keep):
    return (O.make_frame(c["k1"], c["d1"], c.get("ur1"), Cs.BOUNDS, Cs.SF, keep),
            O.make_frame(c["k2"], c["d2"], c.get("ur2"), Cs.BOUNDS, Cs.SF, keep))


BOW_BRANCHES = {"common_node", "skip_side1", "skip_side2", "walk_end_side1", "walk_end_side2", "no_point1", "blocked2",
                "new_best", "new_second", "neither", "accepted", "ratio_reject", "over_th", "no_candidate", "culled"}


def test_search_by_bow_equals_the_oracle(oracle):
    for form in ("frame", "kf"):
        for c in Cs.bow_constructed_cases() + Cs.bow_random_cases():
            n, m12 = Cs.bow_expected(c, form)
            keep = []
            o1, o2 = _oracle_frames(oracle, c, keep)
            v1, b2, max_dist = Cs.bow_entry_args(c, form)
            on, om12 = oracle.search_by_bow(o1, c["n1"], v1, o2, c["n2"], b2, max_dist, c["nnratio"], c["check_ori"])
            assert on == n and om12.dtype == m12.dtype and np.array_equal(om12, m12), (form, c["name"])
    # the random scenes alone take every way out, in either form
    for form in ("frame", "kf"):
        seen = {}
        for c in Cs.bow_random_cases():
            Cs.bow_expected(c, form, seen)
        want = BOW_BRANCHES | ({"no_point2"} if form == "kf" else set())
        assert all(seen.get(k, 0) > 0 for k in want), sorted(want - {k for k, v in seen.items() if v > 0})


TRI_BRANCHES = {"common_node", "skip_side1", "skip_side2", "walk_end_side1", "walk_end_side2", "has_point1", "has_point2",
                "mono1_only_stereo", "mono2_only_stereo", "dist_skip", "epipole_skip", "den_zero", "epipolar_reject",
                "new_best", "tie_replaces", "matched", "unmatched", "shared_candidate", "culled"}


def test_search_for_triangulation_equals_the_oracle(oracle):
    seen = {}
    for c in Cs.tri_constructed_cases() + Cs.tri_random_cases():
        info = seen if c["name"].startswith("tri_") else {}
        n, m12 = Cs.tri_expected(c, info)
        keep = []
        o1, o2 = _oracle_frames(oracle, c, keep)
        v1 = None if c["free1"] is None else c["free1"]
        v2 = None if c["free2"] is None else c["free2"]
        on, om12 = oracle.search_for_triangulation(o1, c["n1"], v1, o2, c["n2"], v2, c["F12"], c["ex"], c["ey"], Cs.SIGMA2,
                                                   c["only_stereo"], c["check_ori"])
        assert on == n and om12.dtype == m12.dtype and np.array_equal(om12, m12), c["name"]
    assert all(seen.get(k, 0) > 0 for k in TRI_BRANCHES), sorted(TRI_BRANCHES - {k for k, v in seen.items() if v > 0})


def test_distinctive_descriptor_equals_the_oracle(oracle):
    lists = Cs.distinctive_lists()
    got = [B.distinctive_descriptor(d) for d in lists]
    assert got == [oracle.distinctive_descriptor(d) for d in lists]
    assert got[-1] == 1                                        # rows 1 and 2 share the least median: the first wins
    assert sorted(len(d) for d in lists) == [1, 2, 3, 4, 4, 63, 64, 65, 129, 2048] and any(len(np.unique(d, axis=0)) < len(d) for d in lists)
