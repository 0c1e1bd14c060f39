"""Everything guided by the DBoW2 vocabulary, restated loop for loop from the cited lines:

  TemplatedVocabulary::loadFromTextFile   Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424
  TemplatedVocabulary::transform (x2)     Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194, :1218-1259
  BowVector::addWeight / addIfNotExist / normalize   Thirdparty/DBoW2/DBoW2/BowVector.cpp:34-84
  FORB::distance / fromString             Thirdparty/DBoW2/DBoW2/FORB.cpp:81-101, :120-135 (distance = the popcount of
                                          a xor b, the same number as ORBmatcher::DescriptorDistance)
  ORBmatcher::CheckDistEpipolarLine       src/ORBmatcher.cc:140-157
  ORBmatcher::SearchByBoW(KeyFrame*, Frame&)      src/ORBmatcher.cc:159-288
  ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*)   src/ORBmatcher.cc:522-655
  ORBmatcher::SearchForTriangulation      src/ORBmatcher.cc:657-823

A DBoW2::FeatureVector arrives the way the package and the oracle take it: one node id per key point, NO_NODE where the
key point is in no list.  `feature_vector` turns that back into the std::map<NodeId, vector<unsigned>> the reference walks
(keys ascending, indices in push_back = ascending order, FeatureVector.cpp addFeature).

Every search takes an optional `info` dict and counts in it how often each way out of its loops was taken.

numpy and the standard library only; like the rest of seqref it imports neither the oracle nor the package."""
import bisect

import numpy as np

from .mappoint import distinctive_descriptor  # noqa: F401  (MapPoint::ComputeDistinctiveDescriptors, src/MapPoint.cc:272-301)
from .matcher import HISTO_LENGTH, TH_LOW, compute_three_maxima, descriptor_distance, rotation_bin

f32, f64 = np.float32, np.float64
NO_NODE = 0xFFFFFFFF

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3                                        # BowVector.h:36-42
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)     # BowVector.h:45-53
# ScoringObject.h:74-89, __SCORING_CLASS(NAME, MUSTNORMALIZE, NORM)
MUST_NORMALIZE = {L1_NORM: (True, "L1"), L2_NORM: (True, "L2"), CHI_SQUARE: (True, "L1"), KL: (True, "L1"),
                  BHATTACHARYYA: (True, "L1"), DOT_PRODUCT: (False, "L1")}


def _count(info, key, by=1):
    if info is not None:
        info[key] = info.get(key, 0) + by


# -- vocabulary --------------------------------------------------------------------------------------------------------

class Vocabulary:
    """m_k, m_L, m_scoring, m_weighting, m_nodes (index = NodeId, 0 = root) and m_words (index = WordId -> NodeId)."""

    def __init__(self, k, L, scoring, weighting):
        self.k, self.L, self.scoring, self.weighting = k, L, scoring, weighting
        self.parent, self.children, self.desc, self.weight, self.word_id = [0], [[]], [None], [0.0], [None]
        self.words = []

    def add_node(self, pid, is_leaf, desc, weight):
        """:1385-1419 for one line of the file."""
        nid = len(self.parent)
        if not 0 <= pid < nid:
            raise ValueError("node %d names parent %d: the reference would index m_nodes out of range" % (nid, pid))
        self.parent.append(pid)
        self.children.append([])
        self.children[pid].append(nid)                      # :1392 push_back: order of appearance in the file
        self.desc.append(np.asarray(desc, np.uint8).reshape(32))
        self.weight.append(float(weight))
        if is_leaf > 0:                                     # :1408-1415: word ids in order of leaf appearance
            self.word_id.append(len(self.words))
            self.words.append(nid)
        else:
            self.word_id.append(None)

    def empty(self):
        return len(self.words) == 0                         # TemplatedVocabulary::empty: m_words.empty()


def from_arrays(k, L, scoring, weighting, parent, is_leaf, desc, weight):
    """The same tree from arrays in file order: entry i is node i + 1."""
    voc = Vocabulary(int(k), int(L), int(scoring), int(weighting))
    for i in range(len(parent)):
        voc.add_node(int(parent[i]), int(is_leaf[i]), desc[i], float(weight[i]))
    return voc


def load_text(path):
    """loadFromTextFile.  Returns None where the reference returns false (:1359-1363), a Vocabulary otherwise."""
    with open(path, "r") as f:
        lines = f.read().split("\n")
    head = lines[0].split()
    try:
        k, L, n1, n2 = (int(t) for t in head[:4])
    except ValueError:
        return None
    if len(head) < 4:
        return None
    if k < 0 or k > 20 or L < 1 or L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:      # :1359
        return None
    voc = Vocabulary(k, L, n1, n2)
    for line in lines[1:]:
        tok = line.split()
        if not tok:
            # CHOICE ("DBoW2 text loader"): blank lines are skipped.  The reference's
            # while(!f.eof()) loop turns the empty string after the last newline into one more child of the root
            # with an uninitialised descriptor.
            continue
        if len(tok) < 35:
            raise ValueError("truncated node line: the reference reads uninitialised values here")
        pid, is_leaf = int(tok[0]), int(tok[1])
        desc = [int(t) & 0xFF for t in tok[2:34]]           # FORB::fromString: (unsigned char)n
        voc.add_node(pid, is_leaf, desc, float(tok[34]))    # operator>>(double&): correctly rounded, as float() is
    return voc


def transform_feature(voc, feature, levelsup):
    """:1218-1259.  Returns (word_id, weight, nid)."""
    nid_level = voc.L - levelsup
    nid = None
    if nid_level <= 0:                                      # :1227
        nid = 0
    final_id = 0
    current_level = 0
    while True:                                             # do { } while(!isLeaf())
        current_level += 1
        nodes = voc.children[final_id]
        if not nodes:
            raise ValueError("inner node %d has no children: the reference reads nodes[0] of an empty vector" % final_id)
        dists = descriptor_distance(feature, np.stack([voc.desc[c] for c in nodes])).tolist()      # F::distance per child
        final_id, best_d = nodes[0], dists[0]
        for cid, d in zip(nodes[1:], dists[1:]):
            if d < best_d:                                  # :1244 strict: the first minimum stays
                best_d, final_id = d, cid
        if current_level == nid_level:                      # :1251
            nid = final_id
        if voc.word_id[final_id] is not None:               # isLeaf(): children.empty(); a leaf line has a word id
            break
    if nid is None:
        # CHOICE ("transform: *nid left unset"): a leaf reached above level L - levelsup reports
        # its own id.  The reference leaves *nid uninitialised.
        nid = final_id
    return voc.word_id[final_id], voc.weight[final_id], nid


def transform(voc, features, levelsup=4):
    """transform(features, BowVector&, FeatureVector&, levelsup), :1127-1194.  Returns the five arrays of the package:
    word_id [n] uint32, word_weight [n] float64, node_id [n] uint32 (NO_NODE: the feature is in no FeatureVector list),
    bow_ids [m] uint32 ascending, bow_vals [m] float64."""
    feats = np.asarray(features, np.uint8).reshape(-1, 32)
    n = len(feats)
    word = np.zeros(n, np.uint32)
    wgt = np.zeros(n, np.float64)
    node = np.full(n, NO_NODE, np.uint32)
    if voc.empty():                                         # :1134-1137
        return {"word_id": word, "word_weight": wgt, "node_id": node, "bow_ids": np.zeros(0, np.uint32),
                "bow_vals": np.zeros(0, np.float64)}
    must, norm = MUST_NORMALIZE[voc.scoring]
    v = {}                                                  # the std::map; iterated in ascending key order below
    accumulate = voc.weighting in (TF, TF_IDF)              # :1145
    for i in range(n):
        wid, w, nid = transform_feature(voc, feats[i], levelsup)
        word[i], wgt[i] = wid, w
        if w > 0:                                           # :1157 / :1185 not stopped
            if accumulate:
                v[wid] = f64(v[wid] + f64(w)) if wid in v else f64(w)       # addWeight
            elif wid not in v:
                v[wid] = f64(w)                                             # addIfNotExist: the first value stays
            node[i] = nid                                                   # fv.addFeature(nid, i_feature)
    ids = sorted(v)
    if accumulate and ids and not must:                     # :1164-1170
        nd = f64(len(ids))
        for wid in ids:
            v[wid] = f64(v[wid] / nd)
    if must:                                                # BowVector::normalize
        s = f64(0.0)
        if norm == "L1":
            for wid in ids:
                s = f64(s + abs(v[wid]))
        else:
            for wid in ids:
                s = f64(s + f64(v[wid] * v[wid]))
            s = np.sqrt(s)
        if s > 0.0:
            for wid in ids:
                v[wid] = f64(v[wid] / s)
    return {"word_id": word, "word_weight": wgt, "node_id": node, "bow_ids": np.array(ids, np.uint32),
            "bow_vals": np.array([v[wid] for wid in ids], np.float64)}


def feature_vector(node_id):
    """(sorted node ids, {node: [feature indices ascending]}) from one node id per key point."""
    fv = {}
    for i, nd in enumerate(np.asarray(node_id).tolist()):
        if nd != NO_NODE:
            fv.setdefault(int(nd), []).append(i)
    return sorted(fv), fv


def _walk(node1, node2, info):
    """The two-iterator walk all three searches share (:180-264, :550-632, :691-789): yields the index lists of every
    node both FeatureVectors hold, skipping with lower_bound."""
    k1, fv1 = feature_vector(node1)
    k2, fv2 = feature_vector(node2)
    a = b = 0
    while a < len(k1) and b < len(k2):
        if k1[a] == k2[b]:
            _count(info, "common_node")
            yield fv1[k1[a]], fv2[k2[b]]
            a += 1
            b += 1
        elif k1[a] < k2[b]:
            _count(info, "skip_side1")
            a = bisect.bisect_left(k1, k2[b])               # lower_bound(f2it->first)
        else:
            _count(info, "skip_side2")
            b = bisect.bisect_left(k2, k1[a])
    _count(info, "walk_end_side1" if a >= len(k1) else "walk_end_side2")


def ratio_accepts(best1, best2, nnratio):
    """static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2), mfNNratio a float member."""
    return bool(f32(best1) < f32(f32(nnratio) * f32(best2)))


def _cull(hist, info):
    """The indices the rotation histogram removes (:267-285, :634-652, :791-808)."""
    ind = compute_three_maxima([len(h) for h in hist])
    out = []
    for b in range(HISTO_LENGTH):
        if b in ind:
            continue
        out += hist[b]
    _count(info, "culled", len(out))
    return out


# -- SearchByBoW -------------------------------------------------------------------------------------------------------

def search_by_bow_kf_frame(keys_kf, desc_kf, node_kf, good_kf, keys_f, desc_f, node_f, nnratio, check_ori=True, info=None):
    """SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches), :159-288.  good_kf[i]: vpMapPointsKF[i] is non-null and not bad
    (None: all).  Returns (nmatches, matches[F.N]) where matches[iF] is the key-frame key point whose map point
    vpMapPointMatches[iF] holds, -1 for NULL."""
    desc_kf = np.asarray(desc_kf, np.uint8).reshape(-1, 32)
    desc_f = np.asarray(desc_f, np.uint8).reshape(-1, 32)
    NF = len(desc_f)
    matches = np.full(NF, -1, np.int32)
    occupied = np.zeros(NF, bool)                           # vpMapPointMatches[realIdxF] != NULL during the walk
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for idx_kf, idx_f in _walk(node_kf, node_f, info):
        for realIdxKF in idx_kf:
            if good_kf is not None and not good_kf[realIdxKF]:           # :193-197
                _count(info, "no_point1")
                continue
            bestDist1, bestIdxF, bestDist2 = 256, -1, 256
            for realIdxF in idx_f:
                if occupied[realIdxF]:                                   # :209
                    _count(info, "blocked2")
                    continue
                dist = int(descriptor_distance(desc_kf[realIdxKF], desc_f[realIdxF]))
                if dist < bestDist1:
                    bestDist2, bestDist1, bestIdxF = bestDist1, dist, realIdxF
                    _count(info, "new_best")
                elif dist < bestDist2:
                    bestDist2 = dist
                    _count(info, "new_second")
                else:
                    _count(info, "neither")
            if bestDist1 <= TH_LOW:                                      # :228, <=
                if ratio_accepts(bestDist1, bestDist2, nnratio):         # :230
                    matches[bestIdxF] = realIdxKF
                    occupied[bestIdxF] = True
                    if check_ori:
                        hist[rotation_bin(keys_kf["angle"][realIdxKF], keys_f["angle"][bestIdxF])].append(bestIdxF)
                    nmatches += 1
                    _count(info, "accepted")
                else:
                    _count(info, "ratio_reject")
            else:
                _count(info, "over_th" if bestIdxF >= 0 else "no_candidate")
    if check_ori:
        for iF in _cull(hist, info):                                     # :281: the slot is cleared after the walk only
            matches[iF] = -1
            nmatches -= 1
    return nmatches, matches


def search_by_bow_kf_kf(keys1, desc1, node1, good1, keys2, desc2, node2, good2, nnratio, check_ori=True, info=None):
    """SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12), :522-655.  good[i]: the slot holds a map point that is not bad
    (None: all).  Returns (nmatches, matches12[N1]): the key point of pKF2 whose map point vpMatches12[i] holds, or -1."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    matches12 = np.full(len(desc1), -1, np.int32)
    vbMatched2 = np.zeros(len(desc2), bool)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for l1, l2 in _walk(node1, node2, info):
        for idx1 in l1:
            if good1 is not None and not good1[idx1]:                    # :559-562
                _count(info, "no_point1")
                continue
            bestDist1, bestIdx2, bestDist2 = 256, -1, 256
            for idx2 in l2:
                if vbMatched2[idx2]:                                     # :576
                    _count(info, "blocked2")
                    continue
                if good2 is not None and not good2[idx2]:                # :576 !pMP2, :579 isBad
                    _count(info, "no_point2")
                    continue
                dist = int(descriptor_distance(desc1[idx1], desc2[idx2]))
                if dist < bestDist1:
                    bestDist2, bestDist1, bestIdx2 = bestDist1, dist, idx2
                    _count(info, "new_best")
                elif dist < bestDist2:
                    bestDist2 = dist
                    _count(info, "new_second")
                else:
                    _count(info, "neither")
            if bestDist1 < TH_LOW:                                       # :598, strict
                if ratio_accepts(bestDist1, bestDist2, nnratio):         # :600
                    matches12[idx1] = bestIdx2
                    vbMatched2[bestIdx2] = True
                    if check_ori:
                        hist[rotation_bin(keys1["angle"][idx1], keys2["angle"][bestIdx2])].append(idx1)
                    nmatches += 1
                    _count(info, "accepted")
                else:
                    _count(info, "ratio_reject")
            else:
                _count(info, "over_th" if bestIdx2 >= 0 else "no_candidate")
    if check_ori:
        for i1 in _cull(hist, info):
            matches12[i1] = -1
            nmatches -= 1
    return nmatches, matches12


# -- SearchForTriangulation --------------------------------------------------------------------------------------------

def check_dist_epipolar_line(x1, y1, x2, y2, octave2, F12, level_sigma2, info=None):
    """CheckDistEpipolarLine, :140-157: float products and sums left to right, the last comparison in double."""
    F = np.asarray(F12, f32).reshape(3, 3)
    x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    with np.errstate(all="ignore"):
        a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0])
        b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
        c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
        num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
        den = f32(f32(a * a) + f32(b * b))
        if den == 0:                                                     # :151
            _count(info, "den_zero")
            return False
        dsqr = f32(f32(num * num) / den)
        return bool(f64(dsqr) < f64(3.84) * f64(f32(level_sigma2[octave2])))     # :156: 3.84 is a double literal


def search_for_triangulation(keys1, desc1, node1, free1, ur1, keys2, desc2, node2, free2, ur2, F12, ex, ey, level_sigma2,
                             scale_factors, only_stereo=False, check_ori=True, info=None):
    """SearchForTriangulation after the epipole (:672-823; ex, ey are arguments as in the package).  free[i]: the slot holds
    no map point (None: all free); ur: mvuRight (None: all -1).  level_sigma2 / scale_factors are pKF2's tables.
    Returns (nmatches, vMatches12[N1])."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    N1, N2 = len(desc1), len(desc2)
    ur1 = np.full(N1, -1, f32) if ur1 is None else np.asarray(ur1, f32)
    ur2 = np.full(N2, -1, f32) if ur2 is None else np.asarray(ur2, f32)
    sf = np.asarray(scale_factors, f32)
    ex, ey = f32(ex), f32(ey)
    vMatches12 = np.full(N1, -1, np.int32)
    vbMatched2 = np.zeros(N2, bool)                                      # :677, never written
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for l1, l2 in _walk(node1, node2, info):
        for idx1 in l1:
            if free1 is not None and not free1[idx1]:                    # :702
                _count(info, "has_point1")
                continue
            bStereo1 = bool(ur1[idx1] >= 0)                              # :705
            if only_stereo and not bStereo1:                             # :707-709
                _count(info, "mono1_only_stereo")
                continue
            bestDist, bestIdx2 = TH_LOW, -1                              # :715-716
            for idx2 in l2:
                if vbMatched2[idx2] or (free2 is not None and not free2[idx2]):      # :725
                    _count(info, "has_point2")
                    continue
                bStereo2 = bool(ur2[idx2] >= 0)
                if only_stereo and not bStereo2:                         # :730-732
                    _count(info, "mono2_only_stereo")
                    continue
                dist = int(descriptor_distance(desc1[idx1], desc2[idx2]))
                if dist > TH_LOW or dist > bestDist:                     # :738
                    _count(info, "dist_skip")
                    continue
                if not bStereo1 and not bStereo2:                        # :743-749
                    with np.errstate(all="ignore"):
                        distex = f32(ex - f32(keys2["x"][idx2]))
                        distey = f32(ey - f32(keys2["y"][idx2]))
                        if f32(f32(distex * distex) + f32(distey * distey)) < f32(f32(100) * sf[keys2["octave"][idx2]]):
                            _count(info, "epipole_skip")
                            continue
                if check_dist_epipolar_line(keys1["x"][idx1], keys1["y"][idx1], keys2["x"][idx2], keys2["y"][idx2],
                                            int(keys2["octave"][idx2]), F12, level_sigma2, info):
                    _count(info, "tie_replaces" if (bestIdx2 >= 0 and dist == bestDist) else "new_best")
                    bestIdx2, bestDist = idx2, dist
                else:
                    _count(info, "epipolar_reject")
            if bestIdx2 >= 0:                                            # :758
                if (vMatches12 == bestIdx2).any():
                    _count(info, "shared_candidate")
                vMatches12[idx1] = bestIdx2
                nmatches += 1
                _count(info, "matched")
                if check_ori:
                    hist[rotation_bin(keys1["angle"][idx1], keys2["angle"][bestIdx2])].append(idx1)
            else:
                _count(info, "unmatched")
    if check_ori:
        for i1 in _cull(hist, info):
            vMatches12[i1] = -1
            nmatches -= 1
    return nmatches, vMatches12
