"""Sequential restatement of the two culling steps of local mapping, loop for loop from the cited lines:

  LocalMapping::MapPointCulling   src/LocalMapping.cc:170-205
  LocalMapping::KeyFrameCulling   src/LocalMapping.cc:632-696
  MapPoint::EraseObservation      src/MapPoint.cc:111-137
  MapPoint::SetBadFlag            src/MapPoint.cc:151-168
  KeyFrame::SetBadFlag            src/KeyFrame.cc:453-545 (without mTcp, Map::EraseKeyFrame, KeyFrameDatabase::erase)
  KeyFrame::EraseConnection       src/KeyFrame.cc:553-567

on Python lists and dicts.  A Map holds, per point, mObservations as a list of (row, key point) in table order (the order
map<KeyFrame*, size_t> has here, as in seqref.localmap), nObs, mpRefKF as a row, the flags, and per bank row mvpMapPoints,
mbBad and mbToBeErased; the graph is seqref.covisibility.Graph.  Entries are erased from the lists: there are no alive marks
and no compaction, the table is written out from the lists at the end.  Address order is row order.

Every function counts in `info` each way out it takes.  It imports neither the oracle nor the package."""
import numpy as np

from . import covisibility as CV

POINT_PRESENT, POINT_OBSERVED = 1, 2
KEPT, ALREADY_BAD, BAD_RATIO, BAD_OBS, DROPPED_OLD = range(5)
NOT_CULLED, CULLED, SKIPPED_ID0, SKIPPED_ENTRY, NOT_ERASE = range(5)
REPORT_FIELDS = ("status", "n_mps", "n_redundant", "n_erased", "n_bad", "n_resorted", "n_children", "fallback")


def _count(info, key):
    if info is not None:
        info[key] = info.get(key, 0) + 1


class Map:
    """slot_point [rows][cap], n [rows], u_right [rows][cap] or None, flags [pcap], kf_bad / to_be_erased [rows] and the
    observation table obs_start / obs_kf / obs_idx / ref_obs.  A point that is bad has no observations."""

    def __init__(self, slot_point, n, u_right, flags, obs_start, obs_kf, obs_idx, ref_obs, kf_bad=None, to_be_erased=None):
        self.slot_point = np.array(slot_point, np.int32)
        self.n = [int(x) for x in n]
        self.u_right = u_right
        self.flags = [int(f) for f in flags]
        rows = len(self.n)
        self.kf_bad = [0] * rows if kf_bad is None else [int(b) for b in kf_bad]
        self.to_be_erased = [0] * rows if to_be_erased is None else [int(b) for b in to_be_erased]
        self.np = len(obs_start) - 1
        self.obs, self.nobs, self.ref = [], [], []
        for p in range(self.np):
            lst = [(int(obs_kf[o]), int(obs_idx[o])) for o in range(int(obs_start[p]), int(obs_start[p + 1]))]
            if not self.flags[p] & POINT_PRESENT:
                lst = []                                              # SetBadFlag cleared mObservations (src/MapPoint.cc:159)
            assert len({k for k, _ in lst}) == len(lst), "mObservations holds a key frame once"
            self.obs.append(lst)
            self.nobs.append(sum(self.weight(k, i) for k, i in lst))  # AddObservation, src/MapPoint.cc:105-108
            j = int(ref_obs[p])
            self.ref.append(lst[j][0] if 0 <= j < len(lst) else None)

    def weight(self, kf, idx):
        return 2 if self.u_right is not None and self.u_right[kf][idx] >= 0 else 1

    def table(self):
        """obs_start, obs_kf, obs_idx, ref_obs of the lists as they are now."""
        start = np.concatenate([[0], np.cumsum([len(x) for x in self.obs])]).astype(np.int32)
        kf = np.array([k for x in self.obs for k, _ in x], np.int32)
        idx = np.array([i for x in self.obs for _, i in x], np.int32)
        ref = np.full(self.np, -1, np.int32)
        for p, lst in enumerate(self.obs):
            rows = [k for k, _ in lst]
            if self.ref[p] in rows:
                ref[p] = rows.index(self.ref[p])
        return start, kf, idx, ref


def map_point_set_bad(M, p, info=None):
    """MapPoint::SetBadFlag, src/MapPoint.cc:151-168."""
    M.flags[p] &= ~POINT_PRESENT                                      # mbBad = true; nObs is not reset
    obs = M.obs[p]
    M.obs[p] = []
    for kf, idx in obs:
        if M.slot_point[kf][idx] != p:
            _count(info, "erase_match_other_point")                   # EraseMapPointMatch(idx) is by index
        M.slot_point[kf][idx] = -1


def erase_observation(M, p, r, info=None):
    """pMP = p ->EraseObservation(r), src/MapPoint.cc:111-137.  Returns (an entry was found, the point turned bad)."""
    bad = False
    rows = [k for k, _ in M.obs[p]]
    if r not in rows:
        _count(info, "erase_not_observed")
        return False, False
    j = rows.index(r)
    M.nobs[p] -= M.weight(r, M.obs[p][j][1])                          # :118-122
    del M.obs[p][j]
    if M.ref[p] == r:                                                 # :126-127
        _count(info, "ref_moved")
        M.ref[p] = M.obs[p][0][0] if M.obs[p] else None
    M.flags[p] = (M.flags[p] & ~POINT_OBSERVED) | (POINT_OBSERVED if M.nobs[p] > 0 else 0)
    if M.nobs[p] <= 2:                                                # :130-131
        bad = True
    if bad:
        _count(info, "erase_turned_bad")
        map_point_set_bad(M, p, info)
    return True, bad


def map_point_culling(M, recent, found, visible, first_kf_id, cur_kf_id, th_obs, info=None):
    """src/LocalMapping.cc:170-205.  Returns (the list left, status per entry of the list passed in)."""
    kept, status = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in recent:
            p = int(p)
            age = int(cur_kf_id) - int(first_kf_id[p])
            if not M.flags[p] & POINT_PRESENT:                        # :186
                st = ALREADY_BAD
            elif np.float32(found[p]) / np.float32(visible[p]) < np.float32(0.25):         # :190, GetFoundRatio
                st = BAD_RATIO
                map_point_set_bad(M, p, info)
            elif age >= 2 and M.nobs[p] <= th_obs:                    # :195
                st = BAD_OBS
                map_point_set_bad(M, p, info)
            elif age >= 3:                                            # :200
                st = DROPPED_OLD
            else:
                st = KEPT
                kept.append(p)
            _count(info, "mp_status_%d" % st)
            status.append(st)
    return kept, np.array(status, np.uint8)


def erase_connection(G, c, r, info=None, touched=None):
    """pKF = c ->EraseConnection(r), src/KeyFrame.cc:553-567.  Returns True when the row was re-sorted."""
    if r in G.conn[c]:
        del G.conn[c][r]
        CV.update_best_covisibles(G, c)
        if touched is not None:
            touched.add(c)
        return True
    _count(info, "asymmetric_connection")
    return False


def key_frame_set_bad(M, G, r, not_erase, id0_row, rep, info=None, touched=None):
    """KeyFrame::SetBadFlag of bank row r, src/KeyFrame.cc:453-545."""
    if r == id0_row:                                                  # :457
        return
    if not_erase is not None and not_erase[r]:                        # :459-463
        _count(info, "not_erase")
        M.to_be_erased[r] = 1
        rep["status"] = NOT_ERASE
        return
    assert r not in G.conn[r], "UpdateConnections never stores a self-connection"
    for c in sorted(G.conn[r]):                                       # :466-467
        rep["n_resorted"] += erase_connection(G, c, r, info, touched)
    for i in range(M.n[r]):                                           # :469-471
        p = int(M.slot_point[r][i])
        if p >= 0:
            hit, bad = erase_observation(M, p, r, info)
            rep["n_erased"] += hit
            rep["n_bad"] += bad
    G.conn[r] = {}                                                    # :476-477
    G.set_lists(r, [], [])
    if touched is not None:
        touched.add(r)
    parent = G.parent[r]
    candidates = set()                                                # :480-481
    if parent >= 0:
        candidates.add(parent)
    else:
        _count(info, "no_parent")
        rep["fallback"] = 1
    children = [c for c in range(G.rows) if G.parent[c] == r and not M.kf_bad[c]]      # mspChildrens, ascending
    rep["n_children"] = len(children)
    while children:                                                   # :485-528
        go_on = False
        mx, pc, pp = -1, None, None
        for c in children:
            for k in G.ord_kf[c]:                                     # vpConnected
                if k in candidates:                                   # :503-505
                    w = G.conn[c].get(k, 0)                           # GetWeight
                    if w > mx:
                        pc, pp, mx, go_on = c, k, w, True
        if go_on:
            _count(info, "child_adopted")
            G.parent[pc] = pp                                         # ChangeParent
            candidates.add(pc)
            children.remove(pc)
        else:
            break
    for c in children:                                                # :531-535
        _count(info, "child_fell_back")
        G.parent[c] = parent
        rep["fallback"] = 1
    M.kf_bad[r] = 1                                                   # :539


def key_frame_culling(M, G, cand, octave, depth, not_erase, id0_row, mono, th_depth, info=None, touched=None):
    """src/LocalMapping.cc:632-696 over `cand`, the copy vpLocalKeyFrames; -1 entries are skipped.  octave [rows][cap] =
    mvKeysUn[i].octave, depth [rows][cap] = mvDepth.  Returns report [U][8] in the order of REPORT_FIELDS."""
    out = np.zeros((len(cand), 8), np.int32)
    th = np.float32(th_depth)
    for u, r in enumerate(int(x) for x in cand):
        rep = dict.fromkeys(REPORT_FIELDS, 0)
        if r < 0:
            rep["status"] = SKIPPED_ENTRY
        elif r == id0_row:                                            # :643
            rep["status"] = SKIPPED_ID0
        else:
            n_red, n_mps = 0, 0
            for i in range(M.n[r]):                                   # :651
                p = int(M.slot_point[r][i])
                if p < 0:
                    continue
                if not M.flags[p] & POINT_PRESENT:
                    _count(info, "decide_bad_point")
                    continue
                if not mono:                                          # :658-662
                    d = np.float32(depth[r][i])
                    if d > th or d < 0:
                        _count(info, "decide_depth_gate")
                        continue
                n_mps += 1
                if M.nobs[p] > 3:                                     # :665
                    level = int(octave[r][i])
                    n_obs = 0
                    for kf, idx in M.obs[p]:                          # :670-683
                        if kf == r:
                            continue
                        if int(octave[kf][idx]) <= level + 1:
                            n_obs += 1
                            if n_obs >= 3:
                                break
                        else:
                            _count(info, "decide_coarser_scale")
                    if n_obs >= 3:
                        n_red += 1
                else:
                    _count(info, "decide_few_observations")
            rep["n_mps"], rep["n_redundant"] = n_mps, n_red
            if n_red > 0.9 * n_mps:                                   # :693
                rep["status"] = CULLED
                if M.kf_bad[r]:
                    _count(info, "bad_candidate_culled_again")
                key_frame_set_bad(M, G, r, not_erase, id0_row, rep, info, touched)
        _count(info, "kf_status_%d" % rep["status"])
        out[u] = [rep[k] for k in REPORT_FIELDS]
    return out
