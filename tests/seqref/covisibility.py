"""Sequential restatement of the covisibility graph of a key frame, loop for loop from the cited lines:

  KeyFrame::AddConnection                  src/KeyFrame.cc:123-136
  KeyFrame::UpdateBestCovisibles           src/KeyFrame.cc:138-157
  KeyFrame::GetBestCovisibilityKeyFrames   src/KeyFrame.cc:174-182
  KeyFrame::UpdateConnections              src/KeyFrame.cc:289-379
  LocalMapping::SearchInNeighbors          src/LocalMapping.cc:457-479 (the target list)
  KeyFrame::SetBadFlag / AddChild          src/KeyFrame.cc:381-385, :453-545 (who is a child of whom)

over tables instead of the map graph: slot_point [rows][cap] / n [rows], the observation table obs_start / obs_kf and the
point flags of seqref.localmap.  A Graph holds, per bank row, mConnectedKeyFrameWeights as a dict {row: weight},
mvpOrderedConnectedKeyFrames / mvOrderedWeights as lists, mbFirstConnection and mpParent.

Where the reference iterates a map<KeyFrame*, int> or sorts pair<int, KeyFrame*> it goes by heap address; here address
order is row order, as in seqref.localmap: maps iterate in ascending row order, and the ascending sort followed by the
push_front reversal gives descending weight, then descending row among equal weights.

Every function counts in `info` each way out it takes.  Like the rest of seqref it imports neither the oracle nor the
package."""
import numpy as np

POINT_PRESENT = 1
OK, EMPTY = 0, 1
TH = 15                    # src/KeyFrame.cc:330
N_COVIS = 10               # the head orbhip_local_map_tables.covis holds
REPORT_FIELDS = ("status", "n_voted", "n_ordered", "max_row", "max_votes", "parent_set", "n_resorted", "fallback")


def _count(info, key):
    if info is not None:
        info[key] = info.get(key, 0) + 1


class Graph:
    def __init__(self, rows):
        self.rows = rows
        self.conn = [dict() for _ in range(rows)]          # mConnectedKeyFrameWeights
        self.ord_kf = [[] for _ in range(rows)]            # mvpOrderedConnectedKeyFrames
        self.ord_w = [[] for _ in range(rows)]             # mvOrderedWeights
        self.first_conn = [True] * rows                    # mbFirstConnection
        self.parent = [-1] * rows                          # mpParent
        self.mirror = None                                 # dense ord_kf / ord_w / covis that follow every rewrite of a list

    def set_lists(self, r, lk, lw):
        """The two vector assignments (:155-156, :368-369).  In the dense layout a rewrite stores the new entries and the
        head and leaves the entries behind them as they were; `mirror` keeps arrays that are written this way."""
        self.ord_kf[r], self.ord_w[r] = lk, lw
        if self.mirror is not None:
            self.mirror["ord_kf"][r, :len(lk)] = lk
            self.mirror["ord_w"][r, :len(lw)] = lw
            self.mirror["covis"][r] = (lk + [-1] * N_COVIS)[:N_COVIS]

    def dense(self, fill=None):
        """The arrays of orbhip_covis_state.  Entries past n_ord hold `fill` (a dict of arrays to start from) or -1 / 0; with
        a mirror, ord_kf / ord_w / covis are the mirror's."""
        rows = self.rows
        A = dict(conn_w=np.zeros((rows, rows), np.int32), ord_kf=np.full((rows, rows), -1, np.int32),
                 ord_w=np.zeros((rows, rows), np.int32), n_ord=np.zeros(rows, np.int32),
                 covis=np.full((rows, N_COVIS), -1, np.int32), first_conn=np.zeros(rows, np.uint8),
                 parent=np.full(rows, -1, np.int32))
        if fill is not None:
            for k in ("ord_kf", "ord_w", "covis"):
                A[k] = np.array(fill[k], np.int32).reshape(A[k].shape).copy()
        for r in range(rows):
            for c, w in self.conn[r].items():
                A["conn_w"][r, c] = w
            k = len(self.ord_kf[r])
            A["ord_kf"][r, :k] = self.ord_kf[r]
            A["ord_w"][r, :k] = self.ord_w[r]
            A["n_ord"][r] = k
            A["covis"][r] = (self.ord_kf[r] + [-1] * N_COVIS)[:N_COVIS]
            A["first_conn"][r] = 1 if self.first_conn[r] else 0
            A["parent"][r] = self.parent[r]
        if self.mirror is not None:
            for k in ("ord_kf", "ord_w", "covis"):
                A[k] = self.mirror[k].copy()
        return A

    @classmethod
    def from_dense(cls, A):
        rows = len(A["n_ord"])
        G = cls(rows)
        for r in range(rows):
            G.conn[r] = {c: int(A["conn_w"][r][c]) for c in range(rows) if A["conn_w"][r][c] != 0}
            k = int(A["n_ord"][r])
            G.ord_kf[r] = [int(x) for x in A["ord_kf"][r][:k]]
            G.ord_w[r] = [int(x) for x in A["ord_w"][r][:k]]
            G.first_conn[r] = bool(A["first_conn"][r])
            G.parent[r] = int(A["parent"][r])
        return G


def _ordered(pairs):
    """sort(vPairs) ascending on (weight, address), then push_front of each (:146-153, :354-361)."""
    lk, lw = [], []
    for w, k in sorted(pairs):
        lk.insert(0, k)
        lw.insert(0, w)
    return lk, lw


def update_best_covisibles(G, c):
    """:138-157: every entry of the weight map, ordered."""
    G.set_lists(c, *_ordered([(w, k) for k, w in sorted(G.conn[c].items())]))


def add_connection(G, c, r, weight, info=None, touched=None):
    """pKF = c ->AddConnection(r, weight), :123-136.  Returns True when the row was re-sorted."""
    if r not in G.conn[c]:
        G.conn[c][r] = weight
    elif G.conn[c][r] != weight:
        G.conn[c][r] = weight
    else:
        _count(info, "equal_weight_return")                     # :131-132
        return False
    update_best_covisibles(G, c)
    _count(info, "resort")
    if touched is not None:
        touched.add(c)
    return True


def update_connections(G, r, slot_point, n, obs_start, obs_kf, flags, id0_row=-1, info=None, touched=None):
    """KeyFrame::UpdateConnections of bank row r, :289-379.  Returns the report as a dict of REPORT_FIELDS."""
    counter = {}                                                # KFcounter
    for i in range(int(n[r])):                                  # :302-320
        p = int(slot_point[r][i])
        if p < 0:
            _count(info, "empty_slot")
            continue
        if not (flags[p] & POINT_PRESENT):
            _count(info, "bad_point")
            continue
        for o in range(int(obs_start[p]), int(obs_start[p + 1])):
            k = int(obs_kf[o])
            if k == r:
                _count(info, "own_row_skip")                    # :316
                continue
            counter[k] = counter.get(k, 0) + 1
    rep = dict(status=OK, n_voted=len(counter), n_ordered=len(G.ord_kf[r]), max_row=-1, max_votes=0, parent_set=-1,
               n_resorted=0, fallback=0)
    if not counter:                                             # :323
        _count(info, "empty_counter")
        rep["status"] = EMPTY
        return rep
    nmax, kmax = 0, -1
    pairs = []
    for k in sorted(counter):                                   # :334-346, the map in ascending row order
        if counter[k] > nmax:
            nmax, kmax = counter[k], k
        if counter[k] >= TH:
            pairs.append((counter[k], k))
            rep["n_resorted"] += add_connection(G, k, r, counter[k], info, touched)
    if not pairs:                                               # :348-352
        _count(info, "fallback_to_max")
        rep["fallback"] = 1
        pairs.append((nmax, kmax))
        rep["n_resorted"] += add_connection(G, kmax, r, nmax, info, touched)
    lk, lw = _ordered(pairs)                                    # :354-361
    G.conn[r] = dict(counter)                                   # :367, entries below the threshold included
    G.set_lists(r, lk, lw)                                      # :368-369
    if touched is not None:
        touched.add(r)
    if G.first_conn[r] and r != id0_row:                        # :371-376
        _count(info, "first_connection")
        G.parent[r] = lk[0]
        G.first_conn[r] = False
        rep["parent_set"] = lk[0]
    elif G.first_conn[r]:
        _count(info, "id0_row")
    else:
        _count(info, "not_first_connection")
    rep.update(n_ordered=len(lk), max_row=kmax, max_votes=nmax)
    return rep


def update_connections_list(G, update_rows, slot_point, n, obs_start, obs_kf, flags, id0_row=-1, info=None, touched=None):
    """UpdateConnections for each entry of update_rows in list order.  Returns report [U][8]."""
    out = np.zeros((len(update_rows), 8), np.int32)
    for u, r in enumerate(update_rows):
        rep = update_connections(G, int(r), slot_point, n, obs_start, obs_kf, flags, id0_row, info, touched)
        out[u] = [rep[k] for k in REPORT_FIELDS]
    return out


def best_covisibility_keyframes(G, r, N):
    """:174-182."""
    if len(G.ord_kf[r]) < N:
        return list(G.ord_kf[r])
    return list(G.ord_kf[r][:N])


def fuse_targets(G, cur, nn, nn2, kf_bad=None, info=None):
    """vpTargetKFs of SearchInNeighbors, src/LocalMapping.cc:457-479 (nn = 10 or 20, nn2 = 5 there)."""
    def bad(k):
        return kf_bad is not None and bool(kf_bad[k])
    targets, stamped = [], set()                                # mnFuseTargetForKF == mpCurrentKeyFrame->mnId
    for k in best_covisibility_keyframes(G, cur, nn):           # :460-462
        if bad(k) or k in stamped:                              # :465
            _count(info, "first_bad_or_stamped")
            continue
        targets.append(k)
        stamped.add(k)
        for k2 in best_covisibility_keyframes(G, k, nn2):       # :471-472
            if bad(k2) or k2 in stamped:                        # :475
                _count(info, "second_bad_or_stamped")
                continue
            if k2 == cur:
                _count(info, "second_is_cur")
                continue
            targets.append(k2)                                  # not stamped: it can come again
    if len(G.ord_kf[cur]) < nn:
        _count(info, "fewer_than_nn")
    return targets


def covisible_targets(G, cur_rows, nn, nn2, kf_bad=None, info=None):
    """The lists of orbhip_covisible_targets for each current row: nn2 == 0 is GetBestCovisibilityKeyFrames(nn) verbatim
    (the neighbours of CreateNewMapPoints, src/LocalMapping.cc:210-213, bad rows included), nn2 > 0 the fuse targets."""
    if nn2 == 0:
        return [best_covisibility_keyframes(G, int(c), nn) for c in cur_rows]
    return [fuse_targets(G, int(c), nn, nn2, kf_bad, info) for c in cur_rows]


def children_from_parents(parent, kf_bad=None):
    """mspChildrens of every row as CSR in ascending row order: c is a child of parent[c] unless c is bad, because
    SetBadFlag erases it from its parent (:453-545).  Returns (child_start [rows+1], child)."""
    rows = len(parent)
    lists = [[] for _ in range(rows)]
    for c in range(rows):
        p = int(parent[c])
        if p < 0:
            continue
        if kf_bad is not None and kf_bad[c]:
            continue
        lists[p].append(c)
    start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return start, np.array([c for x in lists for c in x], np.int32)
