"""Sequential restatement of the local-map bookkeeping of Tracking::TrackLocalMap, loop for loop from the cited lines:

  Tracking::UpdateLocalKeyFrames   src/Tracking.cc:1231-1339
  Tracking::UpdateLocalPoints      src/Tracking.cc:1205-1228
  Tracking::SearchLocalPoints      src/Tracking.cc:1146-1180 (the two loops in front of the search)
  SearchByProjection's slot test   src/ORBmatcher.cc:84-86

over tables instead of the map graph: slot_point [rows][cap] = mvpMapPoints of each bank row (-1 = none) with n [rows];
the observation table obs_start [np+1] / obs_kf of seqref.mappoint; flags [np] with POINT_PRESENT = !isBad() and
POINT_OBSERVED = Observations() > 0; kf_bad [rows]; covis [rows][10] = the head of mvpOrderedConnectedKeyFrames, -1 padded;
children as CSR child_start [rows+1] / child; parent [rows] (-1 = none).

Where the reference iterates a map<KeyFrame*, int> or a set<KeyFrame*> in heap-address order, the order here is the
table's: ascending bank row for the vote map, the caller's order for the children.

Like the rest of seqref it imports neither the oracle nor the package."""
import numpy as np

from .projection import POINT_OBSERVED, POINT_PRESENT

OK, NO_VOTES, ALL_BAD = 0, 1, 2
WALK_EXHAUSTED, WALK_LIMIT, WALK_PARENT = 0, 1, 2
MAX_LOCAL_KF = 80          # :1285
N_COVISIBLE = 10           # GetBestCovisibilityKeyFrames(10), :1290
REPORT_FIELDS = ("status", "n_voted", "n_local_kf", "ref_row", "ref_votes", "walk_end", "n_local_points", "n_to_match")


def update_local_keyframes(frame_point, slot_point, n, obs_start, obs_kf, flags, kf_bad, covis, child_start, child, parent,
                           local_kf):
    """UpdateLocalKeyFrames for one frame.  frame_point = mCurrentFrame.mvpMapPoints as point indices (its N entries);
    local_kf = the previous mvpLocalKeyFrames.  Returns (frame_point, votes[rows], local_kf, report) with report =
    {status, n_voted, n_local_kf, ref_row, ref_votes, walk_end}; ref_row -1 = mpReferenceKF unchanged."""
    rows = len(n)
    frame_point = np.array(frame_point, np.int32).copy()
    votes = np.zeros(rows, np.int32)                            # keyframeCounter
    for i in range(len(frame_point)):                           # :1235-1251
        p = int(frame_point[i])
        if p < 0:
            continue
        if flags[p] & POINT_PRESENT:
            for o in range(int(obs_start[p]), int(obs_start[p + 1])):
                votes[int(obs_kf[o])] += 1
        else:
            frame_point[i] = -1                                 # :1248
    n_voted = int((votes > 0).sum())
    rep = dict(status=OK, n_voted=n_voted, n_local_kf=len(local_kf), ref_row=-1, ref_votes=0, walk_end=WALK_EXHAUSTED)
    if n_voted == 0:                                            # :1253
        rep["status"] = NO_VOTES
        return frame_point, votes, [int(r) for r in local_kf], rep

    def bad(r):
        return kf_bad is not None and bool(kf_bad[r])

    vmax, kfmax = 0, -1
    out, stamped = [], set()                                    # mvpLocalKeyFrames, mnTrackReferenceForFrame == mnId
    for r in range(rows):                                       # :1263-1278, the map in ascending row order
        if votes[r] == 0:
            continue
        if bad(r):
            continue
        if votes[r] > vmax:
            vmax, kfmax = int(votes[r]), r
        out.append(r)
        stamped.add(r)
    n_first = len(out)                                          # itEndKF, taken before the loop
    for v in range(n_first):                                    # :1282-1332
        if len(out) > MAX_LOCAL_KF:                             # :1285
            rep["walk_end"] = WALK_LIMIT
            break
        r = out[v]
        for c in covis[r][:N_COVISIBLE]:                        # :1292-1304
            c = int(c)
            if c < 0:
                continue
            if not bad(c) and c not in stamped:
                out.append(c)
                stamped.add(c)
                break
        for o in range(int(child_start[r]), int(child_start[r + 1])):     # :1306-1319
            c = int(child[o])
            if c < 0:
                continue
            if not bad(c) and c not in stamped:
                out.append(c)
                stamped.add(c)
                break
        pr = int(parent[r])                                     # :1321-1330, no isBad test
        if pr >= 0 and pr not in stamped:
            out.append(pr)
            stamped.add(pr)
            rep["walk_end"] = WALK_PARENT
            break                                               # leaves the walk, not the visit
    rep["n_local_kf"] = len(out)
    if kfmax >= 0:                                              # :1334-1338
        rep["ref_row"], rep["ref_votes"] = kfmax, vmax
    else:
        rep["status"] = ALL_BAD
    return frame_point, votes, out, rep


def update_local_points(local_kf, slot_point, n, flags):
    """UpdateLocalPoints (:1209-1227): the point indices of mvpLocalMapPoints in push_back order, and the number of slots met
    that hold a good point (what the de-duplication starts from)."""
    out, seen, met = [], set(), 0
    for r in local_kf:
        for i in range(int(n[r])):
            p = int(slot_point[r][i])
            if p < 0:
                continue
            if not (flags[p] & POINT_PRESENT):
                continue
            met += 1
            if p in seen:                                       # mnTrackReferenceForFrame == mnId
                continue
            out.append(p)
            seen.add(p)
    return out, met


def update_local_map(T, frame_point, frame_n, local_kf, n_local_kf, pcap=None):
    """The whole bookkeeping for every frame of frame_point [frames][cap].  T: a namespace / dict of the tables (slot_point, n,
    obs_start, obs_kf, flags, kf_bad, covis, child_start, child, parent, world, normal, max_dist, min_dist, point_desc).
    local_kf [frames][rows] / n_local_kf [frames]: the previous lists.  Returns a dict of arrays in the layout of
    orbhip_update_local_map_device; rows past the counts are not part of the answer (the tests fill them with sentinels)."""
    g = (lambda k: T[k]) if isinstance(T, dict) else (lambda k: getattr(T, k))
    slot_point, n, flags = g("slot_point"), g("n"), np.asarray(g("flags"), np.uint8)
    frames, cap = np.asarray(frame_point).shape
    rows = len(n)
    pcap = len(flags) if pcap is None else pcap
    R = dict(frame_point=np.array(frame_point, np.int32).copy(), votes=np.zeros((frames, rows), np.int32),
             local_kf=[None] * frames, local_point=[None] * frames, flags_l=[None] * frames,
             taken=np.zeros((frames, cap), np.uint8), report=np.zeros((frames, 8), np.int32), met=[0] * frames)
    for f in range(frames):
        nf = int(frame_n[f])
        fp, votes, kfs, rep = update_local_keyframes(R["frame_point"][f][:nf], slot_point, n, g("obs_start"), g("obs_kf"), flags,
                                                     g("kf_bad"), g("covis"), g("child_start"), g("child"), g("parent"),
                                                     list(local_kf[f][:int(n_local_kf[f])]))
        R["frame_point"][f][:nf] = fp
        R["votes"][f] = votes
        R["local_kf"][f] = np.array(kfs, np.int32)
        pts, R["met"][f] = update_local_points(kfs, slot_point, n, flags)
        held = set(int(p) for p in fp if p >= 0)                # mnLastFrameSeen == mnId, :1158 / :1170
        fl = np.zeros(len(pts), np.uint8)
        for e, p in enumerate(pts):
            if p not in held:                                   # the query's `observed` is pMP->Observations() > 0
                fl[e] = POINT_PRESENT | (flags[p] & POINT_OBSERVED)
        R["local_point"][f] = np.array(pts, np.int32)
        R["flags_l"][f] = fl
        for i in range(nf):                                     # src/ORBmatcher.cc:84-86
            p = int(fp[i])
            R["taken"][f][i] = 1 if p >= 0 and (flags[p] & POINT_OBSERVED) else 0
        R["report"][f] = [rep["status"], rep["n_voted"], rep["n_local_kf"], rep["ref_row"], rep["ref_votes"], rep["walk_end"],
                          len(pts), 0]
    return R


def gather(T, pts):
    """The five per-point arrays in local-list order."""
    g = (lambda k: T[k]) if isinstance(T, dict) else (lambda k: getattr(T, k))
    idx = np.asarray(pts, np.int64)
    return (np.asarray(g("world"), np.float32).reshape(-1, 3)[idx], np.asarray(g("normal"), np.float32).reshape(-1, 3)[idx],
            np.asarray(g("max_dist"), np.float32)[idx], np.asarray(g("min_dist"), np.float32)[idx],
            np.asarray(g("point_desc"), np.uint8).reshape(-1, 32)[idx])


def apply_assignment(frame_point, local_point, assign):
    """F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:122): assign[i] = local entry held by key point i or -1."""
    fp = np.array(frame_point, np.int32).copy()
    for i, a in enumerate(assign):
        if a >= 0:
            fp[i] = local_point[a]
    return fp
