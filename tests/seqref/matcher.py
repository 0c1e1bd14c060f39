"""The matchers the timed paths run, restated loop for loop: Frame grid and GetFeaturesInArea (src/Frame.cc),
SearchByProjection x2, SearchForInitialization, ComputeThreeMaxima, DescriptorDistance (src/ORBmatcher.cc) and
Frame::ComputeStereoMatches (src/Frame.cc:466-640).

Inputs are the ones the package and the oracle take: a frame is keypoints + descriptors + mvuRight + image
bounds + scale factors; a projection search takes already projected QUERY_DTYPE records.  The slot state
(`mvpMapPoints` of the searched frame) is modelled by two arrays: which query holds a slot, and whether the
map point in it has observations (`taken` marks slots that hold an observed map point on entry).
"""
import math

import numpy as np

from .extractor import KP_DTYPE, f32, std_round

TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30          # src/ORBmatcher.cc:37-39
FRAME_GRID_COLS, FRAME_GRID_ROWS = 64, 48            # include/Frame.h
INT_MAX = 2 ** 31 - 1

QUERY_DTYPE = np.dtype([("valid", "<i4"), ("u", "<f4"), ("v", "<f4"), ("radius", "<f4"),
                        ("min_level", "<i4"), ("max_level", "<i4"), ("ur", "<f4"),
                        ("level_aux", "<i4"), ("angle", "<f4"), ("observed", "<i4")])


def descriptor_distance(a, b):
    """src/ORBmatcher.cc:1647-1663: popcount of a xor b over 256 bits; b may be a stack of descriptors."""
    x = np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))
    return np.unpackbits(x, axis=-1).sum(-1).astype(np.int64)


class Frame:
    """The Frame fields the matchers read, with the grid of AssignFeaturesToGrid (src/Frame.cc:230-245)."""

    def __init__(self, keys, desc, u_right, bounds, scale_factors):
        self.keys = np.asarray(keys, KP_DTYPE)
        self.N = len(self.keys)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.u_right = np.full(self.N, -1, f32) if u_right is None else np.asarray(u_right, f32)
        self.min_x, self.min_y, self.max_x, self.max_y = (f32(b) for b in bounds)
        self.scale_factors = np.asarray(scale_factors, f32)
        # src/Frame.cc:101-102
        self.inv_w = f32(f32(FRAME_GRID_COLS) / f32(self.max_x - self.min_x))
        self.inv_h = f32(f32(FRAME_GRID_ROWS) / f32(self.max_y - self.min_y))
        self.x, self.y = self.keys["x"], self.keys["y"]
        self.octave = self.keys["octave"]
        grid = [[[] for _ in range(FRAME_GRID_ROWS)] for _ in range(FRAME_GRID_COLS)]
        for i in range(self.N):
            p = self.pos_in_grid(i)
            if p is not None:
                grid[p[0]][p[1]].append(i)
        self.grid = [[np.array(c, np.int64) for c in col] for col in grid]

    def pos_in_grid(self, i):
        """src/Frame.cc:382-392: round() of the float cell coordinate, rejected outside the grid."""
        px = std_round(f32(f32(self.x[i] - self.min_x) * self.inv_w))
        py = std_round(f32(f32(self.y[i] - self.min_y) * self.inv_h))
        if px < 0 or px >= FRAME_GRID_COLS or py < 0 or py >= FRAME_GRID_ROWS:
            return None
        return px, py


def features_in_area(F, x, y, r, min_level=-1, max_level=-1):
    """Frame::GetFeaturesInArea (src/Frame.cc:327-380), indices in the reference's visiting order: cell columns
    ix, then rows iy, then push_back order inside the cell."""
    x, y, r = f32(x), f32(y), f32(r)
    nMinCellX = max(0, int(math.floor(f32(f32(f32(x - F.min_x) - r) * F.inv_w))))
    if nMinCellX >= FRAME_GRID_COLS:
        return np.zeros(0, np.int64)
    nMaxCellX = min(FRAME_GRID_COLS - 1, int(math.ceil(f32(f32(f32(x - F.min_x) + r) * F.inv_w))))
    if nMaxCellX < 0:
        return np.zeros(0, np.int64)
    nMinCellY = max(0, int(math.floor(f32(f32(f32(y - F.min_y) - r) * F.inv_h))))
    if nMinCellY >= FRAME_GRID_ROWS:
        return np.zeros(0, np.int64)
    nMaxCellY = min(FRAME_GRID_ROWS - 1, int(math.ceil(f32(f32(f32(y - F.min_y) + r) * F.inv_h))))
    if nMaxCellY < 0:
        return np.zeros(0, np.int64)
    check_levels = (min_level > 0) or (max_level >= 0)                 # :348
    cells = [F.grid[ix][iy] for ix in range(nMinCellX, nMaxCellX + 1) for iy in range(nMinCellY, nMaxCellY + 1)]
    cand = np.concatenate(cells) if cells else np.zeros(0, np.int64)
    if len(cand) == 0:
        return cand
    keep = np.ones(len(cand), bool)
    if check_levels:                                                   # :361-368
        oc = F.octave[cand]
        keep &= oc >= min_level
        if max_level >= 0:
            keep &= oc <= max_level
    distx = F.x[cand] - x                                              # float32 arrays: one rounding each
    disty = F.y[cand] - y
    keep &= (np.abs(distx) < r) & (np.abs(disty) < r)                  # :373, strict
    return cand[keep]


def compute_three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1601-1642) on the bin sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif f32(max3) < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


FACTOR = f32(f32(1.0) / f32(HISTO_LENGTH))            # :413, :1336  1.0f/HISTO_LENGTH


def rotation_bin(angle1, angle2):
    """:1433-1438 (and :475-480): rot = angle1 - angle2 (+360 if negative), bin = round(rot*factor), 30 -> 0.
    round() is half away from zero; with factor = 1/30 only bins 0..12 occur."""
    rot = f32(f32(angle1) - f32(angle2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = std_round(f32(rot * FACTOR))
    if b == HISTO_LENGTH:
        b = 0
    assert 0 <= b < HISTO_LENGTH
    return b


def _slot_state(F, taken):
    holder = np.full(F.N, -1, np.int64)               # query index now in mvpMapPoints[i], -1 = NULL
    blocked = np.zeros(F.N, bool) if taken is None else np.asarray(taken, bool).copy()   # Observations() > 0
    return holder, blocked


def search_by_projection_frame(F, queries, qdesc, taken=None, check_ori=True):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) after the projection
    (src/ORBmatcher.cc:1380-1467).  Returns (nmatches, assign[N])."""
    q = np.asarray(queries, QUERY_DTYPE)
    qdesc = np.asarray(qdesc, np.uint8).reshape(-1, 32)
    holder, blocked = _slot_state(F, taken)
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    for i in range(len(q)):
        if not q["valid"][i]:
            continue
        radius = f32(q["radius"][i])
        idx = features_in_area(F, q["u"][i], q["v"][i], radius, int(q["min_level"][i]), int(q["max_level"][i]))
        if len(idx) == 0:                                                  # :1392
            continue
        dist = descriptor_distance(qdesc[i], F.desc[idx])
        ur = f32(q["ur"][i])
        best_dist, best_idx = 256, -1                                      # :1397-1398
        for i2, d in zip(idx.tolist(), dist.tolist()):
            if blocked[i2]:                                                # :1403-1405
                continue
            if F.u_right[i2] > 0:                                          # :1407-1413
                er = abs(f32(ur - F.u_right[i2]))
                if er > radius:
                    continue
            if d < best_dist:                                              # :1419
                best_dist, best_idx = d, i2
        if best_dist <= TH_HIGH:                                           # :1426
            holder[best_idx] = i
            blocked[best_idx] = bool(q["observed"][i])
            n += 1
            if check_ori:
                hist[rotation_bin(q["angle"][i], F.keys["angle"][best_idx])].append(best_idx)
    if check_ori:                                                          # :1448-1467
        ind = compute_three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b not in ind:
                for s in hist[b]:
                    holder[s] = -1
                    n -= 1
    return n, holder.astype(np.int32)


def search_by_projection_points(F, queries, qdesc, taken=None, nnratio=0.8):
    """ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:51-126); the query carries
    r*mvScaleFactors[nPredictedLevel] as `radius`, mTrackProjXR as `ur` and the level window.  Returns
    (nmatches, assign[N])."""
    q = np.asarray(queries, QUERY_DTYPE)
    qdesc = np.asarray(qdesc, np.uint8).reshape(-1, 32)
    holder, blocked = _slot_state(F, taken)
    ratio = f32(nnratio)
    n = 0
    for i in range(len(q)):
        if not q["valid"][i]:                                              # :54-58
            continue
        radius = f32(q["radius"][i])
        idx = features_in_area(F, q["u"][i], q["v"][i], radius, int(q["min_level"][i]), int(q["max_level"][i]))
        if len(idx) == 0:
            continue
        dist = descriptor_distance(qdesc[i], F.desc[idx])
        ur = f32(q["ur"][i])
        best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1   # :76-80
        for i2, d in zip(idx.tolist(), dist.tolist()):
            if blocked[i2]:                                                # :87-89
                continue
            if F.u_right[i2] > 0:                                          # :91-96
                er = abs(f32(ur - F.u_right[i2]))
                if er > radius:
                    continue
            if d < best_dist:                                              # :102-114
                best_dist2, best_dist = best_dist, d
                best_level2, best_level = best_level, int(F.octave[i2])
                best_idx = i2
            elif d < best_dist2:
                best_level2, best_dist2 = int(F.octave[i2]), d
        if best_dist <= TH_HIGH:                                           # :118-125
            if best_level == best_level2 and f32(best_dist) > f32(ratio * f32(best_dist2)):
                continue
            holder[best_idx] = i
            blocked[best_idx] = bool(q["observed"][i])
            n += 1
    return n, holder.astype(np.int32)


def search_for_initialization(F1, F2, prev_matched, window_size=100, nnratio=0.9, check_ori=True):
    """ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520).  Returns (nmatches, matches12[N1],
    updated prev_matched)."""
    prev = np.asarray(prev_matched, f32).reshape(-1, 2).copy()
    ratio = f32(nnratio)
    m12 = np.full(F1.N, -1, np.int64)
    matched_dist = [INT_MAX] * F2.N
    m21 = [-1] * F2.N
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    for i1 in range(F1.N):
        level1 = int(F1.octave[i1])
        if level1 > 0:                                                     # :422
            continue
        idx = features_in_area(F2, prev[i1, 0], prev[i1, 1], f32(window_size), level1, level1)
        if len(idx) == 0:
            continue
        dist = descriptor_distance(F1.desc[i1], F2.desc[idx])
        best_dist = best_dist2 = INT_MAX
        best_idx2 = -1
        for i2, d in zip(idx.tolist(), dist.tolist()):
            if matched_dist[i2] <= d:                                      # :444
                continue
            if d < best_dist:
                best_dist2, best_dist, best_idx2 = best_dist, d, i2
            elif d < best_dist2:
                best_dist2 = d
        if best_dist <= TH_LOW:                                            # :459
            if f32(best_dist) < f32(f32(best_dist2) * ratio):              # :461, float
                if m21[best_idx2] >= 0:
                    m12[m21[best_idx2]] = -1
                    n -= 1
                m12[i1] = best_idx2
                m21[best_idx2] = i1
                matched_dist[best_idx2] = best_dist
                n += 1
                if check_ori:
                    hist[rotation_bin(F1.keys["angle"][i1], F2.keys["angle"][best_idx2])].append(i1)
    if check_ori:                                                          # :489-512
        ind = compute_three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    n -= 1
    for i1 in range(F1.N):                                                 # :515-517
        if m12[i1] >= 0:
            prev[i1, 0], prev[i1, 1] = F2.x[m12[i1]], F2.y[m12[i1]]
    return n, m12.astype(np.int32), prev


STEREO_EXITS = ("no_candidates", "max_u_negative", "level_gate", "ur_range", "best_dist", "window_edge", "sad_edge", "delta_range",
                "disparity_range", "clamp", "median_cull")


def compute_stereo_matches(keys_l, desc_l, keys_r, desc_r, levels_l, levels_r, scale, inv_scale, mbf, mb, info=None):
    """Frame::ComputeStereoMatches (src/Frame.cc:466-640) on the unpadded pyramid levels of both images.
    `mb` is an explicit argument (the reference reads it before assigning it).
    Returns (number of keypoints with a depth, mvuRight, mvDepth).

    `info`, if a dict, receives what the loop decided: "accepted" {iL: dict(sad, idx_r, vd, delta)} for every left key
    point that reached the disparity assignment (before the median cull), "exit" {iL: name} for every left key point that
    left the loop early or was culled, "count" {name: n} over STEREO_EXITS (level_gate and ur_range count candidates,
    clamp counts accepted key points whose disparity was clamped; the others count left key points), and "median",
    "th_dist", "culled" of the cull (None / [] when nothing was accepted)."""
    count = dict.fromkeys(STEREO_EXITS, 0)
    accepted, exits = {}, {}

    def leave(iL, name):
        count[name] += 1
        exits[iL] = name
    kl = np.asarray(keys_l, KP_DTYPE)
    kr = np.asarray(keys_r, KP_DTYPE)
    dl = np.asarray(desc_l, np.uint8).reshape(-1, 32)
    dr = np.asarray(desc_r, np.uint8).reshape(-1, 32)
    scale = np.asarray(scale, f32)
    inv_scale = np.asarray(inv_scale, f32)
    N = len(kl)
    u_right = np.full(N, -1, f32)
    depth = np.full(N, -1, f32)
    th_orb = (TH_HIGH + TH_LOW) // 2                                       # :471
    n_rows = levels_l[0].shape[0]
    rows = [[] for _ in range(n_rows)]
    for iR in range(len(kr)):                                              # :483-493
        kpY = f32(kr["y"][iR])
        r = f32(f32(2.0) * scale[kr["octave"][iR]])
        maxr = int(math.ceil(f32(kpY + r)))
        minr = int(math.floor(f32(kpY - r)))
        for yi in range(minr, maxr + 1):
            assert 0 <= yi < n_rows
            rows[yi].append(iR)
    minZ = f32(mb)                                                         # :496-498
    minD = f32(0)
    maxD = f32(f32(mbf) / minZ)
    dist_idx = []
    w, L = 5, 5
    for iL in range(N):
        levelL = int(kl["octave"][iL])
        vL, uL = f32(kl["y"][iL]), f32(kl["x"][iL])
        cands = rows[int(vL)]                                              # :511, float index truncated
        if not cands:
            leave(iL, "no_candidates")
            continue
        minU = f32(uL - maxD)
        maxU = f32(uL - minD)
        if maxU < 0:
            leave(iL, "max_u_negative")
            continue
        best_dist, best_idx_r = TH_HIGH, 0                                 # :522-523
        for iR in cands:
            o = int(kr["octave"][iR])
            if o < levelL - 1 or o > levelL + 1:                           # :533
                count["level_gate"] += 1
                continue
            uR = f32(kr["x"][iR])
            if uR >= minU and uR <= maxU:                                  # :538
                d = int(descriptor_distance(dl[iL], dr[iR]))
                if d < best_dist:
                    best_dist, best_idx_r = d, iR
            else:
                count["ur_range"] += 1
        if best_dist >= th_orb:                                            # :552
            leave(iL, "best_dist")
            continue
        uR0 = f32(kr["x"][best_idx_r])
        sfac = inv_scale[levelL]
        suL = std_round(f32(uL * sfac))                                    # :557-559, round()
        svL = std_round(f32(vL * sfac))
        suR0 = std_round(f32(uR0 * sfac))
        Ll, Lr = levels_l[levelL], levels_r[levelL]
        assert svL - w >= 0 and svL + w < Ll.shape[0] and suL - w >= 0 and suL + w < Ll.shape[1]
        IL = Ll[svL - w:svL + w + 1, suL - w:suL + w + 1].astype(np.int64)
        IL = IL - IL[w, w]                                                 # :564-565
        iniu = suR0 + L - w                                                # :573-576
        endu = suR0 + L + w + 1
        if iniu < 0 or endu >= Lr.shape[1]:
            leave(iL, "window_edge")
            continue
        best_sad, best_inc = INT_MAX, 0
        vd = [0] * (2 * L + 1)
        for inc in range(-L, L + 1):                                       # :578-592
            c0 = suR0 + inc - w
            assert c0 >= 0
            IR = Lr[svL - w:svL + w + 1, c0:c0 + 2 * w + 1].astype(np.int64)
            IR = IR - IR[w, w]
            d = f32(np.abs(IL - IR).sum())                                 # cv::norm NORM_L1, exact integer sum
            if d < best_sad:
                best_sad, best_inc = int(d), inc
            vd[L + inc] = d
        if best_inc == -L or best_inc == L:                                # :594-595
            leave(iL, "sad_edge")
            continue
        d1, d2, d3 = vd[L + best_inc - 1], vd[L + best_inc], vd[L + best_inc + 1]
        deltaR = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))   # :602
        if deltaR < -1 or deltaR > 1:
            leave(iL, "delta_range")
            continue
        best_uR = f32(scale[levelL] * f32(f32(f32(suR0) + f32(best_inc)) + deltaR))            # :608
        disparity = f32(uL - best_uR)
        if disparity >= minD and disparity < maxD:                         # :612-622
            if disparity <= 0:
                count["clamp"] += 1
                disparity = f32(0.01)
                best_uR = f32(float(uL) - 0.01)                            # uL - 0.01 in double
            depth[iL] = f32(f32(mbf) / disparity)
            u_right[iL] = best_uR
            dist_idx.append((best_sad, iL))
            accepted[iL] = dict(sad=best_sad, idx_r=best_idx_r, vd=[int(v) for v in vd], delta=deltaR)
        else:
            leave(iL, "disparity_range")
    median = th_dist = None
    if dist_idx:                                                           # :626-639
        dist_idx.sort()
        median = f32(dist_idx[len(dist_idx) // 2][0])
        th_dist = f32(f32(f32(1.5) * f32(1.4)) * median)
        for i in range(len(dist_idx) - 1, -1, -1):
            if f32(dist_idx[i][0]) < th_dist:
                break
            u_right[dist_idx[i][1]] = -1
            depth[dist_idx[i][1]] = -1
            leave(dist_idx[i][1], "median_cull")
    if info is not None:
        info.update(accepted=accepted, exit=exits, count=count, median=median, th_dist=th_dist,
                    culled=sorted(i for i, e in exits.items() if e == "median_cull"))
    return int((depth > 0).sum()), u_right, depth
