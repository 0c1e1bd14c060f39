"""ORBextractor (src/ORBextractor.cc) restated loop for loop, with the OpenCV primitives it calls.

Float expressions are evaluated one float32 operation at a time (numpy float32 element-wise ops do not
contract into FMAs); integer expressions use Python ints.
"""
import math
import os
import re

import numpy as np

f32 = np.float32

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

PATCH_SIZE = 31           # :72
HALF_PATCH_SIZE = 15      # :73
EDGE_THRESHOLD = 19       # :74

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# -- rounding ----------------------------------------------------------------------------------------------

def cv_round(x):
    """cvRound rounds half to even."""
    return int(np.rint(np.float64(x)))


def std_round(x):
    """std::round / round(): half away from zero; exact for a float32 argument (|x| + 0.5 is exact in double)."""
    d = float(x)
    return int(math.copysign(math.floor(abs(d) + 0.5), d))


# -- constructor tables (:410-470) -------------------------------------------------------------------------

def tables(nfeatures, scale_factor, nlevels):
    sf = np.zeros(nlevels, f32)
    sf[0] = 1.0
    for i in range(1, nlevels):                                       # :419-423
        sf[i] = f32(sf[i - 1] * f32(scale_factor))
    inv = np.array([f32(f32(1.0) / s) for s in sf], f32)              # :427-431
    factor = f32(f32(1.0) / f32(scale_factor))                        # :436
    # :437, all float: nfeatures*(1 - factor) / (1 - (float)pow((double)factor, (double)nlevels))
    ndes = f32(f32(f32(nfeatures) * f32(f32(1.0) - factor)) /
               f32(f32(1.0) - f32(math.pow(float(factor), float(nlevels)))))
    feat = []
    total = 0
    for _ in range(nlevels - 1):                                      # :440-445
        feat.append(cv_round(ndes))
        total += feat[-1]
        ndes = f32(ndes * factor)
    feat.append(max(nfeatures - total, 0))                            # :446
    umax = [0] * (HALF_PATCH_SIZE + 1)                                # :454-469
    vmax = int(math.floor(HALF_PATCH_SIZE * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(HALF_PATCH_SIZE * math.sqrt(2.0) / 2))
    hp2 = float(HALF_PATCH_SIZE * HALF_PATCH_SIZE)
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(hp2 - v * v))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return dict(scale=sf, inv_scale=inv, feat=feat, umax=umax)


def level_sizes(cols, rows, inv_scale):
    """:1111-1112  Size(cvRound((float)cols*scale), cvRound((float)rows*scale))."""
    return [(cv_round(f32(f32(cols) * s)), cv_round(f32(f32(rows) * s))) for s in inv_scale]


# -- OpenCV primitives ------------------------------------------------------------------------------------

def resize_linear(src, dw, dh):
    """cv::resize INTER_LINEAR on 8U: the Q11 fixed-point bilinear formula (2048 = 1 << 11 per axis,
    horizontal sums >> 4 before the vertical pass, (. + 2) >> 2 at the end)."""
    sh, sw = src.shape

    def taps(d, s):
        scale = 1.0 / (d / s)                                   # scale = 1./inv_scale, in double
        f = ((np.arange(d) + 0.5) * scale - 0.5).astype(np.float32)
        i = np.floor(f).astype(int)
        f = (f - i).astype(np.float32)
        return i, f
    sx, fx = taps(dw, sw)
    lo, hi = sx < 0, sx >= sw - 1
    fx[lo | hi] = 0
    sx[lo] = 0
    sx[hi] = sw - 1
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(int)
    a1 = np.rint(fx * np.float32(2048)).astype(int)
    sy, fy = taps(dh, sh)
    b0 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(int)
    b1 = np.rint(fy * np.float32(2048)).astype(int)
    y0 = np.clip(sy, 0, sh - 1)
    y1 = np.clip(sy + 1, 0, sh - 1)
    S = src.astype(int)
    x1 = np.minimum(sx + 1, sw - 1)
    Hs = S[:, sx] * a0 + S[:, x1] * a1
    out = (((b0[:, None] * (Hs[y0] >> 4)) >> 16) + ((b1[:, None] * (Hs[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def pad_reflect101(img, b=EDGE_THRESHOLD):
    """copyMakeBorder(..., BORDER_REFLECT_101); numpy 'reflect' is gfedcb|abcdefgh|gfedcba."""
    return np.pad(img, b, mode="reflect")


GAUSS7 = np.array([18, 34, 49, 55, 49, 34, 18])


def gauss7(padded, w=GAUSS7):
    """GaussianBlur(Size(7,7), 2, 2) on 8U: the integer kernel on both passes, (sum + 2^15) >> 16, saturated
    (DESIGN.md section 3).  `padded` carries 3 pixels of border on every side; the result is 6 smaller."""
    p = padded.astype(np.int64)
    h, wd = p.shape[0] - 6, p.shape[1] - 6
    rows = sum(int(w[k]) * p[:, k:k + wd] for k in range(7))
    out = sum(int(w[k]) * rows[k:k + h] for k in range(7))
    return np.minimum((out + 32768) >> 16, 255).astype(np.uint8)


# cv::FAST pattern of 16 pixels on a circle of radius 3 (fast_score.cpp makeOffsets), as (dx, dy)
_CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
           (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_cell(img, t):
    """cv::FAST(img, kps, t, true) (TYPE_9_16) on one (sub-)image -> [(x, y, score)] in emission order.

    Vectorised over the pixels: cornerScore<16> = (max over both polarities and the 16 arcs of 9 of the arc's
    smallest difference) - 1; a pixel is a corner at t iff that score >= t.  Rows/cols [3, dim-3) are tested;
    a corner is kept if its score is strictly greater than its 8 neighbours' (0 for non-corners and for the
    untested frame).  Emission is row-major."""
    h, w = img.shape
    if h < 7 or w < 7:
        return []
    I = img.astype(np.int32)
    c = I[3:h - 3, 3:w - 3]
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in _CIRCLE])
    best = None
    for d in (ring - c, c - ring):
        dd = np.concatenate([d, d[:8]])
        for k in range(16):
            m = dd[k:k + 9].min(0)
            best = m if best is None else np.maximum(best, m)
    score = best - 1
    corner = score >= t
    S = np.zeros((h, w), np.int32)
    S[3:h - 3, 3:w - 3] = np.where(corner, score, 0)
    inner = S[3:h - 3, 3:w - 3]
    keep = corner.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= inner > S[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]
    ys, xs = np.nonzero(keep)
    return [(int(x) + 3, int(y) + 3, int(inner[y, x])) for y, x in zip(ys, xs)]


# cv::fastAtan2 of OpenCV 3.x: degree-7 odd polynomial, coefficients in degrees, float arithmetic
_R2D = f32(180.0 / math.pi)                                  # (float)(180/CV_PI)
ATAN2_P1 = f32(f32(0.9997878412794807) * _R2D)
ATAN2_P3 = f32(f32(-0.3258083974640975) * _R2D)
ATAN2_P5 = f32(f32(0.1555786518463281) * _R2D)
ATAN2_P7 = f32(f32(-0.04432655554792128) * _R2D)
_DBL_EPS_F = f32(2.220446049250313e-16)                      # (float)DBL_EPSILON


def fast_atan2(y, x):
    y, x = f32(y), f32(x)
    ax, ay = f32(abs(x)), f32(abs(y))
    if ax >= ay:
        c = f32(ay / f32(ax + _DBL_EPS_F))
        c2 = f32(c * c)
        a = f32(f32(f32(f32(f32(f32(f32(ATAN2_P7 * c2) + ATAN2_P5) * c2) + ATAN2_P3) * c2) + ATAN2_P1) * c)
    else:
        c = f32(ax / f32(ay + _DBL_EPS_F))
        c2 = f32(c * c)
        p = f32(f32(f32(f32(f32(f32(f32(ATAN2_P7 * c2) + ATAN2_P5) * c2) + ATAN2_P3) * c2) + ATAN2_P1) * c)
        a = f32(f32(90.0) - p)
    if x < 0:
        a = f32(f32(180.0) - a)
    if y < 0:
        a = f32(f32(360.0) - a)
    return a


# -- DistributeOctTree (:481-763) --------------------------------------------------------------------------

class _Node:
    __slots__ = ("UL", "UR", "BL", "BR", "keys", "no_more", "born")


def _new_node(counter):
    n = _Node()
    n.keys, n.no_more = [], False
    n.born = counter[0]            # creation order, for the tie-break of :684
    counter[0] += 1
    return n


def _divide(node, X, Y, counter):
    """ExtractorNode::DivideNode (:481-537); children created n1..n4 in that order."""
    halfX = int(math.ceil(f32(f32(node.UR[0] - node.UL[0]) / f32(2))))
    halfY = int(math.ceil(f32(f32(node.BR[1] - node.UL[1]) / f32(2))))
    n1, n2, n3, n4 = (_new_node(counter) for _ in range(4))
    n1.UL = node.UL
    n1.UR = (node.UL[0] + halfX, node.UL[1])
    n1.BL = (node.UL[0], node.UL[1] + halfY)
    n1.BR = (node.UL[0] + halfX, node.UL[1] + halfY)
    n2.UL = n1.UR
    n2.UR = node.UR
    n2.BL = n1.BR
    n2.BR = (node.UR[0], node.UL[1] + halfY)
    n3.UL = n1.BL
    n3.UR = n1.BR
    n3.BL = node.BL
    n3.BR = (n1.BR[0], node.BL[1])
    n4.UL = n3.UR
    n4.UR = n2.BR
    n4.BL = n3.BR
    n4.BR = node.BR
    for k in node.keys:                                    # :512-526
        if X[k] < n1.UR[0]:
            (n1 if Y[k] < n1.BR[1] else n3).keys.append(k)
        elif Y[k] < n1.BR[1]:
            n2.keys.append(k)
        else:
            n4.keys.append(k)
    for n in (n1, n2, n3, n4):                             # :528-535
        if len(n.keys) == 1:
            n.no_more = True
    return n1, n2, n3, n4


def distribute_octree(X, Y, R, minX, maxX, minY, maxY, N):
    """Indices (into X/Y/R) of the retained keys, in std::list order.  X, Y are relative to the border.

    Octree tie-break: sort() of (size, pointer) pairs at :684 orders equal sizes by heap
    address; the choice is "the node created later goes first", i.e. later-created nodes sort behind earlier
    ones and the loop of :685 walks the sorted vector from its end."""
    X = np.asarray(X, f32)
    Y = np.asarray(Y, f32)
    R = np.asarray(R, f32)
    counter = [0]
    nIni = std_round(f32(f32(maxX - minX) / f32(maxY - minY))) if maxY != minY else 0     # :543
    if nIni == 0:
        nIni = 1               # portrait images (nIni = 0) get one root node
    hX = f32(f32(maxX - minX) / f32(nIni))                                                # :545
    nodes = []                 # the std::list; front = index 0
    ini = []
    for i in range(nIni):                                                                 # :552-563
        ni = _new_node(counter)
        ni.UL = (int(f32(hX * f32(i))), 0)
        ni.UR = (int(f32(hX * f32(i + 1))), 0)
        ni.BL = (ni.UL[0], maxY - minY)
        ni.BR = (ni.UR[0], maxY - minY)
        nodes.append(ni)
        ini.append(ni)
    for k in range(len(X)):                                                               # :566-570
        ini[int(f32(X[k] / hX))].keys.append(k)
    kept = []
    for n in nodes:                                                                       # :572-585
        if len(n.keys) == 1:
            n.no_more = True
        if len(n.keys):
            kept.append(n)
    nodes = kept

    finish = False
    while not finish:                                                                     # :594-739
        prev_size = len(nodes)
        n_expand = 0
        size_ptr = []
        pushed = []            # push_front order: the list becomes reversed(pushed) + the nodes not divided
        rest = []
        for n in nodes:
            if n.no_more:
                rest.append(n)
                continue
            for c in _divide(n, X, Y, counter):
                if len(c.keys) > 0:
                    pushed.append(c)
                    if len(c.keys) > 1:
                        n_expand += 1
                        size_ptr.append(c)
        nodes = pushed[::-1] + rest
        if len(nodes) >= N or len(nodes) == prev_size:                                    # :669-672
            finish = True
        elif len(nodes) + n_expand * 3 > N:                                               # :673
            while not finish:                                                             # :676-737
                prev_size = len(nodes)
                prev = sorted(size_ptr, key=lambda n: (len(n.keys), n.born))
                size_ptr = []
                for j in range(len(prev) - 1, -1, -1):
                    node = prev[j]
                    for c in _divide(node, X, Y, counter):
                        if len(c.keys) > 0:
                            nodes.insert(0, c)
                            if len(c.keys) > 1:
                                size_ptr.append(c)
                    for i, m in enumerate(nodes):                                         # :728
                        if m is node:
                            del nodes[i]
                            break
                    if len(nodes) >= N:
                        break
                if len(nodes) >= N or len(nodes) == prev_size:
                    finish = True
    out = []
    for n in nodes:                                                                       # :744-760
        best = n.keys[0]
        for k in n.keys[1:]:
            if R[k] > R[best]:
                best = k
        out.append(best)
    return out


# -- IC_Angle (:77-104) and computeOrbDescriptor (:108-147) ------------------------------------------------

def ic_angle(level, x, y, umax):
    """Integer moments exactly as the loops of :84-101, vectorised over keypoints at integer (x, y)."""
    cx = np.asarray(x, np.int64)
    cy = np.asarray(y, np.int64)
    I = level.astype(np.int64)
    m10 = np.zeros(len(cx), np.int64)
    m01 = np.zeros(len(cx), np.int64)
    for u in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        m10 += u * I[cy, cx + u]
    for v in range(1, HALF_PATCH_SIZE + 1):
        d = umax[v]
        vsum = np.zeros(len(cx), np.int64)
        for u in range(-d, d + 1):
            plus, minus = I[cy + v, cx + u], I[cy - v, cx + u]
            vsum += plus - minus
            m10 += u * (plus + minus)
        m01 += v * vsum
    return np.array([fast_atan2(f32(a), f32(b)) for a, b in zip(m01.tolist(), m10.tolist())], f32)


def load_pattern():
    """bit_pattern_31_ (:150-406), parsed as data from the committed table: 512 points (x, y)."""
    txt = open(os.path.join(_ROOT, "oracle", "rbrief_pattern.h")).read()
    vals = [int(v) for v in re.findall(r"-?\d+", txt.split("{", 1)[1].split("}")[0])]
    assert len(vals) == 1024
    return np.array(vals, np.int64).reshape(512, 2)


FACTOR_PI = f32(math.pi / 180.0)          # :107 (float)(CV_PI/180.f)


def describe(blurred, x, y, angle, pattern, border):
    """computeOrbDescriptor for keypoints at integer level coordinates (x, y); `blurred` is the blurred level
    with `border` pixels of frame around it.

    det_sincos: (float)cos(angle) is the correctly rounded float of the cosine of the
    float angle.  No FMA contraction: x*b + y*a is two float32 products and one float32 sum.  cvRound of the
    rotated coordinates rounds half to even."""
    out = np.zeros((len(x), 32), np.uint8)
    px = pattern[:, 0].astype(f32)
    py = pattern[:, 1].astype(f32)
    weights = (1 << np.arange(8)).astype(np.int64)
    for i in range(len(x)):
        ang = f32(f32(angle[i]) * FACTOR_PI)
        a = f32(math.cos(float(ang)))
        b = f32(math.sin(float(ang)))
        ry = np.rint((px * b) + (py * a)).astype(np.int64)
        rx = np.rint((px * a) - (py * b)).astype(np.int64)
        cx, cy = int(x[i]) + border, int(y[i]) + border
        assert ry.min() + cy >= 0 and rx.min() + cx >= 0
        vals = blurred[cy + ry, cx + rx].astype(np.int32)
        bits = (vals[0::2] < vals[1::2]).astype(np.int64).reshape(32, 8)
        out[i] = (bits * weights).sum(1).astype(np.uint8)
    return out


# -- the extractor: ComputePyramid (:1107-1132), ComputeKeyPointsOctTree (:765-853), operator() (:1043-1105)

def compute_pyramid(img, inv_scale):
    """Unpadded levels and their 19-px REFLECT_101 frames (the level ROI inside `temp`)."""
    levels, padded = [], []
    for level, s in enumerate(inv_scale):
        if level == 0:
            lv = np.ascontiguousarray(img, np.uint8)
        else:
            w = cv_round(f32(f32(img.shape[1]) * s))
            h = cv_round(f32(f32(img.shape[0]) * s))
            lv = resize_linear(levels[-1], w, h)                # :1120, from the previous level
        levels.append(lv)
        padded.append(pad_reflect101(lv))
    return levels, padded


def level_candidates(level_img, ini_th, min_th):
    """:773-829, the per-cell FAST with the per-cell iniThFAST -> minThFAST retry.  Returns (X, Y, R) relative
    to (minBorderX, minBorderY), in push_back order."""
    W = f32(30)                                                       # :769
    minBorderX = EDGE_THRESHOLD - 3
    minBorderY = minBorderX
    maxBorderX = level_img.shape[1] - EDGE_THRESHOLD + 3
    maxBorderY = level_img.shape[0] - EDGE_THRESHOLD + 3
    width = f32(maxBorderX - minBorderX)
    height = f32(maxBorderY - minBorderY)
    nCols = int(f32(width / W))
    nRows = int(f32(height / W))
    wCell = int(math.ceil(f32(width / f32(nCols))))
    hCell = int(math.ceil(f32(height / f32(nRows))))
    X, Y, R = [], [], []
    for i in range(nRows):
        iniY = f32(minBorderY + i * hCell)
        maxY = f32(iniY + f32(hCell + 6))
        if iniY >= maxBorderY - 3:
            continue
        if maxY > maxBorderY:
            maxY = f32(maxBorderY)
        for j in range(nCols):
            iniX = f32(minBorderX + j * wCell)
            maxX = f32(iniX + f32(wCell + 6))
            if iniX >= maxBorderX - 6:
                continue
            if maxX > maxBorderX:
                maxX = f32(maxBorderX)
            cell = level_img[int(iniY):int(maxY), int(iniX):int(maxX)]
            keys = fast_cell(cell, ini_th)
            if not keys:
                keys = fast_cell(cell, min_th)
            for (kx, ky, s) in keys:                                  # :818-826
                X.append(f32(f32(kx) + f32(j * wCell)))
                Y.append(f32(f32(ky) + f32(i * hCell)))
                R.append(f32(s))
    return X, Y, R, (minBorderX, maxBorderX, minBorderY, maxBorderY)


def extract(img, nfeatures=1000, scale=1.2, nlevels=8, ini_th=20, min_th=7, return_levels=False):
    """ORBextractor::operator() -> (keypoints KP_DTYPE[n], descriptors uint8[n, 32]) [, unpadded levels]."""
    img = np.asarray(img, np.uint8)
    T = tables(nfeatures, scale, nlevels)
    if img.size == 0:                                                 # :1046
        e = (np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8))
        return e + ([],) if return_levels else e
    levels, padded = compute_pyramid(img, T["inv_scale"])
    pattern = load_pattern()
    all_k, all_d = [], []
    for level in range(nlevels):
        X, Y, R, (minBX, maxBX, minBY, maxBY) = level_candidates(levels[level], ini_th, min_th)
        sel = distribute_octree(X, Y, R, minBX, maxBX, minBY, maxBY, T["feat"][level])     # :834-835
        k = np.zeros(len(sel), KP_DTYPE)
        k["x"] = [f32(X[s] + f32(minBX)) for s in sel]                # :841-847
        k["y"] = [f32(Y[s] + f32(minBY)) for s in sel]
        k["response"] = [R[s] for s in sel]
        k["octave"] = level
        k["size"] = f32(int(f32(f32(PATCH_SIZE) * T["scale"][level])))   # :837, int scaledPatchSize
        k["class_id"] = -1
        if len(k):
            k["angle"] = ic_angle(levels[level], k["x"].astype(np.int64), k["y"].astype(np.int64), T["umax"])
            # :1085-1090: GaussianBlur (REFLECT_101, the values the 19-px frame holds), descriptors at the
            # unscaled level coordinates; gauss7 of the padded level leaves a 16-px frame
            blurred = gauss7(padded[level])
            all_d.append(describe(blurred, k["x"], k["y"], k["angle"], pattern, EDGE_THRESHOLD - 3))
            if level != 0:                                            # :1095-1101
                s = T["scale"][level]
                k["x"] = k["x"] * s
                k["y"] = k["y"] * s
        all_k.append(k)
    kps = np.concatenate(all_k)
    desc = np.concatenate(all_d) if all_d else np.zeros((0, 32), np.uint8)
    return (kps, desc, levels) if return_levels else (kps, desc)
