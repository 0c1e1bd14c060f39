"""The geometry in front of the window searches, and the Fuse / SearchBySim3 family, restated from the reference text:
the prologue of SearchByProjection(CurrentFrame, LastFrame) (src/ORBmatcher.cc:1338-1390), Frame::isInFrustum
(src/Frame.cc:269-325) with MapPoint::PredictScale (src/MapPoint.cc:385-418) and the window of
SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:49-69, :131-137), both ORBmatcher::Fuse overloads
(:825-950, :977-1079) and ORBmatcher::SearchBySim3 (:1102-1326).

Two layers per function.

* The LITERAL layer is fp32, and fp64 exactly where the C++ promotes, one numpy scalar operation per C++ operation,
  sequentially per point, in the operation order of DESIGN.md section 3 ("Operation order of the projection prologues")
  where a cv::Mat expression leaves it open.  `logf` is the correctly rounded float logarithm (decimal ln() at 60 digits,
  rounded once).  It returns QUERY_DTYPE records as the entry points of the package do: a point that is skipped is an
  all-zero record.
* The FLOAT64 layer (`*_f64`) states the same geometry plainly with numpy matrix products in fp64, no stated order, and
  returns the values and the signed margin of every decision to its threshold (>= 0 passes, except where noted).

Like the rest of seqref it imports neither the oracle nor the package.
"""
import decimal
import math
from types import SimpleNamespace

import numpy as np

from .matcher import TH_HIGH, descriptor_distance, features_in_area

f32, f64 = np.float32, np.float64

QUERY_DTYPE = np.dtype([("valid", "<i4"), ("u", "<f4"), ("v", "<f4"), ("radius", "<f4"),
                        ("min_level", "<i4"), ("max_level", "<i4"), ("ur", "<f4"),
                        ("level_aux", "<i4"), ("angle", "<f4"), ("observed", "<i4")])
POINT_PRESENT, POINT_OBSERVED = 1, 2       # map point exists and is usable; pMP->Observations() > 0

CAMERA_FIELDS = ("fx", "fy", "cx", "cy", "mbf", "mb", "min_x", "min_y", "max_x", "max_y", "log_scale_factor")


def camera(src):
    """The Frame / KeyFrame statics the prologues read (src/Frame.cc:58-121), copied as float32 from any object with
    these attributes; `scale_factors` is mvScaleFactors, `n_levels` mnScaleLevels."""
    cam = SimpleNamespace(**{k: f32(getattr(src, k)) for k in CAMERA_FIELDS})
    cam.n_levels = int(src.n_levels)
    cam.scale_factors = np.array([src.scale_factors[i] for i in range(cam.n_levels)], f32)
    return cam


def _pose(T):
    return np.ascontiguousarray(np.asarray(T, f32)[:3, :4])


# ---- the scalar pieces -----------------------------------------------------------------------------------------

_LN_CTX = decimal.Context(prec=60)
_LOGF = {}


def logf(x):
    """std::log(float): the correctly rounded float logarithm.  ln() in 60-digit decimal arithmetic, rounded ONCE to
    float32 (the nearest of the float32 neighbours of the double nearest to it, so no double rounding)."""
    x = f32(x)
    if np.isnan(x) or x < 0:
        return f32(np.nan)
    if x == 0:
        return f32(-np.inf)
    if np.isinf(x):
        return x
    key = x.tobytes()
    if key not in _LOGF:
        d = _LN_CTX.ln(decimal.Decimal(float(x)))
        c = f32(float(d))
        cands = (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf)))
        _LOGF[key] = min(cands, key=lambda v: abs(_LN_CTX.subtract(decimal.Decimal(float(v)), d)))
    return _LOGF[key]


def mat_vec(T, x, y, z):
    """`R*x + t` for a 3x4 [R | t] (3x3 * 3x1 + 3x1 in CV_32F): per row ((r0*x + r1*y) + r2*z) + t, DESIGN.md section 3."""
    return [(T[r, 0] * x + T[r, 1] * y + T[r, 2] * z) + T[r, 3] for r in range(3)]


def camera_centre(T):
    """`-Rcw.t()*tcw` (src/ORBmatcher.cc:1341, src/Frame.cc:266, :990): per component -((R0i*t0 + R1i*t1) + R2i*t2)."""
    return [-(T[0, i] * T[0, 3] + T[1, i] * T[1, 3] + T[2, i] * T[2, 3]) for i in range(3)]


def norm3(a, b, c):
    """cv::norm (NORM_L2, CV_32F): squares accumulated in double in element order, sqrt in double, rounded once."""
    return f32(np.sqrt(f64(a) * f64(a) + f64(b) * f64(b) + f64(c) * f64(c)))


def dot3(a, b):
    """Mat::dot (CV_32F): products accumulated in double in element order."""
    return f64(a[0]) * f64(b[0]) + f64(a[1]) * f64(b[1]) + f64(a[2]) * f64(b[2])


def level_real(max_dist, dist, cam):
    """`log(ratio)/mfLogScaleFactor` of PredictScale in float (src/MapPoint.cc:390-393)."""
    ratio = f32(max_dist) / f32(dist)
    return logf(ratio) / cam.log_scale_factor


def predict_scale(max_dist, dist, cam):
    """MapPoint::PredictScale (src/MapPoint.cc:385-418): ceil of the float quotient, clamped to [0, nLevels).  The
    conversion of NaN to int is undefined in C++; level 0 is the choice of DESIGN.md section 3."""
    fl = level_real(max_dist, dist, cam)
    if np.isnan(fl):
        return 0
    if np.isinf(fl):
        return 0 if fl < 0 else cam.n_levels - 1
    n = math.ceil(fl)
    if n < 0:
        n = 0
    elif n >= cam.n_levels:
        n = cam.n_levels - 1
    return n


def scale_factor(cam, level):
    """mvScaleFactors[level].  A level outside the table is caller data the reference reads out of bounds with; the
    choice of DESIGN.md section 3: below 0 the first entry, past the end a factor of 0 (an empty window)."""
    if level < 0:
        return cam.scale_factors[0]
    if level >= len(cam.scale_factors):
        return f32(0)
    return cam.scale_factors[level]


def radius_by_viewing_cos(view_cos):
    """src/ORBmatcher.cc:131-137: the float widened to double against the double literal."""
    return f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)


# ---- literal layer: the prologues --------------------------------------------------------------------------------

def project_last_frame(cam, Tcw, Tlw, world, flags, last_keys, th, mono, aux=None):
    """src/ORBmatcher.cc:1338-1390, and :1409 for `ur`.  flags: POINT_PRESENT = `pMP && !mvbOutlier[i]`."""
    Tcw, Tlw, th = _pose(Tcw), _pose(Tlw), f32(th)
    world = np.asarray(world, f32).reshape(-1, 3)
    q = np.zeros(len(world), QUERY_DTYPE)
    with np.errstate(all="ignore"):
        twc = camera_centre(Tcw)                                              # :1341
        tlc_z = mat_vec(Tlw, twc[0], twc[1], twc[2])[2]                       # :1346
        forward = bool(tlc_z > cam.mb) and not mono                           # :1348
        backward = bool(-tlc_z > cam.mb) and not mono                         # :1349
        if aux is not None:
            aux.update(tlc_z=tlc_z, forward=forward, backward=backward, zc=np.full(len(world), np.nan, f32))
        for i in range(len(world)):
            if not flags[i] & POINT_PRESENT:                                  # :1355-1357
                continue
            xc, yc, zc = mat_vec(Tcw, world[i, 0], world[i, 1], world[i, 2])  # :1361
            if aux is not None:
                aux["zc"][i] = zc
            invzc = f32(f64(1.0) / f64(zc))                                   # :1365  const float invzc = 1.0/z
            if invzc < 0:                                                     # :1367
                continue
            u = cam.fx * xc * invzc + cam.cx                                  # :1370
            v = cam.fy * yc * invzc + cam.cy
            if u < cam.min_x or u > cam.max_x:                                # :1373
                continue
            if v < cam.min_y or v > cam.max_y:                                # :1375
                continue
            o = int(last_keys["octave"][i])                                   # :1378
            r = q[i]
            r["valid"], r["u"], r["v"] = 1, u, v
            r["radius"] = th * scale_factor(cam, o)                           # :1381
            if forward:                                                       # :1385-1390
                r["min_level"], r["max_level"] = o, -1
            elif backward:
                r["min_level"], r["max_level"] = 0, o
            else:
                r["min_level"], r["max_level"] = o - 1, o + 1
            r["ur"] = u - cam.mbf * invzc                                     # :1409
            r["level_aux"], r["angle"] = o, last_keys["angle"][i]
            r["observed"] = 1 if flags[i] & POINT_OBSERVED else 0
    return q


def frustum_queries(cam, Tcw, world, normal, max_dist, min_dist, flags, viewing_cos_limit, th, aux=None):
    """Frame::isInFrustum (src/Frame.cc:269-325), PredictScale, and the window of SearchByProjection(F, vpMapPoints, th)
    (src/ORBmatcher.cc:49-69).  Returns (queries, mTrackViewCos)."""
    Tcw, th, limit = _pose(Tcw), f32(th), f32(viewing_cos_limit)
    world, normal = np.asarray(world, f32).reshape(-1, 3), np.asarray(normal, f32).reshape(-1, 3)
    max_dist, min_dist = np.asarray(max_dist, f32), np.asarray(min_dist, f32)
    n = len(world)
    q, view_cos = np.zeros(n, QUERY_DTYPE), np.zeros(n, f32)
    b_factor = f64(th) != 1.0                                                 # ORBmatcher.cc:49
    if aux is not None:
        aux.update(zc=np.full(n, np.nan, f32), dist=np.full(n, np.nan, f32), view_cos=np.full(n, np.nan, f32),
                   level_real=np.full(n, np.nan, f32))
    with np.errstate(all="ignore"):
        Ow = camera_centre(Tcw)                                               # Frame.cc:266
        for i in range(n):
            if not flags[i] & POINT_PRESENT:
                continue
            P = world[i]
            PcX, PcY, PcZ = mat_vec(Tcw, P[0], P[1], P[2])                    # :277
            if aux is not None:
                aux["zc"][i] = PcZ
            if PcZ < f32(0.0):                                                # :283
                continue
            invz = f32(1.0) / PcZ                                             # :287
            u = cam.fx * PcX * invz + cam.cx                                  # :288
            v = cam.fy * PcY * invz + cam.cy
            if u < cam.min_x or u > cam.max_x:                                # :291
                continue
            if v < cam.min_y or v > cam.max_y:                                # :293
                continue
            max_distance = f32(1.2) * max_dist[i]                             # MapPoint.cc:382
            min_distance = f32(0.8) * min_dist[i]                             # MapPoint.cc:376
            PO = (P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2])                   # :299
            dist = norm3(*PO)                                                 # :300
            if aux is not None:
                aux["dist"][i] = dist
            if dist < min_distance or dist > max_distance:                    # :302
                continue
            vc = f32(dot3(PO, normal[i]) / f64(dist))                         # :308
            if aux is not None:
                aux["view_cos"][i] = vc
            if vc < limit:                                                    # :310
                continue
            level = predict_scale(max_dist[i], dist, cam)                     # :314
            if aux is not None:
                aux["level_real"][i] = level_real(max_dist[i], dist, cam)
            rad = radius_by_viewing_cos(vc)                                   # ORBmatcher.cc:63
            if b_factor:
                rad = rad * th                                                # ORBmatcher.cc:66
            r = q[i]
            r["valid"], r["u"], r["v"] = 1, u, v
            r["radius"] = rad * scale_factor(cam, level)                      # ORBmatcher.cc:69
            r["min_level"], r["max_level"] = level - 1, level
            r["ur"] = u - cam.mbf * invz                                      # :319
            r["level_aux"] = level
            r["observed"] = 1 if flags[i] & POINT_OBSERVED else 0
            view_cos[i] = vc                                                  # :322
    return q, view_cos


def is_in_image(cam, x, y):
    """KeyFrame::IsInImage (src/KeyFrame.cc:610-613): the upper edges are exclusive."""
    return bool(x >= cam.min_x and x < cam.max_x and y >= cam.min_y and y < cam.max_y)


def keyframe_queries(cam, mode, double_invz, T1, T2, world, normal, max_dist, min_dist, flags, th, aux=None):
    """mode 0: the prologue of ORBmatcher::Fuse, :852-890 (`double_invz` false, `1/z`) and of its Scw overload, :1009-1049
    (`double_invz` true, `1.0/z`); T1 = [Rcw | tcw].  mode 1: one direction of SearchBySim3, :1158-1189 and :1238-1269:
    T1 = the pose of the key frame the points come from, T2 = [sR21 | t21] resp. [sR12 | t12]; no normal gate,
    dist3D = |p3Dc|, no `ur`."""
    T1, th = _pose(T1), f32(th)
    T2 = None if T2 is None else _pose(T2)
    world = np.asarray(world, f32).reshape(-1, 3)
    normal = None if normal is None else np.asarray(normal, f32).reshape(-1, 3)
    max_dist, min_dist = np.asarray(max_dist, f32), np.asarray(min_dist, f32)
    n = len(world)
    q = np.zeros(n, QUERY_DTYPE)
    if aux is not None:
        aux.update(zc=np.full(n, np.nan, f32), dist=np.full(n, np.nan, f32), level_real=np.full(n, np.nan, f32),
                   ncos=np.full(n, np.nan, f64))
    with np.errstate(all="ignore"):
        Ow = camera_centre(T1) if mode == 0 else None                         # :836, :990
        for i in range(n):
            if not flags[i] & POINT_PRESENT:                                  # :846-850, :1005, :1152-1156
                continue
            P = world[i]
            X, Y, Z = mat_vec(T1, P[0], P[1], P[2])                           # :853, :1012, :1159
            if mode == 1:
                X, Y, Z = mat_vec(T2, X, Y, Z)                                # :1160, :1240
            if aux is not None:
                aux["zc"][i] = Z
            if Z < f32(0.0):                                                  # :856, :1015, :1163
                continue
            invz = f32(f64(1.0) / f64(Z)) if double_invz else f32(1) / Z      # :1019, :1166 / :859
            x = X * invz                                                      # :860
            y = Y * invz
            u = cam.fx * x + cam.cx                                           # :863
            v = cam.fy * y + cam.cy
            if not is_in_image(cam, u, v):                                    # :867
                continue
            max_distance = f32(1.2) * max_dist[i]                             # :872-873
            min_distance = f32(0.8) * min_dist[i]
            if mode == 0:
                PO = (P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2])               # :874
                dist3D = norm3(*PO)                                           # :875
            else:
                dist3D = norm3(X, Y, Z)                                       # :1179
            if aux is not None:
                aux["dist"][i] = dist3D
            if dist3D < min_distance or dist3D > max_distance:                # :878
                continue
            if mode == 0:
                d = dot3(PO, normal[i])
                if aux is not None:
                    aux["ncos"][i] = d / f64(dist3D)
                if d < 0.5 * f64(dist3D):                                     # :884
                    continue
            level = predict_scale(max_dist[i], dist3D, cam)                   # :887
            if aux is not None:
                aux["level_real"][i] = level_real(max_dist[i], dist3D, cam)
            r = q[i]
            r["valid"], r["u"], r["v"] = 1, u, v
            r["radius"] = th * scale_factor(cam, level)                       # :890
            r["min_level"], r["max_level"] = level - 1, level                 # :911
            r["ur"] = u - cam.mbf * invz if mode == 0 else f32(0)             # :870
            r["level_aux"] = level
    return q


# ---- literal layer: the searches ---------------------------------------------------------------------------------

def best_in_window(F, queries, qdesc, inv_sigma2=None):
    """The search loop of Fuse (:892-949; `inv_sigma2` = mvInvLevelSigma2 turns the chi-square gate of :914-938 on), of
    its Scw overload (:1051-1079) and of SearchBySim3 (:1191-1219), the last two without a gate.  KeyFrame::GetFeaturesInArea
    (src/KeyFrame.cc:569-608) is Frame::GetFeaturesInArea without a level test, in the same visiting order; the first
    minimum wins (`dist<bestDist`).  Returns (best_idx, best_dist), -1 / 256 where nothing passes."""
    q = np.asarray(queries, QUERY_DTYPE)
    qdesc = np.asarray(qdesc, np.uint8).reshape(-1, 32)
    best_idx, best_dist = np.full(len(q), -1, np.int32), np.full(len(q), 256, np.int32)
    for i in range(len(q)):
        if not q["valid"][i]:
            continue
        u, v, ur = f32(q["u"][i]), f32(q["v"][i]), f32(q["ur"][i])
        if np.isnan(u) or np.isnan(v):                                        # `(int)floor(NaN)` is undefined; no key point
            continue                                                          # is within r of NaN, so the window is empty
        idx = features_in_area(F, u, v, f32(q["radius"][i]))
        if len(idx) == 0:                                                     # :894
            continue
        dist = descriptor_distance(qdesc[i], F.desc[idx])
        lo, hi = int(q["min_level"][i]), int(q["max_level"][i])
        bd, bi = 256, -1                                                      # :901-902
        for j, d in zip(idx.tolist(), dist.tolist()):
            level = int(F.octave[j])
            if level < lo or level > hi:                                      # :911
                continue
            if inv_sigma2 is not None:
                ex, ey = u - F.x[j], v - F.y[j]                               # :920-921
                if F.u_right[j] >= 0:                                         # :914
                    er = ur - F.u_right[j]
                    e2 = ex * ex + ey * ey + er * er                          # :923
                    if f64(e2 * f32(inv_sigma2[level])) > 7.8:                # :925
                        continue
                else:
                    e2 = ex * ex + ey * ey                                    # :934
                    if f64(e2 * f32(inv_sigma2[level])) > 5.99:               # :936
                        continue
            if d < bd:                                                        # :944
                bd, bi = d, j
        best_idx[i], best_dist[i] = bi, bd
    return best_idx, best_dist


def fuse(F, cam, Tcw, world, normal, max_dist, min_dist, flags, point_desc, th, inv_sigma2, sim3_form=False):
    """ORBmatcher::Fuse up to the decision `bestDist<=TH_LOW`: :825-949, or the Scw overload :977-1079 (`sim3_form`: `1.0/z`
    and no chi-square gate; Tcw = [sRcw/scw | t/scw] as :986-989 computes it)."""
    q = keyframe_queries(cam, 0, bool(sim3_form), Tcw, None, world, normal, max_dist, min_dist, flags, th)
    return best_in_window(F, q, point_desc, None if sim3_form else inv_sigma2)


def sim3_matrices(s12, R12, t12):
    """src/ORBmatcher.cc:1119-1121: sR12 = s12*R12; sR21 = (1.0/s12)*R12.t(); t21 = -sR21*t12.  The scalar of a
    Mat-times-scalar expression is a double: each element is the float times the double, rounded once.  Returns the
    3x4 (S12, S21) = ([sR12 | t12], [sR21 | t21])."""
    R12, t12, s12 = np.asarray(R12, f32).reshape(3, 3), np.asarray(t12, f32).reshape(3), f32(s12)
    S12, S21 = np.zeros((3, 4), f32), np.zeros((3, 4), f32)
    inv_s = f64(1.0) / f64(s12)
    for r in range(3):
        for c in range(3):
            S12[r, c] = f32(f64(s12) * f64(R12[r, c]))                        # :1119
            S21[r, c] = f32(inv_s * f64(R12[c, r]))                           # :1120
        S12[r, 3] = t12[r]
    for r in range(3):                                                        # :1121: (-sR21)*t12, 3x3 * 3x1
        S21[r, 3] = (-S21[r, 0]) * t12[0] + (-S21[r, 1]) * t12[1] + (-S21[r, 2]) * t12[2]
    return S12, S21


def search_by_sim3(F1, F2, cam, T1w, T2w, pts1, pts2, th, s12=None, R12=None, t12=None, S12=None, S21=None):
    """ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1102-1326).  pts = (world, max_dist, min_dist, flags, descriptor) per
    key-frame slot; POINT_PRESENT = `pMP && !vbAlreadyMatched && !pMP->isBad()`.  Takes (s12, R12, t12) and composes the
    matrices as :1119-1121 does, or takes S12 / S21 ready-made.  Returns (nFound, matches12[N1])."""
    if S12 is None:
        S12, S21 = sim3_matrices(s12, R12, t12)
    w1, mx1, mn1, fl1, d1 = pts1
    w2, mx2, mn2, fl2, d2 = pts2
    q1 = keyframe_queries(cam, 1, True, T1w, S21, w1, None, mx1, mn1, fl1, th)     # :1148-1189, KF1 points into KF2
    q2 = keyframe_queries(cam, 1, True, T2w, S12, w2, None, mx2, mn2, fl2, th)     # :1228-1269, KF2 points into KF1
    m1, bd1 = best_in_window(F2, q1, d1)
    m2, bd2 = best_in_window(F1, q2, d2)
    match1 = np.where(bd1 <= TH_HIGH, m1, -1)                                 # :1221-1224
    match2 = np.where(bd2 <= TH_HIGH, m2, -1)                                 # :1301-1304
    m12 = np.full(F1.N, -1, np.int32)
    found = 0
    for i1 in range(F1.N):                                                    # :1310-1323
        idx2 = int(match1[i1])
        if idx2 >= 0 and int(match2[idx2]) == i1:
            m12[i1] = idx2
            found += 1
    return found, m12


# ---- float64 layer -------------------------------------------------------------------------------------------------

def _rt(T):
    T = np.asarray(T, f64)[:3, :4]
    return T[:, :3], T[:, 3]


def _project_f64(cam, Pc):
    with np.errstate(all="ignore"):
        u = f64(cam.fx) * Pc[:, 0] / Pc[:, 2] + f64(cam.cx)
        v = f64(cam.fy) * Pc[:, 1] / Pc[:, 2] + f64(cam.cy)
        ur = u - f64(cam.mbf) / Pc[:, 2]
    return u, v, ur


def _image_margins(cam, u, v):
    return dict(u_min=u - f64(cam.min_x), u_max=f64(cam.max_x) - u, v_min=v - f64(cam.min_y), v_max=f64(cam.max_y) - v)


def _range_margins(dist, max_dist, min_dist):
    """Relative to the distance: dist in [0.8 min, 1.2 max]."""
    with np.errstate(all="ignore"):
        return dict(dist_min=(dist - 0.8 * np.asarray(min_dist, f64)) / dist,
                    dist_max=(1.2 * np.asarray(max_dist, f64) - dist) / dist)


def _level_f64(cam, max_dist, dist):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(max_dist, f64) / dist) / math.log(float(cam.scale_factors[1]))


def project_last_frame_f64(cam, Tcw, Tlw, world):
    """Values u, v, ur, zc, tlc_z; margins: depth (zc, metres), image (pixels), forward / backward (metres)."""
    (Rc, tc), (Rl, tl) = _rt(Tcw), _rt(Tlw)
    X = np.asarray(world, f64).reshape(-1, 3)
    Pc = X @ Rc.T + tc
    tlc = Rl @ (-Rc.T @ tc) + tl
    u, v, ur = _project_f64(cam, Pc)
    m = dict(depth=Pc[:, 2], **_image_margins(cam, u, v))
    return dict(u=u, v=v, ur=ur, zc=Pc[:, 2], tlc_z=tlc[2], forward=tlc[2] - f64(cam.mb), backward=-tlc[2] - f64(cam.mb),
                margins=m)


def frustum_queries_f64(cam, Tcw, world, normal, max_dist, min_dist, viewing_cos_limit):
    """Values u, v, ur, zc, dist, view_cos, level_real; margins as above plus the range (relative), the viewing-angle gate
    and the 0.998 switch of RadiusByViewingCos (`radius`: > 0 means 2.5)."""
    R, t = _rt(Tcw)
    X = np.asarray(world, f64).reshape(-1, 3)
    Pc = X @ R.T + t
    PO = X - (-R.T @ t)
    dist = np.linalg.norm(PO, axis=1)
    with np.errstate(all="ignore"):
        vc = (PO * np.asarray(normal, f64).reshape(-1, 3)).sum(1) / dist
    u, v, ur = _project_f64(cam, Pc)
    m = dict(depth=Pc[:, 2], **_image_margins(cam, u, v), **_range_margins(dist, max_dist, min_dist),
             view_cos=vc - f64(f32(viewing_cos_limit)))
    return dict(u=u, v=v, ur=ur, zc=Pc[:, 2], dist=dist, view_cos=vc, radius=vc - 0.998,
                level_real=_level_f64(cam, max_dist, dist), margins=m)


def keyframe_queries_f64(cam, mode, T1, T2, world, normal, max_dist, min_dist):
    """mode 0: Pc = T1 X, dist = |X - Ow|, normal gate `ncos - 0.5`; mode 1: Pc = T2 (T1 X), dist = |Pc|."""
    R, t = _rt(T1)
    X = np.asarray(world, f64).reshape(-1, 3)
    Pc = X @ R.T + t
    out = {}
    if mode == 0:
        PO = X - (-R.T @ t)
        dist = np.linalg.norm(PO, axis=1)
        with np.errstate(all="ignore"):
            out["ncos"] = (PO * np.asarray(normal, f64).reshape(-1, 3)).sum(1) / dist
    else:
        R2, t2 = _rt(T2)
        Pc = Pc @ R2.T + t2
        dist = np.linalg.norm(Pc, axis=1)
    u, v, ur = _project_f64(cam, Pc)
    m = dict(depth=Pc[:, 2], **_image_margins(cam, u, v), **_range_margins(dist, max_dist, min_dist))
    if mode == 0:
        m["normal"] = out["ncos"] - 0.5
    out.update(u=u, v=v, ur=ur, zc=Pc[:, 2], dist=dist, level_real=_level_f64(cam, max_dist, dist), margins=m)
    return out


def sim3_matrices_f64(s12, R12, t12):
    """S12 = [s12 R12 | t12] and its inverse S21 = [R12^T / s12 | -R12^T t12 / s12], in fp64."""
    R12, t12, s = np.asarray(R12, f64).reshape(3, 3), np.asarray(t12, f64).reshape(3), float(s12)
    S12 = np.concatenate([s * R12, t12[:, None]], 1)
    S21 = np.concatenate([R12.T / s, (-(R12.T / s) @ t12)[:, None]], 1)
    return S12, S21
