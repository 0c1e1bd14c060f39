"""Sequential restatement of the two functions that refresh a map point from its observations, loop for loop from the
cited lines:

  MapPoint::ComputeDistinctiveDescriptors  src/MapPoint.cc:242-307
  MapPoint::UpdateNormalAndDepth           src/MapPoint.cc:330-371
  KeyFrame::SetPose (Ow)                   src/KeyFrame.cc:66-77

The observations of point p are the entries obs_start[p] .. obs_start[p+1] of (obs_kf, obs_idx): key point obs_idx[o] of key
frame obs_kf[o], in the caller's order (the reference iterates a map<KeyFrame*, size_t> in heap-address order; the order
decides the float sum of the normal and which of several equal medians wins).  ref_obs[p] is the position of mpRefKF's
observation in the point's list.

Two layers.
* The LITERAL layer (`update_map_points`) does one numpy scalar operation per C++ operation, in the order DESIGN.md
  section 3 states for the cv::Mat expressions: float differences, cv::norm with squares accumulated in double,
  `Mat / double` as the Mat times the double 1.0 / s, the sum of the normal in float in table order.
* The FLOAT64 layer (`normal_and_depth_f64`) states the same geometry plainly in fp64 numpy, no stated order.

Like the rest of seqref it imports neither the oracle nor the package."""
import numpy as np

from .matcher import descriptor_distance
from .projection import POINT_PRESENT, camera_centre, scale_factor

f32, f64 = np.float32, np.float64
UPDATE_DESCRIPTOR, UPDATE_NORMAL_DEPTH = 1, 2
UPDATED, BAD, NO_OBSERVATION, NO_DESCRIPTOR, BAD_REF, TOO_MANY = range(6)
MAX_OBSERVATIONS = 2048


_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distance_rows(descs):
    """Distances[i][j] = ORBmatcher::DescriptorDistance of rows i and j (:276-285).  Short lists go through the scalar
    restatement; long ones take the same numbers from a byte popcount table, 128 rows at a time."""
    N = len(descs)
    if N <= 64:
        return np.array([[descriptor_distance(descs[i], descs[j]) for j in range(N)] for i in range(N)], np.int32).reshape(N, N)
    return np.concatenate([_POPCOUNT[descs[i:i + 128, None, :] ^ descs[None, :, :]].sum(2, dtype=np.int32)
                           for i in range(0, N, 128)])


def distinctive_descriptor(descs):
    """src/MapPoint.cc:272-301 for vDescriptors = descs [N][32]: the index of the descriptor with the least median distance
    to the others, the first one where several share it."""
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    N = len(descs)
    Distances = distance_rows(descs)
    BestMedian, BestIdx = 2 ** 31 - 1, 0
    for i in range(N):
        vDists = np.sort(Distances[i])
        median = int(vDists[int(0.5 * (N - 1))])
        if median < BestMedian:
            BestMedian, BestIdx = median, i
    return BestIdx


def view_direction(T, X):
    """(normali, normali / cv::norm(normali)) for the key frame with pose T (3x4 float32) and the point X."""
    Ow = camera_centre(T)
    d = [X[c] - Ow[c] for c in range(3)]
    norm = np.sqrt(f64(d[0]) * f64(d[0]) + f64(d[1]) * f64(d[1]) + f64(d[2]) * f64(d[2]))     # cv::norm, a double
    inv = f64(1.0) / norm
    return d, [f32(inv * f64(d[c])) for c in range(3)]


def update_map_points(cam, what, Tcw, kf_keys, kf_desc, kf_bad, obs_start, obs_kf, obs_idx, ref_obs, world, flags,
                      point_desc, normal, max_dist, min_dist):
    """cam: seqref.projection.camera(); Tcw [K] poses; kf_keys[k] records with an `octave` field (mvKeysUn), kf_desc[k]
    [n_k][32]; kf_bad [K] or None.  The last four arrays are the current values; updated copies are returned as
    (point_desc, normal, max_dist, min_dist, best_obs, status).  An entry the reference does not write keeps its value;
    best_obs is -1 wherever no descriptor was chosen."""
    n_pts = len(obs_start) - 1
    T = [np.ascontiguousarray(np.asarray(t, f32).reshape(-1, 4)[:3, :4]) for t in Tcw]
    world = np.asarray(world, f32).reshape(-1, 3)
    point_desc = np.array(point_desc, np.uint8).reshape(-1, 32).copy()
    normal = np.array(normal, f32).reshape(-1, 3).copy()
    max_dist, min_dist = np.array(max_dist, f32).copy(), np.array(min_dist, f32).copy()
    best_obs = np.full(n_pts, -1, np.int32)
    status = np.zeros(n_pts, np.uint8)
    with np.errstate(all="ignore"):
        for p in range(n_pts):
            if not (flags[p] & POINT_PRESENT):                      # mbBad, :251, :338
                status[p] = BAD
                continue
            o0, N = int(obs_start[p]), int(obs_start[p + 1]) - int(obs_start[p])
            if N <= 0:                                              # observations.empty(), :256, :345
                status[p] = NO_OBSERVATION
                continue
            if N > MAX_OBSERVATIONS:
                status[p] = TOO_MANY
                continue
            obs = [(int(obs_kf[o0 + j]), int(obs_idx[o0 + j])) for j in range(N)]
            st = UPDATED
            if what & UPDATE_DESCRIPTOR:
                kept = [j for j in range(N) if not (kf_bad is not None and kf_bad[obs[j][0]])]        # :265
                if not kept:                                        # :269
                    st = NO_DESCRIPTOR
                else:
                    vDescriptors = np.stack([kf_desc[obs[j][0]][obs[j][1]] for j in kept])
                    BestIdx = distinctive_descriptor(vDescriptors)
                    point_desc[p] = vDescriptors[BestIdx]           # :305
                    best_obs[p] = kept[BestIdx]
            if what & UPDATE_NORMAL_DEPTH:
                r = int(ref_obs[p])
                if r < 0 or r >= N:
                    st = BAD_REF
                else:
                    X = world[p]
                    nrm = [f32(0), f32(0), f32(0)]                  # cv::Mat::zeros(3,1,CV_32F)
                    n = 0
                    for kf, _ in obs:                               # :350-357
                        _, v = view_direction(T[kf], X)
                        nrm = [nrm[c] + v[c] for c in range(3)]
                        n += 1
                    kf, idx = obs[r]
                    PC, _ = view_direction(T[kf], X)                # Pos - pRefKF->GetCameraCenter()
                    dist = f32(np.sqrt(f64(PC[0]) * f64(PC[0]) + f64(PC[1]) * f64(PC[1]) + f64(PC[2]) * f64(PC[2])))
                    level = int(kf_keys[kf]["octave"][idx])
                    mx = dist * scale_factor(cam, level)            # :367
                    max_dist[p] = mx
                    min_dist[p] = mx / cam.scale_factors[cam.n_levels - 1]
                    inv = f64(1.0) / f64(n)
                    normal[p] = [f32(inv * f64(nrm[c])) for c in range(3)]                           # :369
            status[p] = st
    return point_desc, normal, max_dist, min_dist, best_obs, status


def normal_and_depth_f64(cam, Tcw, kf_keys, obs, ref, X):
    """UpdateNormalAndDepth of one point in plain fp64: obs = [(kf, idx)], ref a position in it.  Returns
    (normal[3], max_dist, min_dist) as float64."""
    X = np.asarray(X, f64)
    sf = np.asarray(cam.scale_factors, f64)

    def centre(k):
        T = np.asarray(Tcw[k], f64).reshape(-1, 4)[:3, :4]
        return -T[:, :3].T @ T[:, 3]

    dirs = [(X - centre(k)) / np.linalg.norm(X - centre(k)) for k, _ in obs]
    kf, idx = obs[ref]
    level = int(kf_keys[kf]["octave"][idx])
    s = sf[0] if level < 0 else (0.0 if level >= cam.n_levels else sf[level])
    mx = np.linalg.norm(X - centre(kf)) * s
    return np.sum(dirs, axis=0) / len(obs), mx, mx / sf[cam.n_levels - 1]
