"""Host-side mirror of class ORBmatcher (include/ORBmatcher.h:37-103) and of
Frame::ComputeStereoMatches (src/Frame.cc:466-640) over the C ABI.

`FrameView` carries the handful of Frame fields the matchers read (mvKeysUn,
mDescriptors, mvuRight, image bounds, 64x48 grid scale, mvScaleFactors).  The
projection that precedes the two SearchByProjection searches
(src/ORBmatcher.cc:1360-1390, src/Frame.cc:269-325) is done by the caller and
arrives as `QUERY_DTYPE` records; `project_last_frame` / `project_map_points`
below restate it for callers that hold plain arrays.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import KP_DTYPE, QUERY_DTYPE, check, lib, ptr

TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
FRAME_GRID_ROWS, FRAME_GRID_COLS = 48, 64


class FrameView:
    """Flat view of a Frame (include/Frame.h) for the matchers."""

    def __init__(self, keys_un, descriptors, scale_factors, bounds, u_right=None):
        self.keys = np.ascontiguousarray(keys_un, KP_DTYPE)
        self.desc = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        self.u_right = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        self.bounds = tuple(np.float32(b) for b in bounds)  # mnMinX, mnMinY, mnMaxX, mnMaxY
        # src/Frame.cc:101-102
        self.grid_inv_w = np.float32(FRAME_GRID_COLS) / (self.bounds[2] - self.bounds[0])
        self.grid_inv_h = np.float32(FRAME_GRID_ROWS) / (self.bounds[3] - self.bounds[1])
        self.N = len(self.keys)

    def c_view(self):
        v = capi.FrameView()
        v.n = self.N
        v.keys, v.desc, v.u_right = ptr(self.keys), ptr(self.desc), ptr(self.u_right)
        v.min_x, v.min_y, v.max_x, v.max_y = self.bounds
        v.grid_inv_w, v.grid_inv_h = self.grid_inv_w, self.grid_inv_h
        v.n_levels = len(self.scale_factors)
        v.scale_factors = ptr(self.scale_factors)
        return v


class ORBmatcher:
    TH_HIGH, TH_LOW, HISTO_LENGTH = TH_HIGH, TH_LOW, HISTO_LENGTH

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self._lib = lib()
        h = C.c_void_p()
        check(self._lib.orbhip_matcher_create(device, C.byref(h)), "orbhip_matcher_create")
        self._h = h
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.orbhip_matcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- DescriptorDistance (src/ORBmatcher.cc:1647-1663), batched ------------
    def DescriptorDistance(self, a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros((len(a), len(b)), np.int32)
        check(self._lib.orbhip_descriptor_distance(self._h, ptr(a), len(a), ptr(b), len(b), ptr(out)),
              "orbhip_descriptor_distance")
        return out

    # -- SearchForInitialization (src/ORBmatcher.cc:405-520) -------------------
    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10):
        """Returns (nmatches, vnMatches12, updated vbPrevMatched)."""
        pm = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2).copy()
        m12 = np.full(max(F1.N, 1), -1, np.int32)
        n = C.c_int()
        v1, v2 = F1.c_view(), F2.c_view()
        check(self._lib.orbhip_search_for_initialization(self._h, C.byref(v1), C.byref(v2), ptr(pm), ptr(m12),
                                                         int(windowSize), self.mfNNratio,
                                                         int(self.mbCheckOrientation), C.byref(n)),
              "orbhip_search_for_initialization")
        return n.value, m12[:F1.N].copy(), pm

    # -- SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1328-1470) ---
    def SearchByProjectionFrame(self, CurrentFrame, queries, query_desc, taken=None):
        """queries: QUERY_DTYPE[nq] (already projected).  Returns (nmatches, assign[N])."""
        q = np.ascontiguousarray(queries, QUERY_DTYPE)
        qd = np.ascontiguousarray(query_desc, np.uint8).reshape(-1, 32)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        out = np.full(max(CurrentFrame.N, 1), -1, np.int32)
        n = C.c_int()
        v = CurrentFrame.c_view()
        check(self._lib.orbhip_search_by_projection_frame(self._h, C.byref(v), ptr(q), ptr(qd), len(q), ptr(tk),
                                                          ptr(out), int(self.mbCheckOrientation), C.byref(n)),
              "orbhip_search_by_projection_frame")
        return n.value, out[:CurrentFrame.N].copy()

    # -- SearchByProjection(F, vpMapPoints, th) (:45-129) ----------------------
    def SearchByProjectionPoints(self, F, queries, query_desc, taken=None):
        q = np.ascontiguousarray(queries, QUERY_DTYPE)
        qd = np.ascontiguousarray(query_desc, np.uint8).reshape(-1, 32)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        out = np.full(max(F.N, 1), -1, np.int32)
        n = C.c_int()
        v = F.c_view()
        check(self._lib.orbhip_search_by_projection_points(self._h, C.byref(v), ptr(q), ptr(qd), len(q), ptr(tk),
                                                           ptr(out), self.mfNNratio, C.byref(n)),
              "orbhip_search_by_projection_points")
        return n.value, out[:F.N].copy()

    # -- SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1472-1599) ---
    def SearchByProjectionKeyFrame(self, CurrentFrame, queries, query_desc, taken=None, ORBdist=100):
        q = np.ascontiguousarray(queries, QUERY_DTYPE)
        qd = np.ascontiguousarray(query_desc, np.uint8).reshape(-1, 32)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        out = np.full(max(CurrentFrame.N, 1), -1, np.int32)
        n = C.c_int()
        v = CurrentFrame.c_view()
        check(self._lib.orbhip_search_by_projection_keyframe(self._h, C.byref(v), ptr(q), ptr(qd), len(q), ptr(tk),
                                                             ptr(out), int(ORBdist), int(self.mbCheckOrientation),
                                                             C.byref(n)), "orbhip_search_by_projection_keyframe")
        return n.value, out[:CurrentFrame.N].copy()

    # -- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:290-403) -------
    def SearchByProjectionSim3(self, KF, queries, query_desc, matched=None):
        q = np.ascontiguousarray(queries, QUERY_DTYPE)
        qd = np.ascontiguousarray(query_desc, np.uint8).reshape(-1, 32)
        tk = None if matched is None else np.ascontiguousarray(matched, np.uint8)
        out = np.full(max(KF.N, 1), -1, np.int32)
        n = C.c_int()
        v = KF.c_view()
        check(self._lib.orbhip_search_by_projection_sim3(self._h, C.byref(v), ptr(q), ptr(qd), len(q), ptr(tk), ptr(out),
                                                         C.byref(n)), "orbhip_search_by_projection_sim3")
        return n.value, out[:KF.N].copy()

    # -- inner search of Fuse x2 (:825-1100) and SearchBySim3 (:1102-1326) -------
    def SearchBestInWindow(self, KF, queries, query_desc, inv_level_sigma2=None):
        """Independent best match per query; chi-square gate enabled when inv_level_sigma2 is given (Fuse).
        Returns (best_idx[nq], best_dist[nq])."""
        q = np.ascontiguousarray(queries, QUERY_DTYPE)
        qd = np.ascontiguousarray(query_desc, np.uint8).reshape(-1, 32)
        bi = np.full(max(len(q), 1), -1, np.int32)
        bd = np.full(max(len(q), 1), 256, np.int32)
        sig = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        v = KF.c_view()
        check(self._lib.orbhip_search_best_in_window(self._h, C.byref(v), ptr(q), ptr(qd), len(q), int(sig is not None),
                                                     ptr(sig), ptr(bi), ptr(bd)), "orbhip_search_best_in_window")
        return bi[:len(q)].copy(), bd[:len(q)].copy()

    # -- vocabulary-guided searches ---------------------------------------------
    def SearchByBoW(self, F1, node1, valid1, F2, node2, blocked2=None, max_dist=50):
        """ORBmatcher::SearchByBoW (src/ORBmatcher.cc:159-288 with max_dist=50; :522-655 with max_dist=49 and
        blocked2 = "pKF2 has no good map point").  node1/node2: vocabulary node id per keypoint (capi.NO_NODE = absent
        from the FeatureVector).  Returns (nmatches, matches12[n1])."""
        v1, v2 = F1.c_view(), F2.c_view()
        n1a = np.ascontiguousarray(node1, np.uint32)
        n2a = np.ascontiguousarray(node2, np.uint32)
        if len(n1a) != F1.N or len(n2a) != F2.N:
            raise ValueError("node id arrays must have one entry per keypoint")
        va = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
        bl = None if blocked2 is None else np.ascontiguousarray(blocked2, np.uint8)
        m12 = np.full(max(F1.N, 1), -1, np.int32)
        nm = C.c_int(0)
        check(self._lib.orbhip_search_by_bow(self._h, C.byref(v1), ptr(n1a), ptr(va), C.byref(v2), ptr(n2a), ptr(bl),
                                             int(max_dist), self.mfNNratio, int(self.mbCheckOrientation), ptr(m12),
                                             C.byref(nm)), "orbhip_search_by_bow")
        return nm.value, m12[:F1.N].copy()

    def SearchByBoWDevice(self, pairs, cap, side1, f1_first, f1_step, side2, f2_first, f2_step, d_matches12, d_nmatches,
                          max_dist=50, d_valid1=0, d_blocked2=0):
        """Device-resident, batched SearchByBoW.  side1 / side2 = (d_kps, d_desc, d_n, d_node) device pointers (ints)
        in the extractor / vocabulary batch layout; asynchronous on the matcher's stream."""
        check(self._lib.orbhip_search_by_bow_device(self._h, pairs, cap, side1[0], side1[1], side1[2], side1[3], d_valid1,
                                                    f1_first, f1_step, side2[0], side2[1], side2[2], side2[3], d_blocked2,
                                                    f2_first, f2_step, int(max_dist), self.mfNNratio,
                                                    int(self.mbCheckOrientation), d_matches12, d_nmatches),
              "orbhip_search_by_bow_device")

    def SearchForTriangulation(self, F1, node1, valid1, F2, node2, valid2, F12, epipole, level_sigma2, bOnlyStereo=False):
        """ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823).  Returns (nmatches, matches12[n1]); the
        reference's vMatchedPairs are the (i, matches12[i]) with matches12[i] >= 0."""
        v1, v2 = F1.c_view(), F2.c_view()
        n1a = np.ascontiguousarray(node1, np.uint32)
        n2a = np.ascontiguousarray(node2, np.uint32)
        if len(n1a) != F1.N or len(n2a) != F2.N:
            raise ValueError("node id arrays must have one entry per keypoint")
        va = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
        vb = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sg = np.ascontiguousarray(level_sigma2, np.float32)
        m12 = np.full(max(F1.N, 1), -1, np.int32)
        nm = C.c_int(0)
        check(self._lib.orbhip_search_for_triangulation(self._h, C.byref(v1), ptr(n1a), ptr(va), C.byref(v2), ptr(n2a),
                                                        ptr(vb), ptr(F), float(epipole[0]), float(epipole[1]), ptr(sg),
                                                        int(bOnlyStereo), int(self.mbCheckOrientation), ptr(m12),
                                                        C.byref(nm)), "orbhip_search_for_triangulation")
        return nm.value, m12[:F1.N].copy()

    def ComputeDistinctiveDescriptors(self, descriptor_lists):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) for a batch of map points.
        descriptor_lists: sequence of (N_p x 32) uint8 arrays; returns best index per map point (-1 if empty)."""
        lens = [len(np.asarray(d).reshape(-1, 32)) for d in descriptor_lists]
        off = np.zeros(len(lens) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        flat = (np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in descriptor_lists])
                if off[-1] > 0 else np.zeros((1, 32), np.uint8))
        flat = np.ascontiguousarray(flat, np.uint8)
        best = np.full(max(len(lens), 1), -1, np.int32)
        check(self._lib.orbhip_distinctive_descriptors(self._h, ptr(flat), ptr(off), len(lens), ptr(best)),
              "orbhip_distinctive_descriptors")
        return best[:len(lens)].copy()

    # -- Frame constructor glue --------------------------------------------------
    def UndistortKeyPoints(self, keys, fx, fy, cx, cy, dist):
        """Frame::UndistortKeyPoints (src/Frame.cc:404-434); dist = (k1, k2, p1, p2[, k3]).  Returns mvKeysUn."""
        k = np.ascontiguousarray(keys, KP_DTYPE)
        d = np.zeros(5, np.float32)
        d[:len(dist)] = dist
        out = np.zeros(max(len(k), 1), KP_DTYPE)
        check(self._lib.orbhip_undistort_keypoints(self._h, ptr(k), len(k), fx, fy, cx, cy, ptr(d), ptr(out)),
              "orbhip_undistort_keypoints")
        return out[:len(k)].copy()

    def AssignFeaturesToGrid(self, F):
        """Frame::AssignFeaturesToGrid (src/Frame.cc:230-245).  Returns (cell_of[n], cell_start[3073], cell_items[m]):
        mGrid[x][y] = cell_items[cell_start[x*48+y] : cell_start[x*48+y+1]]."""
        v = F.c_view()
        cell_of = np.full(max(F.N, 1), -1, np.int32)
        start = np.zeros(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1, np.int32)
        items = np.zeros(max(F.N, 1), np.int32)
        check(self._lib.orbhip_assign_features_to_grid(self._h, C.byref(v), ptr(cell_of), ptr(start), ptr(items)),
              "orbhip_assign_features_to_grid")
        return cell_of[:F.N].copy(), start, items[:start[-1]].copy()

    def AssignFeaturesToGridDevice(self, frames, d_kps_un, d_n, cap, bounds, d_cell_of, d_cell_start, d_cell_items):
        """Batched, device-resident form (device pointers as ints): d_cell_of / d_cell_items [frames][cap] int32,
        d_cell_start [frames][3073] int32.  Asynchronous on the matcher's stream."""
        b = [np.float32(v) for v in bounds]
        check(self._lib.orbhip_assign_features_to_grid_device(
            self._h, frames, d_kps_un, d_n, cap, b[0], b[1], np.float32(FRAME_GRID_COLS) / (b[2] - b[0]),
            np.float32(FRAME_GRID_ROWS) / (b[3] - b[1]), d_cell_of, d_cell_start, d_cell_items),
            "orbhip_assign_features_to_grid_device")

    def ComputeStereoFromRGBD(self, keys, keys_un, imDepth, mbf):
        """Frame::ComputeStereoFromRGBD (src/Frame.cc:643-664); imDepth: 2-D float32.  Returns (mvuRight, mvDepth)."""
        k = np.ascontiguousarray(keys, KP_DTYPE)
        ku = k if keys_un is None else np.ascontiguousarray(keys_un, KP_DTYPE)
        d = np.ascontiguousarray(imDepth, np.float32)
        ur = np.full(max(len(k), 1), -1, np.float32)
        dp = np.full(max(len(k), 1), -1, np.float32)
        check(self._lib.orbhip_compute_stereo_from_rgbd(self._h, ptr(k), ptr(ku), len(k), ptr(d), d.shape[0], d.shape[1],
                                                        d.shape[1], float(mbf), ptr(ur), ptr(dp)),
              "orbhip_compute_stereo_from_rgbd")
        return ur[:len(k)].copy(), dp[:len(k)].copy()

    def ComputeStereoFromRGBDRaw(self, keys, keys_un, imDepth, depth_factor, mbf):
        """Frame::ComputeStereoFromRGBD on the depth image as the sensor delivers it: imDepth 2-D uint16 or float32,
        depth_factor = mDepthMapFactor (settings.depth_map_factor).  The convertTo of src/Tracking.cc:227-228 is applied to
        the sampled values only.  Returns (mvuRight, mvDepth)."""
        k = np.ascontiguousarray(keys, KP_DTYPE)
        ku = k if keys_un is None else np.ascontiguousarray(keys_un, KP_DTYPE)
        d = np.asarray(imDepth)
        if d.ndim != 2 or d.dtype not in (np.uint16, np.float32):
            raise TypeError("expected a CV_16U or CV_32F depth image")
        d = np.ascontiguousarray(d)
        typ = capi.DEPTH_U16 if d.dtype == np.uint16 else capi.DEPTH_F32
        ur = np.full(max(len(k), 1), -1, np.float32)
        dp = np.full(max(len(k), 1), -1, np.float32)
        check(self._lib.orbhip_compute_stereo_from_rgbd_raw(self._h, ptr(k), ptr(ku), len(k), ptr(d), typ, d.shape[0],
                                                            d.shape[1], d.shape[1], float(np.float32(depth_factor)),
                                                            float(mbf), ptr(ur), ptr(dp)),
              "orbhip_compute_stereo_from_rgbd_raw")
        return ur[:len(k)].copy(), dp[:len(k)].copy()

    def compute_stereo_from_rgbd_raw_device(self, frames, d_kps, d_kps_un, d_n, cap, d_depth, depth_type, rows, cols,
                                            depth_factor, mbf, d_u_right, d_depth_out, stride=None, frame_stride=None):
        """Batched, device-resident form (device pointers as ints); strides in elements.  Asynchronous."""
        stride = cols if stride is None else stride
        frame_stride = rows * stride if frame_stride is None else frame_stride
        check(self._lib.orbhip_compute_stereo_from_rgbd_raw_device(self._h, frames, d_kps, d_kps_un, d_n, cap, d_depth,
                                                                   depth_type, rows, cols, stride, frame_stride,
                                                                   float(np.float32(depth_factor)), float(mbf), d_u_right,
                                                                   d_depth_out),
              "orbhip_compute_stereo_from_rgbd_raw_device")

    # -- seeding stereo / RGB-D map points (src/Tracking.cc:523-538, 812-864, 1073-1133; src/Frame.cc:666-680) --------
    def SeedStereoPoints(self, cam, Tcw, keys_un, depth, th_depth, mode, created_flags, world, flags):
        """The depth-sorted map-point creation of Tracking::UpdateLastFrame / CreateNewKeyFrame (mode capi.SEED_CLOSEST)
        or the one of StereoInitialization (capi.SEED_ALL) with Frame::UnprojectStereo.  flags [n] uint8: POINT_PRESENT =
        the slot has a map point, POINT_OBSERVED = it has observations; world [n,3] = their positions.  Returns
        (world, flags, order, created, (n_valid, n_visited, n_created)): copies of world / flags with the created entries
        filled in, the visited keypoint indices in visiting order, and a 0 / 1 mark per keypoint."""
        Tc = np.ascontiguousarray(np.asarray(Tcw, np.float32)[:3, :4])
        k = np.ascontiguousarray(keys_un, KP_DTYPE)
        n = len(k)
        z = np.ascontiguousarray(depth, np.float32)
        w = np.array(world, np.float32, order="C").reshape(-1, 3)
        fg = np.array(flags, np.uint8, order="C")
        if len(z) != n or len(w) != n or len(fg) != n:
            raise ValueError("depth, world and flags must have one entry per keypoint")
        order = np.full(max(n, 1), -1, np.int32)
        created = np.zeros(max(n, 1), np.uint8)
        counts = np.zeros(3, np.int32)
        check(self._lib.orbhip_seed_stereo_points(self._h, C.byref(cam), ptr(Tc), ptr(k), ptr(z), n, float(np.float32(th_depth)),
                                                  int(mode), int(created_flags), ptr(w), ptr(fg), ptr(order), ptr(created),
                                                  ptr(counts)), "orbhip_seed_stereo_points")
        return w, fg, order[:counts[1]].copy(), created[:n].copy(), tuple(int(c) for c in counts)

    def SeedStereoPointsDevice(self, frames, cam, d_Tcw, d_kps, d_n, cap, kp_first, kp_step, d_depth, th_depth, mode,
                               created_flags, d_world, d_flags, d_counts, d_order=0, d_created=0):
        """Batched, device-resident form (device pointers as ints): d_world / d_flags are updated in place, ready for
        TrackLastFrameDevice.  Asynchronous on the matcher's stream."""
        check(self._lib.orbhip_seed_stereo_points_device(self._h, frames, C.byref(cam), d_Tcw, d_kps, d_n, cap, kp_first,
                                                         kp_step, d_depth, float(np.float32(th_depth)), int(mode),
                                                         int(created_flags), d_world, d_flags, d_order, d_created, d_counts),
              "orbhip_seed_stereo_points_device")

    def CountClosePoints(self, depth, flags, th_depth):
        """Tracking::NeedNewKeyFrame's (nTrackedClose, nNonTrackedClose) (src/Tracking.cc:1001-1018); here POINT_PRESENT
        means mvpMapPoints[i] && !mvbOutlier[i]."""
        z = np.ascontiguousarray(depth, np.float32)
        fg = np.ascontiguousarray(flags, np.uint8)
        if len(z) != len(fg):
            raise ValueError("depth and flags must have one entry per keypoint")
        a, b = C.c_int(), C.c_int()
        check(self._lib.orbhip_count_close_points(self._h, ptr(z), ptr(fg), len(z), float(np.float32(th_depth)), C.byref(a),
                                                  C.byref(b)), "orbhip_count_close_points")
        return a.value, b.value

    def CountClosePointsDevice(self, frames, d_depth, d_flags, d_n, cap, th_depth, d_counts):
        check(self._lib.orbhip_count_close_points_device(self._h, frames, d_depth, d_flags, d_n, cap,
                                                         float(np.float32(th_depth)), d_counts),
              "orbhip_count_close_points_device")

    # -- refreshing map points (src/MapPoint.cc:242-307, :330-371) ------------------------------------------------------
    def UpdateMapPoints(self, cam, what, KFs, Tcw, kf_bad, obs_start, obs_kf, obs_idx, ref_obs, world, flags, point_desc,
                        normal, max_dist, min_dist):
        """MapPoint::ComputeDistinctiveDescriptors (what & capi.UPDATE_DESCRIPTOR) and MapPoint::UpdateNormalAndDepth
        (what & capi.UPDATE_NORMAL_DEPTH) for the np = len(obs_start) - 1 map points of an observation table in CSR form:
        observation j of point p is key point obs_idx[o] of KFs[obs_kf[o]], o = obs_start[p] + j, and ref_obs[p] is the
        position of mpRefKF's observation in the point's list.  KFs: K FrameViews, Tcw [K] poses (4x4 or 3x4), kf_bad [K]
        (None: no key frame is bad); flags [np]: POINT_PRESENT = !mbBad; world [np, 3].  One staged copy, one device call,
        one read-back.  Returns (point_desc, normal, max_dist, min_dist, best_obs, status): updated copies of the four
        arrays (an entry the reference would not write keeps the value passed in), the position of the chosen descriptor
        in each list (-1: none) and one capi.MAPPOINT_* code per point."""
        K = len(KFs)
        start = np.ascontiguousarray(obs_start, np.int32)
        n = len(start) - 1
        if n < 0:
            raise ValueError("obs_start needs np + 1 entries")
        okf, oidx = np.ascontiguousarray(obs_kf, np.int32), np.ascontiguousarray(obs_idx, np.int32)
        if len(okf) != len(oidx) or (n > 0 and len(okf) < start[-1]):
            raise ValueError("obs_kf and obs_idx must hold obs_start[-1] entries")
        Tc = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(K, -1, 4)[:, :3, :]).reshape(K, 12)
        bad = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.uint8)
        ref = np.ascontiguousarray(ref_obs, np.int32)
        w = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
        fg = np.ascontiguousarray(flags, np.uint8)
        pd = np.array(point_desc, np.uint8, order="C").reshape(-1, 32)
        nn = np.array(normal, np.float32, order="C").reshape(-1, 3)
        mx, mn = np.array(max_dist, np.float32, order="C"), np.array(min_dist, np.float32, order="C")
        if (bad is not None and len(bad) != K) or any(len(a) < n for a in (ref, w, fg, pd, nn, mx, mn)):
            raise ValueError("every per-point array needs one entry per map point, kf_bad one per key frame")
        best, status = np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.uint8)
        views = [kf.c_view() for kf in KFs]
        arr = (C.POINTER(capi.FrameView) * max(K, 1))(*[C.pointer(v) for v in views])
        check(self._lib.orbhip_update_map_points(self._h, C.byref(cam), int(what), K, arr, ptr(Tc), ptr(bad), n, ptr(start),
                                                 ptr(okf), ptr(oidx), ptr(ref), ptr(w), ptr(fg), ptr(pd), ptr(nn), ptr(mx),
                                                 ptr(mn), ptr(best), ptr(status)), "orbhip_update_map_points")
        return pd, nn, mx, mn, best[:n].copy(), status[:n].copy()

    def UpdateMapPointsDevice(self, cam, what, d_Tcw, d_kps, d_desc, d_n, cap, np_, pcap, d_obs_start, d_obs_kf, d_obs_idx,
                              d_ref_obs, d_world, d_flags, d_point_desc, d_normal, d_max_dist, d_min_dist, d_status,
                              d_best_obs=0, d_kf_bad=0):
        """Device-resident form (device pointers as ints; see orbhip_update_map_points_device in include/orbhip.h): the
        table indexes the rows of the extractor-layout bank, and the four arrays are the ones FuseDevice,
        FrustumQueriesDevice and KeyFrameQueries read.  Asynchronous on the matcher's stream."""
        check(self._lib.orbhip_update_map_points_device(self._h, C.byref(cam), int(what), d_Tcw, d_kps, d_desc, d_n, int(cap),
                                                        d_kf_bad, int(np_), int(pcap), d_obs_start, d_obs_kf, d_obs_idx,
                                                        d_ref_obs, d_world, d_flags, d_point_desc, d_normal, d_max_dist,
                                                        d_min_dist, d_best_obs, d_status),
              "orbhip_update_map_points_device")

    # -- local map (src/Tracking.cc:1146-1180, :1205-1339) ---------------------------------------------------------------
    LOCAL_MAP_TABLES = tuple(k for k, _ in capi.LocalMapTables._fields_)
    LOCAL_MAP_IO = tuple(k for k, _ in capi.LocalMapIO._fields_)
    LOCAL_MAP_TRACK = tuple(k for k, _ in capi.LocalMapTrack._fields_)

    @staticmethod
    def _record(cls, values, optional=()):
        """A ctypes record from a dict of addresses (ints, or objects with data_ptr()); keys in `optional` may be absent."""
        rec = cls()
        for k, _ in cls._fields_:
            v = values.get(k)
            if v is None:
                if k not in optional:
                    raise ValueError("%s: %r is missing" % (cls.__name__, k))
                continue
            setattr(rec, k, v.data_ptr() if hasattr(v, "data_ptr") else int(v))
        return rec

    def UpdateLocalMap(self, tables, frame_point, frame_n, local_kf, n_local_kf, fill=0):
        """Tracking::UpdateLocalKeyFrames, UpdateLocalPoints and the bookkeeping in front of SearchLocalPoints' search for the
        frames of frame_point [frames, cap], from host arrays: `tables` is a dict with the keys of LOCAL_MAP_TABLES
        (slot_point [rows, cap], n [rows], kf_bad [rows] or None, covis [rows, 10], child_start [rows+1], child, parent
        [rows], obs_start [np+1], obs_kf, flags [pcap], world / normal [pcap, 3], max_dist / min_dist [pcap], point_desc
        [pcap, 32]); local_kf [frames, rows] / n_local_kf [frames] are the previous lists.  One staged copy, one device
        call, one read-back; range-checked (OrbHipError with E_ARG).  Returns a dict with the keys of LOCAL_MAP_IO: updated
        copies of frame_point, local_kf and n_local_kf, and the outputs, whose entries past the counts hold `fill`."""
        i32, f32, u8 = np.int32, np.float32, np.uint8
        fp = np.array(frame_point, i32, order="C", ndmin=2)
        frames, cap = fp.shape
        T = {k: tables.get(k) for k in self.LOCAL_MAP_TABLES}
        for k, dt in (("slot_point", i32), ("n", i32), ("covis", i32), ("child_start", i32), ("child", i32), ("parent", i32),
                      ("obs_start", i32), ("obs_kf", i32), ("flags", u8), ("world", f32), ("normal", f32), ("max_dist", f32),
                      ("min_dist", f32), ("point_desc", u8)):
            if T[k] is None:
                raise ValueError("tables[%r] is missing" % k)
            T[k] = np.ascontiguousarray(T[k], dt)
        T["kf_bad"] = None if T["kf_bad"] is None else np.ascontiguousarray(T["kf_bad"], u8)
        rows, pcap, n_pts = len(T["n"]), len(T["flags"]), len(T["obs_start"]) - 1
        if (T["slot_point"].size != rows * cap or T["covis"].size != rows * 10 or len(T["child_start"]) != rows + 1 or
                len(T["parent"]) != rows or n_pts < 0 or n_pts > pcap or (T["kf_bad"] is not None and len(T["kf_bad"]) != rows) or
                T["world"].size != 3 * pcap or T["normal"].size != 3 * pcap or len(T["max_dist"]) != pcap or
                len(T["min_dist"]) != pcap or T["point_desc"].size != 32 * pcap or
                len(T["child"]) < max(int(T["child_start"][-1]), 0) or len(T["obs_kf"]) < max(int(T["obs_start"][-1]), 0)):
            raise ValueError("the local-map tables do not agree on rows, cap or pcap")
        for k in ("child", "obs_kf"):        # a required pointer even when the list is empty
            if T[k].size == 0:
                T[k] = np.zeros(1, i32)
        io = dict(frame_point=fp, frame_n=np.ascontiguousarray(frame_n, i32),
                  local_kf=np.array(local_kf, i32, order="C").reshape(frames, rows), n_local_kf=np.array(n_local_kf, i32, order="C"),
                  votes=np.full((frames, rows), fill, i32), local_point=np.full((frames, pcap), fill, i32),
                  world_l=np.full((frames, pcap, 3), fill, f32), normal_l=np.full((frames, pcap, 3), fill, f32),
                  max_dist_l=np.full((frames, pcap), fill, f32), min_dist_l=np.full((frames, pcap), fill, f32),
                  desc_l=np.full((frames, pcap, 32), fill, u8), flags_l=np.full((frames, pcap), fill, u8),
                  np_l=np.full(frames, fill, i32), taken=np.full((frames, cap), fill, u8), report=np.full((frames, 8), fill, i32))
        if len(io["frame_n"]) != frames or len(io["n_local_kf"]) != frames:
            raise ValueError("frame_n and n_local_kf need one entry per frame")
        keep = [np.zeros(1, u8) if a.size == 0 else a for a in io.values()]      # never pass a null required pointer
        rt = self._record(capi.LocalMapTables, {k: (None if v is None else ptr(v).value) for k, v in T.items()}, ("kf_bad",))
        rio = self._record(capi.LocalMapIO, {k: ptr(a).value for k, a in zip(io, keep)})
        check(self._lib.orbhip_update_local_map(self._h, frames, rows, cap, n_pts, pcap, C.byref(rt), C.byref(rio)),
              "orbhip_update_local_map")
        return io

    def UpdateLocalMapDevice(self, frames, rows, cap, np_, pcap, tables, io):
        """Device-resident form (orbhip_update_local_map_device in include/orbhip.h): `tables` and `io` are dicts with the
        keys of LOCAL_MAP_TABLES / LOCAL_MAP_IO holding device addresses (ints, or tensors); kf_bad may be absent.
        Asynchronous on the matcher's stream."""
        rt = self._record(capi.LocalMapTables, tables, ("kf_bad",))
        rio = self._record(capi.LocalMapIO, io)
        check(self._lib.orbhip_update_local_map_device(self._h, int(frames), int(rows), int(cap), int(np_), int(pcap), C.byref(rt),
                                                       C.byref(rio)), "orbhip_update_local_map_device")

    def TrackLocalMapDevice(self, frames, rows, cap, np_, pcap, tables, io, cam, track, viewing_cos_limit, th, nnratio):
        """UpdateLocalMapDevice, then the frustum prologue and the points search on the same stream
        (orbhip_track_local_map_device): `track` holds Tcw, kps, desc, u_right (may be absent), q, assign, nmatches."""
        rt = self._record(capi.LocalMapTables, tables, ("kf_bad",))
        rio = self._record(capi.LocalMapIO, io)
        rtr = self._record(capi.LocalMapTrack, track, ("u_right",))
        check(self._lib.orbhip_track_local_map_device(self._h, int(frames), int(rows), int(cap), int(np_), int(pcap), C.byref(rt),
                                                      C.byref(rio), C.byref(cam), C.byref(rtr),
                                                      float(np.float32(viewing_cos_limit)), float(np.float32(th)),
                                                      float(np.float32(nnratio))), "orbhip_track_local_map_device")

    # -- covisibility graph (src/KeyFrame.cc:123-182, :289-379; src/LocalMapping.cc:457-479) -----------------------------
    COVIS_TABLES = tuple(k for k, _ in capi.CovisTables._fields_)
    COVIS_STATE = tuple(k for k, _ in capi.CovisState._fields_)

    def UpdateConnections(self, tables, state, update_rows, id0_row=-1):
        """KeyFrame::UpdateConnections for the bank rows of update_rows, in list order, from host arrays: `tables` is a
        dict with the keys of COVIS_TABLES (slot_point [rows, cap], n [rows], obs_start [np+1], obs_kf, flags [pcap]),
        `state` a dict with the keys of COVIS_STATE (conn_w / ord_kf / ord_w [rows, rows], n_ord [rows], covis [rows, 10],
        first_conn [rows] uint8, parent [rows]).  One staged copy of the rows the call can reach, one device call, one
        read-back; range-checked (OrbHipError with E_ARG).  Returns (state, report): updated copies of the seven arrays
        (rows the call does not reach, and list entries past n_ord, as passed in) and report [U, 8] int32 in the order of
        capi.CONNECTIONS_REPORT."""
        i32, u8 = np.int32, np.uint8
        T = {}
        for k, dt in (("slot_point", i32), ("n", i32), ("obs_start", i32), ("obs_kf", i32), ("flags", u8)):
            if tables.get(k) is None:
                raise ValueError("tables[%r] is missing" % k)
            T[k] = np.ascontiguousarray(tables[k], dt)
        rows, pcap, n_pts = len(T["n"]), len(T["flags"]), len(T["obs_start"]) - 1
        if T["slot_point"].ndim != 2 or T["slot_point"].shape[0] != rows or n_pts < 0 or n_pts > pcap or \
                len(T["obs_kf"]) < max(int(T["obs_start"][-1]), 0):
            raise ValueError("the covisibility tables do not agree on rows or pcap")
        cap = T["slot_point"].shape[1]
        S = {}
        for k, dt, shape in (("conn_w", i32, (rows, rows)), ("ord_kf", i32, (rows, rows)), ("ord_w", i32, (rows, rows)),
                             ("n_ord", i32, (rows,)), ("covis", i32, (rows, 10)), ("first_conn", u8, (rows,)),
                             ("parent", i32, (rows,))):
            if state.get(k) is None:
                raise ValueError("state[%r] is missing" % k)
            S[k] = np.array(state[k], dt, order="C").reshape(shape)
        upd = np.ascontiguousarray(update_rows, i32).reshape(-1)
        U = len(upd)
        report = np.zeros((U, 8), i32)
        keep = {k: (np.zeros(1, a.dtype) if a.size == 0 else a) for k, a in list(T.items()) + list(S.items())}
        rt = self._record(capi.CovisTables, {k: ptr(keep[k]).value for k in self.COVIS_TABLES})
        rs = self._record(capi.CovisState, {k: ptr(keep[k]).value for k in self.COVIS_STATE})
        pad = [np.zeros(1, i32) if a.size == 0 else a for a in (upd, report)]      # never pass a null required pointer
        check(self._lib.orbhip_update_connections(self._h, rows, cap, n_pts, pcap, C.byref(rt), C.byref(rs), int(id0_row), U,
                                                  ptr(pad[0]), ptr(pad[1])), "orbhip_update_connections")
        return S, report

    def UpdateConnectionsDevice(self, rows, cap, np_, pcap, tables, state, id0_row, U, d_update_rows, d_report):
        """Device-resident form (orbhip_update_connections_device in include/orbhip.h): `tables` and `state` are dicts with
        the keys of COVIS_TABLES / COVIS_STATE holding device addresses (ints, or tensors).  Asynchronous on the matcher's
        stream."""
        rt = self._record(capi.CovisTables, tables)
        rs = self._record(capi.CovisState, state)
        check(self._lib.orbhip_update_connections_device(self._h, int(rows), int(cap), int(np_), int(pcap), C.byref(rt),
                                                         C.byref(rs), int(id0_row), int(U), d_update_rows, d_report),
              "orbhip_update_connections_device")

    def CovisibleTargets(self, ord_kf, n_ord, cur, nn, nn2=0, kf_bad=None):
        """GetBestCovisibilityKeyFrames(nn) of each row of `cur` (nn2 == 0: the neighbours of CreateNewMapPoints) or the
        target list of SearchInNeighbors (nn2 > 0) from the host arrays ord_kf [rows, rows] / n_ord [rows] / kf_bad [rows].
        Returns a list of int32 arrays, one per current row."""
        i32 = np.int32
        no = np.ascontiguousarray(n_ord, i32)
        rows = len(no)
        ok = np.ascontiguousarray(ord_kf, i32).reshape(rows, rows)
        bad = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.uint8)
        if bad is not None and len(bad) != rows:
            raise ValueError("kf_bad needs one entry per bank row")
        c = np.ascontiguousarray(cur, i32).reshape(-1)
        Q, width = len(c), max(int(nn), 0) * (1 + max(int(nn2), 0))
        targets, counts = np.full((max(Q, 1), max(width, 1)), -1, i32), np.zeros(max(Q, 1), i32)
        pad = [np.zeros(1, i32) if a.size == 0 else a for a in (ok, no, c)]
        check(self._lib.orbhip_covisible_targets(self._h, rows, ptr(pad[0]), ptr(pad[1]), ptr(bad), Q, ptr(pad[2]), int(nn),
                                                 int(nn2), ptr(targets), ptr(counts)), "orbhip_covisible_targets")
        return [targets[q, :counts[q]].copy() for q in range(Q)]

    def CovisibleTargetsDevice(self, rows, d_ord_kf, d_n_ord, d_kf_bad, Q, d_cur, nn, nn2, d_targets, d_counts):
        """Device-resident form (orbhip_covisible_targets_device): d_targets [Q, nn * (1 + nn2)] int32, -1 behind the
        count, and d_counts [Q].  K of the following CreateNewMapPointsDevice / FuseDevice call is a host integer, so the
        caller reads d_counts.  Asynchronous on the matcher's stream."""
        check(self._lib.orbhip_covisible_targets_device(self._h, int(rows), d_ord_kf, d_n_ord, d_kf_bad, int(Q), d_cur, int(nn),
                                                        int(nn2), d_targets, d_counts), "orbhip_covisible_targets_device")

    def ChildrenFromParentsDevice(self, rows, d_parent, d_kf_bad, d_child_start, d_child):
        """d_child_start [rows + 1] / d_child [rows] from d_parent [rows] and d_kf_bad [rows] (0: no row is bad)
        (orbhip_children_from_parents_device).  Asynchronous on the matcher's stream."""
        check(self._lib.orbhip_children_from_parents_device(self._h, int(rows), d_parent, d_kf_bad, d_child_start, d_child),
              "orbhip_children_from_parents_device")

    # -- culling (src/LocalMapping.cc:170-205, :632-696; src/KeyFrame.cc:453-567; src/MapPoint.cc:111-168) ----------------
    CULL_TABLES = tuple(k for k, _ in capi.CullTables._fields_)
    CULL_IO = tuple(k for k, _ in capi.CullIO._fields_)
    _CULL_DTYPES = dict(kps=capi.KP_DTYPE, u_right=np.float32, depth=np.float32, n=np.int32, obs_start=np.int32, obs_kf=np.int32,
                        obs_idx=np.int32, ref_obs=np.int32, not_erase=np.uint8, slot_point=np.int32, flags=np.uint8,
                        kf_bad=np.uint8, to_be_erased=np.uint8, child_start=np.int32, child=np.int32)

    def _cull_host(self, tables, io, key_frames, fill):
        """The records of the host culling entries from dicts of host arrays, with fresh in/out copies and the table out."""
        T = {k: (None if tables.get(k) is None else np.ascontiguousarray(tables[k], self._CULL_DTYPES[k])) for k in self.CULL_TABLES}
        for k in ("obs_start", "obs_kf", "obs_idx", "ref_obs") + (("kps", "n") if key_frames else ()):
            if T[k] is None:
                raise ValueError("tables[%r] is missing" % k)
        IO = {}
        need = ("slot_point", "flags") + (("kf_bad", "child_start", "child") if key_frames else ())
        for k in ("slot_point", "flags", "kf_bad", "to_be_erased", "child_start", "child"):
            if io.get(k) is None:
                if k in need:
                    raise ValueError("io[%r] is missing" % k)
                IO[k] = None
            else:
                IO[k] = np.array(io[k], self._CULL_DTYPES[k], order="C")
        if IO["slot_point"].ndim != 2:
            raise ValueError("slot_point is [rows, cap]")
        rows, cap = IO["slot_point"].shape
        n_pts, pcap = len(T["obs_start"]) - 1, len(IO["flags"])
        obs_cap = len(T["obs_kf"])
        if n_pts < 0 or len(T["obs_idx"]) != obs_cap or len(T["ref_obs"]) < n_pts:
            raise ValueError("the observation table does not agree with itself")
        IO["obs_start_out"] = np.full(n_pts + 1, fill, np.int32)
        IO["obs_kf_out"] = np.full(max(obs_cap, 1), fill, np.int32)
        IO["obs_idx_out"] = np.full(max(obs_cap, 1), fill, np.int32)
        IO["ref_obs_out"] = np.full(max(n_pts, 1), fill, np.int32)
        keep = [np.zeros(1, a.dtype) if a is not None and a.size == 0 else a for a in list(T.values()) + list(IO.values())]
        rt = self._record(capi.CullTables, {k: ptr(a).value for k, a in zip(T, keep) if a is not None},
                          ("kps", "u_right", "depth", "n", "not_erase"))
        rio = self._record(capi.CullIO, {k: ptr(a).value for k, a in zip(IO, keep[len(T):]) if a is not None},
                           ("kf_bad", "to_be_erased", "child_start", "child"))
        return rt, rio, IO, keep, (rows, cap, n_pts, pcap, obs_cap)

    def CullMapPoints(self, tables, io, recent, found, visible, first_kf_id, cur_kf_id, th_obs, fill=0):
        """LocalMapping::MapPointCulling from host arrays (orbhip_cull_map_points): `tables` holds obs_start, obs_kf, obs_idx,
        ref_obs and optionally u_right [rows, cap]; `io` holds slot_point [rows, cap] and flags [pcap].  Returns (io, kept,
        status): copies of slot_point and flags as the call left them plus the table out (obs_start_out, obs_kf_out,
        obs_idx_out, ref_obs_out; entries the call does not write hold `fill`), the kept entries of `recent` in order and one capi.CULLPOINT_* code per entry."""
        i32 = np.int32
        rt, rio, IO, keep, (rows, cap, n_pts, pcap, obs_cap) = self._cull_host(tables, io, False, fill)
        rec = np.ascontiguousarray(recent, i32).reshape(-1)
        R = len(rec)
        per_point = [np.ascontiguousarray(a, i32) for a in (found, visible, first_kf_id)]
        if any(len(a) < n_pts for a in per_point):
            raise ValueError("found, visible and first_kf_id need one entry per point")
        out, n_out, status = np.zeros(max(R, 1), i32), np.zeros(1, i32), np.zeros(max(R, 1), np.uint8)
        pad = [np.zeros(1, i32) if a.size == 0 else a for a in [rec] + per_point]
        check(self._lib.orbhip_cull_map_points(self._h, rows, cap, n_pts, pcap, obs_cap, C.byref(rt), C.byref(rio), R, ptr(pad[0]),
                                               ptr(pad[1]), ptr(pad[2]), ptr(pad[3]), int(cur_kf_id), int(th_obs), ptr(out),
                                               ptr(n_out), ptr(status)), "orbhip_cull_map_points")
        return IO, out[:int(n_out[0])].copy(), status[:R].copy()

    def CullMapPointsDevice(self, rows, cap, np_, pcap, obs_cap, tables, io, R, d_recent, d_found, d_visible, d_first_kf_id,
                            cur_kf_id, th_obs, d_recent_out, d_n_recent_out, d_status):
        """Device-resident form (orbhip_cull_map_points_device in include/orbhip.h): `tables` and `io` are dicts with the keys
        of CULL_TABLES / CULL_IO holding device addresses (ints, or tensors); what the call does not read may be absent.
        Asynchronous on the matcher's stream."""
        rt = self._record(capi.CullTables, tables, ("kps", "u_right", "depth", "n", "not_erase"))
        rio = self._record(capi.CullIO, io, ("kf_bad", "to_be_erased", "child_start", "child"))
        check(self._lib.orbhip_cull_map_points_device(self._h, int(rows), int(cap), int(np_), int(pcap), int(obs_cap), C.byref(rt),
                                                      C.byref(rio), int(R), d_recent, d_found, d_visible, d_first_kf_id,
                                                      int(cur_kf_id), int(th_obs), d_recent_out, d_n_recent_out, d_status),
              "orbhip_cull_map_points_device")

    def CullKeyFrames(self, tables, io, state, cand, id0_row=-1, mono=False, th_depth=0.0, fill=0):
        """LocalMapping::KeyFrameCulling over the candidate rows `cand` (-1 entries are skipped) from host arrays
        (orbhip_cull_key_frames): `tables` with the keys of CULL_TABLES (u_right, depth, not_erase may be absent), `io` with
        slot_point, flags, kf_bad, child_start [rows + 1], child [rows] and optionally to_be_erased, `state` with the keys of
        COVIS_STATE.  Returns (io, state, report): copies as the call left them, the table out among io, and report [U, 8]
        int32 in the order of capi.CULLKF_REPORT."""
        i32, u8 = np.int32, np.uint8
        rt, rio, IO, keep, (rows, cap, n_pts, pcap, obs_cap) = self._cull_host(tables, io, True, fill)
        S = {}
        for k, dt, shape in (("conn_w", i32, (rows, rows)), ("ord_kf", i32, (rows, rows)), ("ord_w", i32, (rows, rows)),
                             ("n_ord", i32, (rows,)), ("covis", i32, (rows, 10)), ("first_conn", u8, (rows,)),
                             ("parent", i32, (rows,))):
            if state.get(k) is None:
                raise ValueError("state[%r] is missing" % k)
            S[k] = np.array(state[k], dt, order="C").reshape(shape)
        skeep = {k: (np.zeros(1, a.dtype) if a.size == 0 else a) for k, a in S.items()}
        rs = self._record(capi.CovisState, {k: ptr(skeep[k]).value for k in self.COVIS_STATE})
        c = np.ascontiguousarray(cand, i32).reshape(-1)
        U = len(c)
        report = np.zeros((max(U, 1), 8), i32)
        check(self._lib.orbhip_cull_key_frames(self._h, rows, cap, n_pts, pcap, obs_cap, C.byref(rt), C.byref(rio), C.byref(rs),
                                               int(id0_row), U, ptr(c if U else np.zeros(1, i32)), int(bool(mono)),
                                               float(np.float32(th_depth)), ptr(report)), "orbhip_cull_key_frames")
        return IO, S, report[:U].copy()

    def CullKeyFramesDevice(self, rows, cap, np_, pcap, obs_cap, tables, io, state, id0_row, U, d_cand, mono, th_depth, d_report):
        """Device-resident form (orbhip_cull_key_frames_device): `tables`, `io` and `state` are dicts with the keys of
        CULL_TABLES / CULL_IO / COVIS_STATE holding device addresses; u_right, depth (with mono), not_erase and to_be_erased
        may be absent, first_conn is not read.  Asynchronous on the matcher's stream."""
        rt = self._record(capi.CullTables, tables, ("u_right", "depth", "not_erase"))
        rio = self._record(capi.CullIO, io, ("to_be_erased",))
        rs = self._record(capi.CovisState, state, ("first_conn",))
        check(self._lib.orbhip_cull_key_frames_device(self._h, int(rows), int(cap), int(np_), int(pcap), int(obs_cap), C.byref(rt),
                                                      C.byref(rio), C.byref(rs), int(id0_row), int(U), d_cand, int(bool(mono)),
                                                      float(np.float32(th_depth)), d_report), "orbhip_cull_key_frames_device")

    # -- Sim3 RANSAC (src/Sim3Solver.cc) ---------------------------------------
    SIM3_TABLES = tuple(k for k, _ in capi.Sim3Tables._fields_)
    SIM3_SOLVERS = tuple(k for k, _ in capi.Sim3Solvers._fields_)
    _SIM3_DTYPES = dict(slot_point=np.int32, obs_start=np.int32, obs_kf=np.int32, obs_idx=np.int32, flags=np.uint8,
                        world=np.float32, Tcw=np.float32, kps=capi.KP_DTYPE, n=np.int32)

    @staticmethod
    def _sigma2(level_sigma2, cam):
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        if len(sig) < cam.n_levels:
            raise ValueError("level_sigma2 needs one entry per pyramid level")
        return sig

    def Sim3SetupDevice(self, C_, cur, d_kf_index, cam, rows, cap, np_, pcap, tables, d_matched12, match_form, level_sigma2,
                        solvers, prob=0.99, min_inliers=20, max_its=300):
        """The Sim3Solver constructor and SetRansacParameters for C_ candidates (orbhip_sim3_setup_device in
        include/orbhip.h): `tables` and `solvers` are dicts with the keys of SIM3_TABLES / SIM3_SOLVERS holding device
        addresses (ints, or tensors).  Asynchronous on the matcher's stream."""
        sig = self._sigma2(level_sigma2, cam)
        rt, rs = self._record(capi.Sim3Tables, tables), self._record(capi.Sim3Solvers, solvers)
        dp = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a  # noqa: E731
        check(self._lib.orbhip_sim3_setup_device(self._h, int(C_), int(cur), dp(d_kf_index), C.byref(cam), int(rows), int(cap),
                                                 int(np_), int(pcap), C.byref(rt), dp(d_matched12), int(match_form), ptr(sig),
                                                 float(prob), int(min_inliers), int(max_its), C.byref(rs)),
              "orbhip_sim3_setup_device")

    def Sim3IterateDevice(self, C_, cap, cam, solvers, d_draws, max_its, n_iterations, min_inliers, fix_scale, d_sim3,
                          d_inliers, d_report):
        """Sim3Solver::iterate for every candidate at once (orbhip_sim3_iterate_device): at most n_iterations more
        iterations each, draws[c][it] serving iteration number it.  Asynchronous on the matcher's stream."""
        rs = self._record(capi.Sim3Solvers, solvers)
        dp = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a  # noqa: E731
        check(self._lib.orbhip_sim3_iterate_device(self._h, int(C_), int(cap), C.byref(cam), C.byref(rs), dp(d_draws),
                                                   int(max_its), int(n_iterations), int(min_inliers), int(bool(fix_scale)),
                                                   dp(d_sim3), dp(d_inliers), dp(d_report)), "orbhip_sim3_iterate_device")

    def _sim3_tables(self, tables):
        T = {}
        for k in self.SIM3_TABLES:
            if tables.get(k) is None:
                raise ValueError("tables[%r] is missing" % k)
            T[k] = np.ascontiguousarray(tables[k], self._SIM3_DTYPES[k])
        if T["slot_point"].ndim != 2:
            raise ValueError("slot_point is [rows, cap]")
        rows, cap = T["slot_point"].shape
        T["Tcw"] = np.ascontiguousarray(T["Tcw"].reshape(rows, -1, 4)[:, :3, :]).reshape(rows, 12)
        return T, rows, cap, len(T["obs_start"]) - 1, len(T["flags"])

    def Sim3Setup(self, tables, cur, kf_index, cam, matched12, match_form, level_sigma2, prob=0.99, min_inliers=20,
                  max_its=300, fill=0):
        """Sim3SetupDevice from host arrays: `tables` is a dict with the keys of SIM3_TABLES (slot_point [rows, cap], n
        [rows], obs_start [np+1], obs_kf, obs_idx, flags [pcap], world [pcap, 3], Tcw [rows, 12 or 4x4], kps [rows, cap]
        KP_DTYPE), matched12 [C, cap].  The arrays are uploaded as torch tensors; the returned solver record keeps them and
        the solver state on the device for Sim3Iterate, and holds host copies of the solver arrays under "host" (entries
        the call does not write hold `fill` bytes)."""
        import torch
        T, rows, cap, n_pts, pcap = self._sim3_tables(tables)
        kf = np.ascontiguousarray(kf_index, np.int32).reshape(-1)
        Cn = len(kf)
        m12 = np.ascontiguousarray(matched12, np.int32).reshape(Cn, cap)
        dev = torch.device("cuda")
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(4, np.uint8)).to(dev)  # noqa: E731
        dT = {k: up(v) for k, v in T.items()}
        shapes = dict(x1=(cap, 3), x2=(cap, 3), p1=(cap, 2), p2=(cap, 2), max_err1=(cap,), max_err2=(cap,), slot1=(cap,),
                      n_corr=(), n1=(), limit=(), state=(2,))
        dS = {k: torch.full((max(Cn, 1) * int(np.prod(shapes[k], dtype=np.int64)) * 4,), fill, dtype=torch.uint8, device=dev)
              for k in self.SIM3_SOLVERS}
        d_kf, d_m12 = up(kf), up(m12)
        torch.cuda.synchronize()
        self.Sim3SetupDevice(Cn, cur, d_kf, cam, rows, cap, n_pts, pcap, dT, d_m12, match_form, level_sigma2, dS, prob,
                             min_inliers, max_its)
        self.sync()
        dts = dict(x1=np.float32, x2=np.float32, p1=np.float32, p2=np.float32, max_err1=np.uint32, max_err2=np.uint32)
        host = {k: dS[k].cpu().numpy().view(dts.get(k, np.int32))[:Cn * int(np.prod(shapes[k], dtype=np.int64))]
                .reshape((Cn,) + shapes[k]).copy() for k in self.SIM3_SOLVERS}
        return dict(C=Cn, cap=cap, cam=cam, tables=dT, solvers=dS, keep=(d_kf, d_m12), host=host, min_inliers=int(min_inliers),
                    max_its=int(max_its))

    def Sim3Iterate(self, solver, draws, n_iterations, fix_scale=False, fill=0):
        """Sim3IterateDevice on the record Sim3Setup returned; draws [C, max_its, 3] int32.  Returns (report [C, 8] int32
        in the order of capi.SIM3_REPORT, sim3 [C, 16] float32, inliers [C, cap] uint8); sim3 rows of candidates that did
        not return, and inliers behind n1, hold `fill` bytes.  The solver's state advances on the device."""
        import torch
        Cn, cap, max_its = solver["C"], solver["cap"], solver["max_its"]
        d = np.ascontiguousarray(draws, np.int32).reshape(Cn, max_its, 3)
        dev = torch.device("cuda")
        d_draws = torch.from_numpy(d.reshape(-1).copy() if d.size else np.zeros(3, np.int32)).to(dev)
        d_sim3 = torch.full((max(Cn, 1) * 64,), fill, dtype=torch.uint8, device=dev)
        d_inl = torch.full((max(Cn, 1) * cap,), fill, dtype=torch.uint8, device=dev)
        d_rep = torch.full((max(Cn, 1) * 32,), fill, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.Sim3IterateDevice(Cn, cap, solver["cam"], solver["solvers"], d_draws, max_its, n_iterations, solver["min_inliers"],
                               fix_scale, d_sim3, d_inl, d_rep)
        self.sync()
        solver["host"]["state"] = solver["solvers"]["state"].cpu().numpy().view(np.int32)[:Cn * 2].reshape(Cn, 2).copy()
        return (d_rep.cpu().numpy().view(np.int32)[:Cn * 8].reshape(Cn, 8).copy(),
                d_sim3.cpu().numpy().view(np.float32)[:Cn * 16].reshape(Cn, 16).copy(),
                d_inl.cpu().numpy()[:Cn * cap].reshape(Cn, cap).copy())

    def Sim3Ransac(self, tables, cur, kf_index, cam, matched12, match_form, level_sigma2, draws, fix_scale=False, prob=0.99,
                   min_inliers=20, max_its=300, n_iterations=None, state=None, fill=0):
        """Setup and iterate from host arrays in one staged copy, one device sequence and one read-back
        (orbhip_sim3_ransac), range-checked (OrbHipError with E_ARG), draws included.  n_iterations None = max_its, i.e.
        Sim3Solver::find; `state` [C, 2] resumes solvers an earlier call left.  Returns dict(report [C, 8], sim3 [C, 16],
        inliers [C, cap], state [C, 2]); what the call does not write holds `fill` bytes."""
        T, rows, cap, n_pts, pcap = self._sim3_tables(tables)
        kf = np.ascontiguousarray(kf_index, np.int32).reshape(-1)
        Cn = len(kf)
        m12 = np.ascontiguousarray(matched12, np.int32).reshape(Cn, cap)
        d = np.ascontiguousarray(draws, np.int32).reshape(Cn, max_its, 3)
        sig = self._sigma2(level_sigma2, cam)
        st = np.zeros((max(Cn, 1), 2), np.int32)
        if state is not None:
            st[:Cn] = np.asarray(state, np.int32).reshape(Cn, 2)
        sim3 = np.full(max(Cn, 1) * 64, fill, np.uint8).view(np.float32).reshape(-1, 16)
        inl = np.full((max(Cn, 1), cap), fill, np.uint8)
        rep = np.full(max(Cn, 1) * 32, fill, np.uint8).view(np.int32).reshape(-1, 8)
        keep = {k: (np.zeros(1, a.dtype) if a.size == 0 else a) for k, a in T.items()}
        rt = self._record(capi.Sim3Tables, {k: ptr(a).value for k, a in keep.items()})
        pad = [np.zeros(3, np.int32) if a.size == 0 else a for a in (kf, m12, d)]
        check(self._lib.orbhip_sim3_ransac(self._h, Cn, int(cur), ptr(pad[0]), C.byref(cam), rows, cap, n_pts, pcap, C.byref(rt),
                                           ptr(pad[1]), int(match_form), ptr(sig), float(prob), int(min_inliers), int(max_its),
                                           int(bool(fix_scale)), ptr(pad[2]), int(max_its if n_iterations is None else n_iterations),
                                           ptr(st), ptr(sim3), ptr(inl), ptr(rep)), "orbhip_sim3_ransac")
        return dict(report=rep[:Cn].copy(), sim3=sim3[:Cn].copy(), inliers=inl[:Cn].copy(), state=st[:Cn].copy())

    # -- PnP RANSAC (src/PnPsolver.cc) -----------------------------------------
    PNP_SOLVERS = tuple(k for k, _ in capi.PnpSolvers._fields_)
    _PNP_SHAPES = dict(p2d=("cap", 2, np.float32), p3d=("cap", 3, np.float32), max_err=("cap", 1, np.float32),
                       kp_index=("cap", 1, np.int32), n_corr=(1, 1, np.int32), min_inliers=(1, 1, np.int32),
                       limit=(1, 1, np.int32), state=(1, 2, np.int32), best_inliers=("cap", 1, np.uint8),
                       best_Tcw=(1, 12, np.float32))

    @staticmethod
    def pnp_params(prob=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991):
        """The arguments of PnPsolver::SetRansacParameters as an orbhip_pnp_params record."""
        return capi.PnpParams(float(prob), int(min_inliers), int(max_its), int(min_set), float(epsilon), float(th2))

    def PnpSetupDevice(self, C_, d_kps, n, cap, d_matches, match_form, d_kf_index, rows, np_, pcap, pmap, cam, level_sigma2,
                       params, solvers):
        """The PnPsolver constructor and SetRansacParameters for C_ candidates (orbhip_pnp_setup_device in
        include/orbhip.h): `pmap` and `solvers` are dicts with the fields of capi.PnpMap / PNP_SOLVERS holding device
        addresses (ints, or tensors).  Asynchronous on the matcher's stream."""
        sig = self._sigma2(level_sigma2, cam)
        rm, rs = self._record(capi.PnpMap, pmap, optional=("slot_point",)), self._record(capi.PnpSolvers, solvers)
        dp = lambda a: 0 if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)  # noqa: E731
        check(self._lib.orbhip_pnp_setup_device(self._h, int(C_), dp(d_kps), int(n), int(cap), dp(d_matches), int(match_form),
                                                dp(d_kf_index), int(rows), int(np_), int(pcap), C.byref(rm), C.byref(cam), ptr(sig),
                                                C.byref(params), C.byref(rs)), "orbhip_pnp_setup_device")

    def PnpIterateDevice(self, C_, n, cap, cam, params, solvers, d_draws, draw_rows, n_iterations, d_Tcw, d_inliers, d_report):
        """PnPsolver::iterate for every candidate at once (orbhip_pnp_iterate_device): iterations mnIterations ...
        max(limit, mnIterations + n_iterations) - 1, draws[c][it] serving iteration number it.  Asynchronous."""
        rs = self._record(capi.PnpSolvers, solvers)
        dp = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a  # noqa: E731
        check(self._lib.orbhip_pnp_iterate_device(self._h, int(C_), int(n), int(cap), C.byref(cam), C.byref(params), C.byref(rs),
                                                  dp(d_draws), int(draw_rows), int(n_iterations), dp(d_Tcw), dp(d_inliers),
                                                  dp(d_report)), "orbhip_pnp_iterate_device")

    @staticmethod
    def _pnp_inputs(kps, matches, kf_index, pmap):
        k = np.ascontiguousarray(kps, KP_DTYPE).reshape(-1)
        m = np.ascontiguousarray(matches, np.int32)
        if m.ndim != 2:
            raise ValueError("matches is [C, cap]")
        Cn, cap = m.shape
        kf = None if kf_index is None else np.ascontiguousarray(kf_index, np.int32).reshape(Cn)
        M = dict(flags=np.ascontiguousarray(pmap["flags"], np.uint8).reshape(-1),
                 world=np.ascontiguousarray(pmap["world"], np.float32).reshape(-1, 3))
        rows = 0
        if pmap.get("slot_point") is not None:
            M["slot_point"] = np.ascontiguousarray(pmap["slot_point"], np.int32)
            if M["slot_point"].ndim != 2 or M["slot_point"].shape[1] != cap:
                raise ValueError("slot_point is [rows, cap]")
            rows = M["slot_point"].shape[0]
        return k, m, kf, M, Cn, cap, rows, int(pmap.get("np", len(M["flags"]))), len(M["flags"])

    def PnpSetup(self, kps, matches, match_form, kf_index, pmap, cam, level_sigma2, params=None, fill=0):
        """PnpSetupDevice from host arrays: kps [n] KP_DTYPE (mvKeysUn), matches [C, cap] int32, kf_index [C] (None with
        point matches), pmap = dict(flags [pcap], world [pcap, 3], slot_point [rows, cap] for slot matches, optional np).
        The arrays are uploaded as torch tensors; the returned record keeps them and the solver record on the device for
        PnpIterate, and holds host copies of the solver arrays under "host" (what the call does not write holds `fill`)."""
        import torch
        params = params or self.pnp_params()
        k, m, kf, M, Cn, cap, rows, n_pts, pcap = self._pnp_inputs(kps, matches, kf_index, pmap)
        dev = torch.device("cuda")
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(4, np.uint8)).to(dev)  # noqa: E731
        dM = {key: up(v) for key, v in M.items()}
        size = lambda key: (cap if self._PNP_SHAPES[key][0] == "cap" else 1) * self._PNP_SHAPES[key][1]  # noqa: E731
        dS = {key: torch.full((max(Cn, 1) * size(key) * np.dtype(self._PNP_SHAPES[key][2]).itemsize,), fill, dtype=torch.uint8,
                              device=dev) for key in self.PNP_SOLVERS}
        d_k, d_m, d_kf = up(k), up(m), (None if kf is None else up(kf))
        torch.cuda.synchronize()
        self.PnpSetupDevice(Cn, d_k, len(k), cap, d_m, match_form, d_kf, rows, n_pts, pcap, dM, cam, level_sigma2, params, dS)
        self.sync()
        rec = dict(C=Cn, n=len(k), cap=cap, cam=cam, params=params, map=dM, solvers=dS, keep=(d_k, d_m, d_kf))
        rec["host"] = self._pnp_host(rec)
        return rec

    def _pnp_host(self, rec):
        Cn, cap, out = rec["C"], rec["cap"], {}
        for key in self.PNP_SOLVERS:
            per, width, dt = self._PNP_SHAPES[key]
            cnt = (cap if per == "cap" else 1) * width
            a = rec["solvers"][key].cpu().numpy().view(dt)[:Cn * cnt]
            out[key] = a.reshape((Cn,) + ((cap,) if per == "cap" else ()) + ((width,) if width > 1 else ())).copy()
        return out

    def PnpIterate(self, solver, draws, n_iterations, fill=0):
        """PnpIterateDevice on the record PnpSetup returned; draws [C, draw_rows, 4] int32.  Returns (report [C, 8] int32 in
        the order of capi.PNP_REPORT, Tcw [C, 12] float32, inliers [C, cap] uint8); what the call does not write holds `fill`
        bytes.  The solver record advances on the device; solver["host"] is refreshed."""
        import torch
        Cn, cap = solver["C"], solver["cap"]
        d = np.ascontiguousarray(draws, np.int32)
        d = d.reshape(Cn, -1, 4)
        dev = torch.device("cuda")
        d_draws = torch.from_numpy(d.reshape(-1).copy() if d.size else np.zeros(4, np.int32)).to(dev)
        d_T = torch.full((max(Cn, 1) * 48,), fill, dtype=torch.uint8, device=dev)
        d_inl = torch.full((max(Cn, 1) * cap,), fill, dtype=torch.uint8, device=dev)
        d_rep = torch.full((max(Cn, 1) * 32,), fill, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.PnpIterateDevice(Cn, solver["n"], cap, solver["cam"], solver["params"], solver["solvers"], d_draws, d.shape[1],
                              n_iterations, d_T, d_inl, d_rep)
        self.sync()
        solver["host"] = self._pnp_host(solver)
        return (d_rep.cpu().numpy().view(np.int32)[:Cn * 8].reshape(Cn, 8).copy(),
                d_T.cpu().numpy().view(np.float32)[:Cn * 12].reshape(Cn, 12).copy(),
                d_inl.cpu().numpy()[:Cn * cap].reshape(Cn, cap).copy())

    def PnpRansac(self, kps, matches, match_form, kf_index, pmap, cam, level_sigma2, draws, params=None, n_iterations=None,
                  state=None, best_inliers=None, best_Tcw=None, fill=0):
        """Setup and iterate from host arrays in one staged copy, one device sequence and one read-back
        (orbhip_pnp_ransac), range-checked (OrbHipError with E_ARG), draws included.  n_iterations None = max_its, i.e.
        PnPsolver::find; state [C, 2], best_inliers [C, cap] and best_Tcw [C, 12] resume solvers an earlier call left.
        Returns dict(report, Tcw, inliers, state, best_inliers, best_Tcw); what the call does not write holds `fill`."""
        params = params or self.pnp_params()
        k, m, kf, M, Cn, cap, rows, n_pts, pcap = self._pnp_inputs(kps, matches, kf_index, pmap)
        d = np.ascontiguousarray(draws, np.int32).reshape(Cn, -1, 4) if Cn else np.zeros((0, int(params.max_its), 4), np.int32)
        sig = self._sigma2(level_sigma2, cam)
        c1 = max(Cn, 1)
        st = np.zeros((c1, 2), np.int32)
        bi = np.full((c1, cap), fill, np.uint8)
        bt = np.full(c1 * 48, fill, np.uint8).view(np.float32).reshape(c1, 12)
        if state is not None:
            st[:Cn] = np.asarray(state, np.int32).reshape(Cn, 2)
            bi[:Cn] = np.asarray(best_inliers, np.uint8).reshape(Cn, cap)
            bt[:Cn] = np.asarray(best_Tcw, np.float32).reshape(Cn, 12)
        T = np.full(c1 * 48, fill, np.uint8).view(np.float32).reshape(c1, 12)
        inl = np.full((c1, cap), fill, np.uint8)
        rep = np.full(c1 * 32, fill, np.uint8).view(np.int32).reshape(c1, 8)
        pad = lambda a: None if a is None else (np.zeros(4, a.dtype) if a.size == 0 else a)  # noqa: E731
        keep = {key: pad(v) for key, v in M.items()}
        rm = self._record(capi.PnpMap, {key: ptr(a).value for key, a in keep.items()}, optional=("slot_point",))
        args = [pad(k), pad(m), pad(kf), pad(d)]
        check(self._lib.orbhip_pnp_ransac(self._h, Cn, ptr(args[0]), len(k), cap, ptr(args[1]), int(match_form),
                                          None if kf is None else ptr(args[2]), rows, n_pts, pcap, C.byref(rm), C.byref(cam), ptr(sig),
                                          C.byref(params), ptr(args[3]), d.shape[1], int(params.max_its if n_iterations is None else n_iterations),
                                          ptr(st), ptr(bi), ptr(bt), ptr(T), ptr(inl), ptr(rep)), "orbhip_pnp_ransac")
        return dict(report=rep[:Cn].copy(), Tcw=T[:Cn].copy(), inliers=inl[:Cn].copy(), state=st[:Cn].copy(),
                    best_inliers=bi[:Cn].copy(), best_Tcw=bt[:Cn].copy())

    # -- pose optimisation (src/Optimizer.cc:239-451) ---------------------------
    def PoseOptimizationDevice(self, frames, d_kps, d_n, cap, d_u_right, d_world, d_point_flags, wrows, pcap, d_world_row, cam,
                               inv_level_sigma2, d_Tcw, d_frame_point, d_outlier, d_discarded, d_report,
                               mode=capi.POSEOPT_PLAIN, flags=0):
        """Optimizer::PoseOptimization for `frames` frames, one workgroup each, and with mode DISCARD / LOCAL_MAP the loop of
        Tracking that follows it (orbhip_pose_optimization_device in include/orbhip.h).  The d_* are device addresses (ints,
        or tensors); d_u_right, d_point_flags (PLAIN only), d_world_row and d_discarded may be None.  Asynchronous on the
        matcher's stream."""
        sig = self._sigma2(inv_level_sigma2, cam)
        dp = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)  # noqa: E731
        check(self._lib.orbhip_pose_optimization_device(self._h, int(frames), dp(d_kps), dp(d_n), int(cap), dp(d_u_right), dp(d_world),
                                                        dp(d_point_flags), int(wrows), int(pcap), dp(d_world_row), C.byref(cam),
                                                        ptr(sig), int(mode), int(flags), dp(d_Tcw), dp(d_frame_point), dp(d_outlier),
                                                        dp(d_discarded), dp(d_report)), "orbhip_pose_optimization_device")

    def PoseOptimization(self, kps, n, u_right, world, point_flags, world_row, cam, inv_level_sigma2, Tcw, frame_point,
                         outlier=None, mode=capi.POSEOPT_PLAIN, flags=0, fill=0):
        """The same from host arrays in one staged copy, one launch and one read-back (orbhip_pose_optimization),
        range-checked (OrbHipError with E_ARG).  kps [frames, cap] KP_DTYPE, n [frames], u_right [frames, cap] or None,
        world [wrows, pcap, 3], point_flags [wrows, pcap] or None, world_row [frames] or None, Tcw [frames, 12],
        frame_point [frames, cap]; `outlier` [frames, cap] is the caller's mvbOutlier (default: `fill` bytes).  Returns
        dict(Tcw, frame_point, outlier, discarded, report): copies, what the call does not write holds the input / `fill`."""
        fp = np.array(frame_point, np.int32, order="C", ndmin=2)
        frames, cap = fp.shape
        k = np.ascontiguousarray(kps, KP_DTYPE).reshape(frames, cap)
        nn = np.ascontiguousarray(n, np.int32).reshape(frames)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32).reshape(frames, cap)
        w = np.ascontiguousarray(world, np.float32)
        w = w.reshape((1,) + w.shape) if w.ndim == 2 else w
        wrows, pcap = w.shape[0], w.shape[1]
        pf = None if point_flags is None else np.ascontiguousarray(point_flags, np.uint8).reshape(wrows, pcap)
        row = None if world_row is None else np.ascontiguousarray(world_row, np.int32).reshape(frames)
        sig = self._sigma2(inv_level_sigma2, cam)
        f1 = max(frames, 1)
        T = np.zeros((f1, 12), np.float32)
        T[:frames] = np.asarray(Tcw, np.float32).reshape(frames, 12)
        out = np.full((f1, cap), fill, np.uint8)
        if outlier is not None:
            out[:frames] = np.asarray(outlier, np.uint8).reshape(frames, cap)
        dis = np.full(f1 * cap * 4, fill, np.uint8).view(np.int32).reshape(f1, cap)
        rep = np.full(f1 * 32, fill, np.uint8).view(np.int32).reshape(f1, 8)
        pad = lambda a: None if a is None else (np.zeros(8, a.dtype) if a.size == 0 else a)  # noqa: E731
        args = [pad(a) for a in (k, nn, ur, w, pf, row, fp)]
        check(self._lib.orbhip_pose_optimization(self._h, frames, ptr(args[0]), ptr(args[1]), cap, ptr(args[2]), ptr(args[3]),
                                                 ptr(args[4]), wrows, pcap, ptr(args[5]), C.byref(cam), ptr(sig), int(mode), int(flags),
                                                 ptr(T), ptr(args[6]), ptr(out), ptr(dis), ptr(rep)), "orbhip_pose_optimization")
        return dict(Tcw=T[:frames].copy(), frame_point=fp.copy(), outlier=out[:frames].copy(),
                    discarded=dis[:frames].copy(), report=rep[:frames].copy())

    # -- Sim3 optimisation (src/Optimizer.cc:1046-1241) --------------------------
    def OptimizeSim3Device(self, C_, cur, d_kf_index, cam, rows, cap, np_, pcap, tables, match_form, inv_level_sigma2,
                           d_matched12, d_sim3, d_S12, d_Scw, d_report, th2=10.0, fix_scale=False, d_select=None):
        """Optimizer::OptimizeSim3 for the current key frame and C_ loop candidates, one workgroup each
        (orbhip_optimize_sim3_device in include/orbhip.h).  `tables` is a dict with the keys of SIM3_TABLES holding device
        addresses (ints, or tensors), the d_* are device addresses; d_Scw and d_select may be None.  Asynchronous on the
        matcher's stream."""
        sig = self._sigma2(inv_level_sigma2, cam)
        rt = self._record(capi.Sim3Tables, tables)
        dp = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)  # noqa: E731
        check(self._lib.orbhip_optimize_sim3_device(self._h, int(C_), int(cur), dp(d_kf_index), C.byref(cam), int(rows), int(cap),
                                                    int(np_), int(pcap), C.byref(rt), int(match_form), ptr(sig), float(th2),
                                                    int(bool(fix_scale)), dp(d_select), dp(d_matched12), dp(d_sim3), dp(d_S12),
                                                    dp(d_Scw), dp(d_report)), "orbhip_optimize_sim3_device")

    def OptimizeSim3(self, tables, cur, kf_index, cam, matched12, match_form, inv_level_sigma2, sim3, th2=10.0, fix_scale=False,
                     select=None, want_scw=True, fill=0):
        """The same from host arrays in one staged copy, one launch and one read-back (orbhip_optimize_sim3), range-checked
        (OrbHipError with E_ARG).  `tables` as for Sim3Setup, matched12 [C, cap], sim3 [C, 16] as Sim3Iterate returns it,
        select [C] or None.  Returns dict(matched12 [C, cap], S12 [C, 8] float64, Scw [C, 12] float32 or None, report [C, 8] in
        the order of capi.SIM3OPT_REPORT): copies, what the call does not write holds the input / `fill` bytes."""
        T, rows, cap, n_pts, pcap = self._sim3_tables(tables)
        kf = np.ascontiguousarray(kf_index, np.int32).reshape(-1)
        Cn = len(kf)
        c1 = max(Cn, 1)
        m12 = np.zeros((c1, cap), np.int32)
        m12[:Cn] = np.asarray(matched12, np.int32).reshape(Cn, cap)
        rec = np.zeros((c1, 16), np.float32)
        rec[:Cn] = np.asarray(sim3, np.float32).reshape(Cn, 16)
        sel = None if select is None else np.ascontiguousarray(select, np.uint8).reshape(Cn)
        sig = self._sigma2(inv_level_sigma2, cam)
        S12 = np.full(c1 * 64, fill, np.uint8).view(np.float64).reshape(c1, 8)
        Scw = np.full(c1 * 48, fill, np.uint8).view(np.float32).reshape(c1, 12) if want_scw else None
        rep = np.full(c1 * 32, fill, np.uint8).view(np.int32).reshape(c1, 8)
        keep = {k: (np.zeros(1, a.dtype) if a.size == 0 else a) for k, a in T.items()}
        rt = self._record(capi.Sim3Tables, {k: ptr(a).value for k, a in keep.items()})
        pad = [None if a is None else (np.zeros(4, a.dtype) if a.size == 0 else a) for a in (kf, sel)]
        check(self._lib.orbhip_optimize_sim3(self._h, Cn, int(cur), ptr(pad[0]), C.byref(cam), rows, cap, n_pts, pcap, C.byref(rt),
                                             int(match_form), ptr(sig), float(th2), int(bool(fix_scale)), ptr(pad[1]), ptr(m12),
                                             ptr(rec), ptr(S12), ptr(Scw), ptr(rep)), "orbhip_optimize_sim3")
        return dict(matched12=m12[:Cn].copy(), S12=S12[:Cn].copy(), Scw=None if Scw is None else Scw[:Cn].copy(),
                    report=rep[:Cn].copy())

    # -- local bundle adjustment (src/Optimizer.cc:453-778) ----------------------
    LBA_TABLES = tuple(k for k, _ in capi.LbaTables._fields_)
    LBA_OUT = tuple(k for k, _ in capi.LbaOut._fields_)
    _LBA_DTYPES = dict(slot_point=np.int32, n=np.int32, kf_bad=np.uint8, obs_start=np.int32, obs_kf=np.int32, obs_idx=np.int32,
                       flags=np.uint8, kps=capi.KP_DTYPE, u_right=np.float32, ord_kf=np.int32, n_ord=np.int32, Tcw=np.float32,
                       world=np.float32)

    def LocalBundleAdjustmentDevice(self, cur, id0_row, cam, rows, cap, np_, pcap, tables, inv_level_sigma2, max_points, max_edges,
                                    out, d_stop=None):
        """Optimizer::LocalBundleAdjustment for the key frame in row `cur` (orbhip_local_bundle_adjustment_device in
        include/orbhip.h).  `tables` and `out` are dicts with the keys of LBA_TABLES / LBA_OUT holding device addresses (ints,
        or tensors); kf_bad and u_right may be None; Tcw and world are updated in place.  d_stop: a device byte or None.
        Asynchronous on the matcher's stream: a fixed sequence of small launches, no host synchronisation."""
        sig = self._sigma2(inv_level_sigma2, cam)
        rt, ro = self._record(capi.LbaTables, tables, optional=("kf_bad", "u_right")), self._record(capi.LbaOut, out)
        dp = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)  # noqa: E731
        check(self._lib.orbhip_local_bundle_adjustment_device(self._h, int(cur), int(id0_row), C.byref(cam), int(rows), int(cap),
                                                              int(np_), int(pcap), C.byref(rt), ptr(sig), int(max_points),
                                                              int(max_edges), dp(d_stop), C.byref(ro)),
              "orbhip_local_bundle_adjustment_device")

    def LocalBundleAdjustment(self, tables, cur, id0_row, cam, inv_level_sigma2, max_points, max_edges, stop=None, fill=0):
        """The same from host arrays in one staged copy, the call and one read-back (orbhip_local_bundle_adjustment),
        range-checked (OrbHipError with E_ARG).  `tables`: dict with the keys of LBA_TABLES (slot_point [rows, cap], n [rows],
        kf_bad [rows] or None, obs_start [np+1], obs_kf, obs_idx, flags [pcap], kps [rows, cap] KP_DTYPE, u_right [rows, cap]
        or None, ord_kf [rows, rows], n_ord [rows], Tcw [rows, 12], world [pcap, 3]); stop: None or the value of the stop byte.
        Returns dict(Tcw, world, local_kf [rows], fixed_kf [rows], local_point [max_points], erase [max_edges, 3], report [16]
        in the order of capi.LBA_REPORT): copies, what the call does not write holds the input / `fill` bytes."""
        T = {}
        for k in self.LBA_TABLES:
            if tables.get(k) is None:
                if k in ("kf_bad", "u_right"):
                    T[k] = None
                    continue
                raise ValueError("tables[%r] is missing" % k)
            T[k] = np.array(tables[k], self._LBA_DTYPES[k], order="C") if k in ("Tcw", "world") else \
                np.ascontiguousarray(tables[k], self._LBA_DTYPES[k])
        rows, cap = T["slot_point"].shape
        n_pts, pcap = len(T["obs_start"]) - 1, len(T["flags"])
        T["Tcw"], T["world"] = T["Tcw"].reshape(rows, 12), T["world"].reshape(pcap, 3)
        sig = self._sigma2(inv_level_sigma2, cam)
        ints = lambda count: np.full(max(count, 1) * 4, fill, np.uint8).view(np.int32)  # noqa: E731
        O = dict(local_kf=ints(rows), fixed_kf=ints(rows), local_point=ints(max_points), erase=ints(max_edges * 3), report=ints(16))
        keep = {k: (None if a is None else (np.zeros(4, a.dtype) if a.size == 0 else a)) for k, a in T.items()}
        rt = self._record(capi.LbaTables, {k: (None if a is None else ptr(a).value) for k, a in keep.items()}, optional=("kf_bad", "u_right"))
        ro = self._record(capi.LbaOut, {k: ptr(a).value for k, a in O.items()})
        sb = None if stop is None else np.array([stop], np.uint8)
        check(self._lib.orbhip_local_bundle_adjustment(self._h, int(cur), int(id0_row), C.byref(cam), rows, cap, n_pts, pcap,
                                                       C.byref(rt), ptr(sig), int(max_points), int(max_edges), ptr(sb), C.byref(ro)),
              "orbhip_local_bundle_adjustment")
        return dict(Tcw=keep["Tcw"].copy(), world=keep["world"].copy(), local_kf=O["local_kf"][:rows].copy(),
                    fixed_kf=O["fixed_kf"][:rows].copy(), local_point=O["local_point"][:max_points].copy(),
                    erase=O["erase"][:max_edges * 3].reshape(max_edges, 3).copy(), report=O["report"].copy())

    # -- essential-graph optimisation (src/Optimizer.cc:781-1044) -----------------
    EG_TABLES = tuple(k for k, _ in capi.EgTables._fields_)
    EG_OUT = tuple(k for k, _ in capi.EgOut._fields_)
    _EG_DTYPES = dict(kf_bad=np.uint8, kf_id=np.int32, parent=np.int32, conn_w=np.int32, ord_kf=np.int32, ord_w=np.int32, n_ord=np.int32,
                      loop_start=np.int32, loop_kf=np.int32, lc_start=np.int32, lc_kf=np.int32, corrected=np.float64,
                      non_corrected=np.float64, in_corrected=np.uint8, in_non_corrected=np.uint8, flags=np.uint8, ref_kf=np.int32,
                      corrected_by_kf=np.int32, corrected_ref=np.int32, Tcw=np.float32, world=np.float32)
    _EG_POINT_KEYS = ("flags", "ref_kf", "corrected_by_kf", "corrected_ref", "world")

    def OptimizeEssentialGraphDevice(self, cur, loop_row, rows, pcap, tables, fix_scale, max_edges, out):
        """Optimizer::OptimizeEssentialGraph between the key frames in rows `cur` and `loop_row`
        (orbhip_optimize_essential_graph_device in include/orbhip.h).  `tables` and `out` are dicts with the keys of EG_TABLES /
        EG_OUT holding device addresses (ints, or tensors); kf_bad may be None, and with pcap == 0 so may the point arrays; Tcw
        and world are updated in place.  The call synchronises the matcher's stream once per Levenberg-Marquardt trial; when it
        returns the outputs are written."""
        optional = ("kf_bad",) + (self._EG_POINT_KEYS if pcap == 0 else ())
        rt = self._record(capi.EgTables, tables, optional=optional)
        ro = self._record(capi.EgOut, out, optional=("point_list",) if pcap == 0 else ())
        check(self._lib.orbhip_optimize_essential_graph_device(self._h, int(cur), int(loop_row), int(rows), int(pcap), C.byref(rt),
                                                               int(bool(fix_scale)), int(max_edges), C.byref(ro)),
              "orbhip_optimize_essential_graph_device")

    def OptimizeEssentialGraph(self, tables, cur, loop_row, fix_scale, max_edges, fill=0):
        """The same from host arrays in one staged copy, the call and one read-back (orbhip_optimize_essential_graph), range-checked
        (OrbHipError with E_ARG; also for a parent, loop_kf entry or lc_kf entry that is a bad row).  `tables`: dict with the keys
        of EG_TABLES (kf_bad [rows] or None, kf_id, parent, n_ord [rows], conn_w, ord_kf, ord_w [rows, rows], loop_start / lc_start
        [rows + 1], loop_kf, lc_kf, corrected / non_corrected [rows, 8] float64, in_corrected / in_non_corrected [rows], flags,
        ref_kf, corrected_by_kf, corrected_ref [pcap], Tcw [rows, 12], world [pcap, 3]).  Returns dict(Tcw, world, point_list
        [pcap], Scw [rows, 8], Swc [rows, 8], report [16] in the order of capi.EG_REPORT): copies, what the call does not write
        holds the input / `fill` bytes."""
        T = {}
        for k in self.EG_TABLES:
            if tables.get(k) is None:
                if k == "kf_bad":
                    T[k] = None
                    continue
                raise ValueError("tables[%r] is missing" % k)
            T[k] = np.array(tables[k], self._EG_DTYPES[k], order="C") if k in ("Tcw", "world") else \
                np.ascontiguousarray(tables[k], self._EG_DTYPES[k])
        rows, pcap = len(T["kf_id"]), len(T["flags"])
        T["Tcw"], T["world"] = T["Tcw"].reshape(rows, 12), T["world"].reshape(pcap, 3)
        raw = lambda count, dt: np.full(max(count, 1) * np.dtype(dt).itemsize, fill, np.uint8).view(dt)  # noqa: E731
        O = dict(point_list=raw(pcap, np.int32), Scw=raw(rows * 8, np.float64), Swc=raw(rows * 8, np.float64), report=raw(16, np.int32))
        keep = {k: (None if a is None else (np.zeros(4, a.dtype) if a.size == 0 else a)) for k, a in T.items()}
        rt = self._record(capi.EgTables, {k: (None if a is None else ptr(a).value) for k, a in keep.items()}, optional=("kf_bad",))
        ro = self._record(capi.EgOut, {k: ptr(a).value for k, a in O.items()})
        check(self._lib.orbhip_optimize_essential_graph(self._h, int(cur), int(loop_row), rows, pcap, C.byref(rt), int(bool(fix_scale)),
                                                        int(max_edges), C.byref(ro)), "orbhip_optimize_essential_graph")
        return dict(Tcw=T["Tcw"].copy(), world=T["world"].copy(), point_list=O["point_list"][:pcap].copy(),
                    Scw=O["Scw"][:rows * 8].reshape(rows, 8).copy(), Swc=O["Swc"][:rows * 8].reshape(rows, 8).copy(),
                    report=O["report"].copy())

    def EssentialGraphCounters(self):
        """(stream synchronisations, kernel launches) of this matcher's last OptimizeEssentialGraph* call."""
        c = np.zeros(2, np.int32)
        check(self._lib.orbhip_optimize_essential_graph_counters(self._h, ptr(c)), "orbhip_optimize_essential_graph_counters")
        return int(c[0]), int(c[1])

    # -- global bundle adjustment (src/Optimizer.cc:41-237, src/LoopClosing.cc:676-737) ----
    GBA_TABLES = tuple(k for k, _ in capi.GbaTables._fields_)
    GBA_OUT = tuple(k for k, _ in capi.GbaOut._fields_)
    GBA_APPLY = tuple(k for k, _ in capi.GbaApply._fields_)
    _GBA_DTYPES = dict(kf_bad=np.uint8, kf_id=np.int32, obs_start=np.int32, obs_kf=np.int32, obs_idx=np.int32, flags=np.uint8,
                       kps=capi.KP_DTYPE, u_right=np.float32, Tcw=np.float32, world=np.float32)
    _GBA_APPLY_DTYPES = dict(origins=np.int32, parent=np.int32, kf_bad=np.uint8, pt_mark=np.uint8, posGBA=np.float32, flags=np.uint8,
                             ref_kf=np.int32, kf_mark=np.uint8, TcwGBA=np.float32, Tcw=np.float32, world=np.float32,
                             TcwBefGBA=np.float32, report=np.int32)

    def GlobalBundleAdjustmentDevice(self, cam, rows, cap, np_, pcap, tables, inv_level_sigma2, iterations, robust, mode, max_points,
                                     max_edges, out, d_kf_list=None, nkf=0, d_pt_list=None, npt=0, d_stop=None):
        """Optimizer::BundleAdjustment over device arrays (orbhip_global_bundle_adjustment_device in include/orbhip.h); with both
        lists None it is GlobalBundleAdjustemnt.  `tables` and `out` are dicts with the keys of GBA_TABLES / GBA_OUT holding
        device addresses (ints, or tensors); kf_bad and u_right may be None, and so may the outputs of the other mode
        (capi.GBA_IN_PLACE writes Tcw, world and point_list; capi.GBA_STAGED writes TcwGBA, posGBA and the marks).  The call
        synchronises the matcher's stream once per Levenberg-Marquardt trial; when it returns the outputs are written."""
        sig = self._sigma2(inv_level_sigma2, cam)
        rt = self._record(capi.GbaTables, tables, optional=("kf_bad", "u_right"))
        ro = self._record(capi.GbaOut, out, optional=("TcwGBA", "posGBA", "kf_mark", "pt_mark", "point_list"))
        dp = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a)  # noqa: E731
        check(self._lib.orbhip_global_bundle_adjustment_device(self._h, C.byref(cam), int(rows), int(cap), int(np_), int(pcap),
                                                               C.byref(rt), ptr(sig), dp(d_kf_list), int(nkf), dp(d_pt_list), int(npt),
                                                               int(iterations), int(bool(robust)), int(mode), int(max_points),
                                                               int(max_edges), dp(d_stop), C.byref(ro)),
              "orbhip_global_bundle_adjustment_device")

    def GlobalBundleAdjustment(self, tables, cam, inv_level_sigma2, iterations, robust, mode, max_points, max_edges, kf_list=None,
                               pt_list=None, stop=None, out=None, fill=0):
        """The same from host arrays in one staged copy, the call and one read-back (orbhip_global_bundle_adjustment), range-checked
        (OrbHipError with E_ARG; also for a null vertex).  `tables`: dict with the keys of GBA_TABLES (kf_bad [rows] or None, kf_id
        [rows], obs_start [np+1], obs_kf, obs_idx, flags [pcap], kps [rows, cap] KP_DTYPE, u_right [rows, cap] or None, Tcw
        [rows, 12], world [pcap, 3]); kf_list / pt_list: None or the lists; stop: None or the value of the stop byte; out: None or
        a dict with the caller's TcwGBA, posGBA, kf_mark, pt_mark to start from (STAGED).  Returns dict(Tcw, world, TcwGBA, posGBA,
        kf_mark, pt_mark, point_list [max_points], report [16] in the order of capi.GBA_REPORT): copies, what the call does not
        write holds the input / `fill` bytes."""
        T = {}
        for k in self.GBA_TABLES:
            if tables.get(k) is None:
                if k in ("kf_bad", "u_right"):
                    T[k] = None
                    continue
                raise ValueError("tables[%r] is missing" % k)
            T[k] = np.array(tables[k], self._GBA_DTYPES[k], order="C") if k in ("Tcw", "world") else \
                np.ascontiguousarray(tables[k], self._GBA_DTYPES[k])
        rows, cap = T["kps"].shape
        n_pts, pcap = len(T["obs_start"]) - 1, len(T["flags"])
        T["Tcw"], T["world"] = T["Tcw"].reshape(rows, 12), T["world"].reshape(pcap, 3)
        sig = self._sigma2(inv_level_sigma2, cam)
        raw = lambda count, dt: np.full(max(count, 1) * np.dtype(dt).itemsize, fill, np.uint8).view(dt)  # noqa: E731
        O = dict(TcwGBA=raw(rows * 12, np.float32), posGBA=raw(pcap * 3, np.float32), kf_mark=raw(rows, np.uint8),
                 pt_mark=raw(pcap, np.uint8), point_list=raw(max_points, np.int32), report=raw(16, np.int32))
        for k in ("TcwGBA", "posGBA", "kf_mark", "pt_mark"):
            if out is not None and out.get(k) is not None:
                src = np.ascontiguousarray(out[k], O[k].dtype).reshape(-1)
                O[k][:len(src)] = src
        keep = {k: (None if a is None else (np.zeros(4, a.dtype) if a.size == 0 else a)) for k, a in T.items()}
        rt = self._record(capi.GbaTables, {k: (None if a is None else ptr(a).value) for k, a in keep.items()}, optional=("kf_bad", "u_right"))
        ro = self._record(capi.GbaOut, {k: ptr(a).value for k, a in O.items()})
        kl = None if kf_list is None else np.ascontiguousarray(kf_list, np.int32).reshape(-1)
        pl = None if pt_list is None else np.ascontiguousarray(pt_list, np.int32).reshape(-1)
        pad = [None if a is None else (np.zeros(4, np.int32) if a.size == 0 else a) for a in (kl, pl)]
        sb = None if stop is None else np.array([stop], np.uint8)
        check(self._lib.orbhip_global_bundle_adjustment(self._h, C.byref(cam), rows, cap, n_pts, pcap, C.byref(rt), ptr(sig), ptr(pad[0]),
                                                        0 if kl is None else len(kl), ptr(pad[1]), 0 if pl is None else len(pl),
                                                        int(iterations), int(bool(robust)), int(mode), int(max_points), int(max_edges),
                                                        ptr(sb), C.byref(ro)), "orbhip_global_bundle_adjustment")
        return dict(Tcw=keep["Tcw"].copy(), world=T["world"].copy(), TcwGBA=O["TcwGBA"][:rows * 12].reshape(rows, 12).copy(),
                    posGBA=O["posGBA"][:pcap * 3].reshape(pcap, 3).copy(), kf_mark=O["kf_mark"][:rows].copy(),
                    pt_mark=O["pt_mark"][:pcap].copy(), point_list=O["point_list"][:max_points].copy(), report=O["report"].copy())

    def GlobalBACounters(self):
        """(stream synchronisations, kernel launches) of this matcher's last GlobalBundleAdjustment* call."""
        c = np.zeros(2, np.int32)
        check(self._lib.orbhip_global_bundle_adjustment_counters(self._h, ptr(c)), "orbhip_global_bundle_adjustment_counters")
        return int(c[0]), int(c[1])

    def ApplyGlobalBADevice(self, n_origins, rows, pcap, arrays):
        """The map update after a staged global bundle adjustment (orbhip_apply_global_ba_device in include/orbhip.h): `arrays` is a
        dict with the keys of GBA_APPLY holding device addresses (ints, or tensors); kf_bad may be None, and with pcap == 0 so may
        the point arrays.  Asynchronous on the matcher's stream, two launches."""
        optional = ("kf_bad",) + (("pt_mark", "posGBA", "flags", "ref_kf", "world") if pcap == 0 else ()) + (("origins",) if n_origins == 0 else ())
        rec = self._record(capi.GbaApply, arrays, optional=optional)
        check(self._lib.orbhip_apply_global_ba_device(self._h, int(n_origins), int(rows), int(pcap), C.byref(rec)),
              "orbhip_apply_global_ba_device")

    def ApplyGlobalBA(self, arrays, fill=0):
        """The same from host arrays (orbhip_apply_global_ba), range-checked (OrbHipError with E_ARG).  `arrays`: dict with origins
        [n_origins], parent [rows], kf_bad [rows] or None, kf_mark [rows], TcwGBA / Tcw [rows, 12], pt_mark, flags, ref_kf [pcap],
        posGBA / world [pcap, 3].  Returns dict(kf_mark, TcwGBA, Tcw, world, TcwBefGBA [rows, 12], report [8] in the order of
        capi.GBA_APPLY_REPORT): copies, what the call does not write holds the input / `fill` bytes."""
        A = {}
        for k in self.GBA_APPLY:
            if k in ("TcwBefGBA", "report"):
                continue
            if arrays.get(k) is None:
                if k == "kf_bad":
                    A[k] = None
                    continue
                raise ValueError("arrays[%r] is missing" % k)
            A[k] = np.array(arrays[k], self._GBA_APPLY_DTYPES[k], order="C").reshape(-1)
        rows, pcap, n_origins = len(A["parent"]), len(A["flags"]), len(A["origins"])
        A["TcwBefGBA"] = np.full(rows * 48, fill, np.uint8).view(np.float32)
        A["report"] = np.full(32, fill, np.uint8).view(np.int32)
        keep = {k: (None if a is None else (np.zeros(4, a.dtype) if a.size == 0 else a)) for k, a in A.items()}
        rec = self._record(capi.GbaApply, {k: (None if a is None else ptr(a).value) for k, a in keep.items()}, optional=("kf_bad",))
        check(self._lib.orbhip_apply_global_ba(self._h, n_origins, rows, pcap, C.byref(rec)), "orbhip_apply_global_ba")
        return dict(kf_mark=A["kf_mark"].copy(), TcwGBA=A["TcwGBA"].reshape(rows, 12).copy(), Tcw=A["Tcw"].reshape(rows, 12).copy(),
                    world=A["world"].reshape(pcap, 3).copy(), TcwBefGBA=A["TcwBefGBA"].reshape(rows, 12).copy(), report=A["report"].copy())

    # -- device-resident, batched SearchByProjection ---------------------------
    def set_stream(self, stream):
        check(self._lib.orbhip_matcher_set_stream(self._h, stream), "orbhip_matcher_set_stream")

    def sync(self):
        check(self._lib.orbhip_matcher_sync(self._h), "orbhip_matcher_sync")

    def FillScratch(self, byte):
        """Test hook (orbhip_matcher_fill_scratch in include/orbhip.h): every workspace of the handle is overwritten with `byte`;
        returns the number of bytes filled.  No call's result may depend on it."""
        n = C.c_ulonglong(0)
        check(self._lib.orbhip_matcher_fill_scratch(self._h, int(byte), C.byref(n)), "orbhip_matcher_fill_scratch")
        return int(n.value)

    def SearchByProjectionFrameDevice(self, pairs, d_kps, d_desc, d_n, cap, bounds, d_q, d_qdesc, d_nq, qcap, d_assign,
                                      d_nmatches, d_u_right=0, d_taken=0):
        """All d_* are device pointers (ints).  bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY)."""
        b = [np.float32(v) for v in bounds]
        inv_w = np.float32(FRAME_GRID_COLS) / (b[2] - b[0])
        inv_h = np.float32(FRAME_GRID_ROWS) / (b[3] - b[1])
        check(self._lib.orbhip_search_by_projection_frame_device(
            self._h, pairs, d_kps, d_desc, d_n, cap, d_u_right, d_taken, b[0], b[1], inv_w, inv_h, d_q, d_qdesc, d_nq,
            qcap, int(self.mbCheckOrientation), d_assign, d_nmatches), "orbhip_search_by_projection_frame_device")

    def SearchForInitializationDevice(self, pairs, d_kps, d_desc, d_n, cap, f1_first, f1_step, f2_first, f2_step, bounds,
                                      keep_prev, d_prev_matched, windowSize, d_matches12, d_nmatches):
        """Batched, device-resident SearchForInitialization; keep_prev = 0 resets vbPrevMatched to F1's keypoints."""
        b = [np.float32(v) for v in bounds]
        inv_w = np.float32(FRAME_GRID_COLS) / (b[2] - b[0])
        inv_h = np.float32(FRAME_GRID_ROWS) / (b[3] - b[1])
        check(self._lib.orbhip_search_for_initialization_device(
            self._h, pairs, d_kps, d_desc, d_n, cap, f1_first, f1_step, f2_first, f2_step, b[0], b[1], inv_w, inv_h,
            int(not keep_prev), d_prev_matched, int(windowSize), self.mfNNratio, int(self.mbCheckOrientation), d_matches12,
            d_nmatches), "orbhip_search_for_initialization_device")

    # -- projection prologues on the device (src/ORBmatcher.cc:1339-1390; src/Frame.cc:269-325) ------------------
    def ProjectLastFrame(self, cam, Tcw, Tlw, world, flags, last_keys, th, bMono):
        """Prologue of SearchByProjection(CurrentFrame, LastFrame, th, bMono): QUERY_DTYPE[n] for
        SearchByProjectionFrame.  Tcw / Tlw: 4x4 or 3x4 float32; world [n,3]; flags [n] uint8 (POINT_* bits)."""
        Tc = np.ascontiguousarray(np.asarray(Tcw, np.float32)[:3, :4])
        Tl = np.ascontiguousarray(np.asarray(Tlw, np.float32)[:3, :4])
        world = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
        flags = np.ascontiguousarray(flags, np.uint8)
        keys = np.ascontiguousarray(last_keys, KP_DTYPE)
        n = len(keys)
        q = np.zeros(n, QUERY_DTYPE)
        check(self._lib.orbhip_project_last_frame(self._h, C.byref(cam), ptr(Tc), ptr(Tl), n, ptr(world), ptr(flags),
                                                  ptr(keys), float(th), int(bMono), ptr(q)), "orbhip_project_last_frame")
        return q

    def FrustumQueries(self, cam, Tcw, world, normal, max_dist, min_dist, flags, viewingCosLimit, th):
        """Frame::isInFrustum for n map points + the window of SearchByProjection(F, vpMapPoints, th).
        Returns (QUERY_DTYPE[n], view_cos[n])."""
        Tc = np.ascontiguousarray(np.asarray(Tcw, np.float32)[:3, :4])
        world = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
        normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mx, mn = np.ascontiguousarray(max_dist, np.float32), np.ascontiguousarray(min_dist, np.float32)
        flags = np.ascontiguousarray(flags, np.uint8)
        n = len(world)
        q, vc = np.zeros(n, QUERY_DTYPE), np.zeros(n, np.float32)
        check(self._lib.orbhip_frustum_queries(self._h, C.byref(cam), ptr(Tc), n, ptr(world), ptr(normal), ptr(mx), ptr(mn),
                                               ptr(flags), float(viewingCosLimit), float(th), ptr(q), ptr(vc)),
              "orbhip_frustum_queries")
        return q, vc

    # -- Fuse x2 (src/ORBmatcher.cc:825-1100) and SearchBySim3 (:1102-1326), prologue included ---------------------
    @staticmethod
    def _pts(world, normal, max_dist, min_dist, flags):
        w = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
        nn = None if normal is None else np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        return (w, nn, np.ascontiguousarray(max_dist, np.float32), np.ascontiguousarray(min_dist, np.float32),
                np.ascontiguousarray(flags, np.uint8))

    def KeyFrameQueries(self, cam, mode, double_invz, T1, T2, world, normal, max_dist, min_dist, flags, th):
        T1 = np.ascontiguousarray(np.asarray(T1, np.float32)[:3, :4])
        T2 = None if T2 is None else np.ascontiguousarray(np.asarray(T2, np.float32)[:3, :4])
        w, nn, mx, mn, fg = self._pts(world, normal, max_dist, min_dist, flags)
        q = np.zeros(len(w), QUERY_DTYPE)
        check(self._lib.orbhip_keyframe_queries(self._h, C.byref(cam), int(mode), int(double_invz), ptr(T1), ptr(T2), len(w),
                                                ptr(w), ptr(nn), ptr(mx), ptr(mn), ptr(fg), float(th), ptr(q)),
              "orbhip_keyframe_queries")
        return q

    def Fuse(self, KF, cam, Tcw, world, normal, max_dist, min_dist, flags, point_desc, th, inv_level_sigma2, sim3_form=False):
        """Fuse up to the decision: (best_idx[n], best_dist[n]); the caller applies bestDist <= TH_LOW and the
        replace-or-add side effects in order."""
        Tc = np.ascontiguousarray(np.asarray(Tcw, np.float32)[:3, :4])
        w, nn, mx, mn, fg = self._pts(world, normal, max_dist, min_dist, flags)
        pd = np.ascontiguousarray(point_desc, np.uint8).reshape(-1, 32)
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        bi, bd = np.full(max(len(w), 1), -1, np.int32), np.full(max(len(w), 1), 256, np.int32)
        v = KF.c_view()
        check(self._lib.orbhip_fuse(self._h, C.byref(v), C.byref(cam), ptr(Tc), int(sim3_form), len(w), ptr(w), ptr(nn), ptr(mx),
                                    ptr(mn), ptr(fg), ptr(pd), float(th), ptr(sig), ptr(bi), ptr(bd)), "orbhip_fuse")
        return bi[:len(w)].copy(), bd[:len(w)].copy()

    def FuseBatch(self, KFs, cam, Tcw, world, normal, max_dist, min_dist, flags, point_desc, th, inv_level_sigma2,
                  sim3_form=False):
        """Fuse up to the decision for K key frames and one set of n map points (LocalMapping::SearchInNeighbors,
        src/LocalMapping.cc:454-515; LoopClosing::SearchAndFuse, src/LoopClosing.cc:585-610; ORBmatcher::Fuse,
        src/ORBmatcher.cc:825-950 / :975-1075) in one staged copy, one launch and one read-back.  KFs: K FrameViews;
        Tcw [K] poses (4x4 or 3x4); flags [K, n] (POINT_PRESENT = good and not IsInKeyFrame of that target).  Returns
        (best_idx[K, n], best_dist[K, n]); row k equals Fuse(KFs[k], cam, Tcw[k], ..., flags[k], ...)."""
        K = len(KFs)
        Tc = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(K, -1, 4)[:, :3, :]).reshape(K, 12)
        w, nn, mx, mn, _ = self._pts(world, normal, max_dist, min_dist, np.zeros(0, np.uint8))
        n = len(w)
        fg = np.ascontiguousarray(flags, np.uint8).reshape(K, n)
        pd = np.ascontiguousarray(point_desc, np.uint8).reshape(-1, 32)
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        bi, bd = np.full((K, n), -1, np.int32), np.full((K, n), 256, np.int32)
        views = [kf.c_view() for kf in KFs]
        arr = (C.POINTER(capi.FrameView) * max(K, 1))(*[C.pointer(v) for v in views])
        check(self._lib.orbhip_fuse_batch(self._h, K, arr, C.byref(cam), ptr(Tc), int(sim3_form), n, ptr(w), ptr(nn), ptr(mx),
                                          ptr(mn), ptr(fg), ptr(pd), float(th), ptr(sig), ptr(bi), ptr(bd)),
              "orbhip_fuse_batch")
        return bi, bd

    def FuseDevice(self, K, d_kf_index, cam, d_Tcw, d_kps, d_desc, d_n, cap, np_, pcap, d_world, d_normal, d_max_dist,
                   d_min_dist, d_point_desc, d_flags, th, inv_level_sigma2, d_best_idx, d_best_dist, sim3_form=False,
                   d_u_right=0, d_cell_start=0, d_cell_items=0, d_q=0):
        """Device-resident FuseBatch (device pointers as ints; see orbhip_fuse_device in include/orbhip.h): target k is
        frame row kf_index[k] of the extractor-layout arrays, d_flags [K][pcap], outputs [K][pcap].  d_cell_start /
        d_cell_items: the arrays AssignFeaturesToGridDevice wrote for the same frames, or 0 to build the grids inside the
        call.  Asynchronous on the matcher's stream."""
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        if len(sig) < cam.n_levels:
            raise ValueError("inv_level_sigma2 needs one entry per pyramid level")
        check(self._lib.orbhip_fuse_device(self._h, int(K), d_kf_index, C.byref(cam), d_Tcw, int(sim3_form), d_kps, d_desc, d_n,
                                           int(cap), d_u_right, d_cell_start, d_cell_items, int(np_), int(pcap), d_world,
                                           d_normal, d_max_dist, d_min_dist, d_point_desc, d_flags, float(th), ptr(sig),
                                           d_best_idx, d_best_dist, d_q), "orbhip_fuse_device")

    def CreateNewMapPoints(self, cur, node_cur, has_point_cur, depth_cur, Tcw_cur, KFs, nodes, has_points, depths, Tcw,
                           cam, level_sigma2, median_depth=None, bOnlyStereo=False):
        """LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452) up to `new MapPoint` for the current key frame
        `cur` and the K neighbours `KFs` (FrameViews; u_right on all or on none) in one staged copy, one device call and
        one read-back.  nodes[k] / has_points[k] (None = no slot holds a point) / depths[k] (stereo only): one entry per
        key point; Tcw_cur and Tcw [K]: poses (4x4 or 3x4); median_depth [K]: ComputeSceneMedianDepth(2), monocular only.
        Returns a dict: matches12 [K, n], nmatches [K], x3d [K, n, 3], status [K, n] (capi.NEWPOINT_*), skipped [K],
        f12 [K, 3, 3], epipole [K, 2]; INTEGRATION.md section 3 says how the rows are applied in neighbour order."""
        K, n = len(KFs), cur.N
        T0 = np.ascontiguousarray(np.asarray(Tcw_cur, np.float32)[:3, :4]).reshape(12)
        Tc = (np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(K, -1, 4)[:, :3, :]).reshape(K, 12) if K
              else np.zeros((1, 12), np.float32))
        stereo = cur.u_right is not None
        keep = []

        def arr(a, dt, count):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if len(a) != count:
                raise ValueError("per-keypoint arrays must have one entry per keypoint")
            keep.append(a)
            return a

        def table(seq, dt):
            if seq is None:
                return None
            rows = [arr(seq[k], dt, KFs[k].N) for k in range(K)]
            return (C.c_void_p * max(K, 1))(*[None if r is None else r.ctypes.data for r in rows])

        nc, hc = arr(node_cur, np.uint32, n), arr(has_point_cur, np.uint8, n)
        zc = arr(depth_cur, np.float32, n) if stereo else None
        t_node, t_hp = table(nodes, np.uint32), table(has_points, np.uint8)
        t_z = table(depths, np.float32) if stereo else None
        med = None if median_depth is None else np.ascontiguousarray(median_depth, np.float32)
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        if len(sig) < cam.n_levels:
            raise ValueError("level_sigma2 needs one entry per pyramid level")
        out = {"matches12": np.full((K, n), -1, np.int32), "nmatches": np.zeros(K, np.int32),
               "x3d": np.zeros((K, n, 3), np.float32), "status": np.full((K, n), capi.NEWPOINT_NO_MATCH, np.uint8),
               "skipped": np.zeros(K, np.uint8), "f12": np.zeros((K, 3, 3), np.float32),
               "epipole": np.zeros((K, 2), np.float32)}
        views = [kf.c_view() for kf in KFs]
        vc = cur.c_view()
        varr = (C.POINTER(capi.FrameView) * max(K, 1))(*[C.pointer(v) for v in views])
        check(self._lib.orbhip_create_new_map_points(
            self._h, C.byref(vc), ptr(nc), ptr(hc), ptr(zc), ptr(T0), K, varr, t_node, t_hp, t_z, ptr(Tc), ptr(med),
            C.byref(cam), int(bOnlyStereo), int(self.mbCheckOrientation), ptr(sig), ptr(out["matches12"]),
            ptr(out["nmatches"]), ptr(out["x3d"]), ptr(out["status"]), ptr(out["skipped"]), ptr(out["f12"]),
            ptr(out["epipole"])), "orbhip_create_new_map_points")
        return out

    def CreateNewMapPointsDevice(self, cur, K, d_kf_index, cam, d_Tcw, d_kps, d_desc, d_n, cap, d_node, level_sigma2,
                                 d_matches12, d_nmatches, d_x3d, d_status, d_skipped, d_u_right=0, d_depth=0,
                                 d_has_point=0, d_median_depth=0, bOnlyStereo=False, d_f12=0, d_epipole=0):
        """Device-resident CreateNewMapPoints (see orbhip_create_new_map_points_device in include/orbhip.h).  Every d_*
        is a torch tensor on the matcher's device or a raw device pointer (int, 0 = NULL): the current key frame is frame
        row `cur`, neighbour k frame row kf_index[k] of the extractor-layout arrays; outputs [K][cap].  Asynchronous on
        the matcher's stream."""
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        if len(sig) < cam.n_levels:
            raise ValueError("level_sigma2 needs one entry per pyramid level")

        def dp(a):
            return int(a.data_ptr()) if hasattr(a, "data_ptr") else (int(a) or None)

        check(self._lib.orbhip_create_new_map_points_device(
            self._h, int(cur), int(K), dp(d_kf_index), C.byref(cam), dp(d_Tcw), dp(d_kps), dp(d_desc), dp(d_n), int(cap),
            dp(d_u_right), dp(d_depth), dp(d_node), dp(d_has_point), dp(d_median_depth), int(bOnlyStereo),
            int(self.mbCheckOrientation), ptr(sig), dp(d_matches12), dp(d_nmatches), dp(d_x3d), dp(d_status),
            dp(d_skipped), dp(d_f12), dp(d_epipole)), "orbhip_create_new_map_points_device")

    def SearchBySim3(self, KF1, KF2, cam, T1w, T2w, S21, S12, pts1, pts2, th):
        """pts = (world, max_dist, min_dist, flags, desc) per key-frame slot.  Returns (nFound, matches12[N1])."""
        mats = [np.ascontiguousarray(np.asarray(T, np.float32)[:3, :4]) for T in (T1w, T2w, S21, S12)]
        a = [self._pts(p[0], None, p[1], p[2], p[3]) + (np.ascontiguousarray(p[4], np.uint8).reshape(-1, 32),) for p in (pts1, pts2)]
        m12 = np.full(max(KF1.N, 1), -1, np.int32)
        n = C.c_int()
        v1, v2 = KF1.c_view(), KF2.c_view()
        check(self._lib.orbhip_search_by_sim3(self._h, C.byref(v1), C.byref(v2), C.byref(cam), ptr(mats[0]), ptr(mats[1]),
                                              ptr(mats[2]), ptr(mats[3]), ptr(a[0][0]), ptr(a[0][2]), ptr(a[0][3]), ptr(a[0][4]),
                                              ptr(a[0][5]), ptr(a[1][0]), ptr(a[1][2]), ptr(a[1][3]), ptr(a[1][4]), ptr(a[1][5]),
                                              float(th), ptr(m12), C.byref(n)), "orbhip_search_by_sim3")
        return n.value, m12[:KF1.N].copy()

    def ProjectLastFrameDevice(self, pairs, cam, d_Tcw, d_Tlw, d_kps, d_n, cap, last_first, last_step, d_world, d_flags, th,
                               bMono, d_q, d_nq):
        check(self._lib.orbhip_project_last_frame_device(self._h, pairs, C.byref(cam), d_Tcw, d_Tlw, d_kps, d_n, cap,
                                                         last_first, last_step, d_world, d_flags, float(th), int(bMono),
                                                         d_q, d_nq), "orbhip_project_last_frame_device")

    def TrackLastFrameDevice(self, pairs, cam, d_Tcw, d_Tlw, d_kps, d_desc, d_n, cap, cur_first, cur_step, last_first,
                             last_step, d_world, d_flags, th, bMono, d_assign, d_nmatches, d_u_right=0, d_taken=0):
        """Prologue + search + resolve + rotation cull of SearchByProjection(CurrentFrame, LastFrame, th, bMono) for
        `pairs` (current, last) frame pairs of the extractor output arrays, all on the device, one stream."""
        check(self._lib.orbhip_track_last_frame_device(self._h, pairs, C.byref(cam), d_Tcw, d_Tlw, d_kps, d_desc, d_n, cap,
                                                       cur_first, cur_step, last_first, last_step, d_world, d_flags,
                                                       d_u_right, d_taken, float(th), int(bMono),
                                                       int(self.mbCheckOrientation), d_assign, d_nmatches),
              "orbhip_track_last_frame_device")

    def FrustumQueriesDevice(self, frames, cam, d_Tcw, pcap, d_np, d_world, d_normal, d_max_dist, d_min_dist, d_flags,
                             viewingCosLimit, th, d_q, d_view_cos=0):
        check(self._lib.orbhip_frustum_queries_device(self._h, frames, C.byref(cam), d_Tcw, pcap, d_np, d_world, d_normal,
                                                      d_max_dist, d_min_dist, d_flags, float(viewingCosLimit), float(th),
                                                      d_q, d_view_cos), "orbhip_frustum_queries_device")

    def SearchByProjectionPointsDevice(self, pairs, d_kps, d_desc, d_n, cap, bounds, d_q, d_qdesc, d_nq, qcap, d_assign,
                                       d_nmatches, d_u_right=0, d_taken=0):
        b = [np.float32(v) for v in bounds]
        inv_w = np.float32(FRAME_GRID_COLS) / (b[2] - b[0])
        inv_h = np.float32(FRAME_GRID_ROWS) / (b[3] - b[1])
        check(self._lib.orbhip_search_by_projection_points_device(
            self._h, pairs, d_kps, d_desc, d_n, cap, d_u_right, d_taken, b[0], b[1], inv_w, inv_h, d_q, d_qdesc, d_nq,
            qcap, self.mfNNratio, d_assign, d_nmatches), "orbhip_search_by_projection_points_device")

    def ComputeStereoMatchesDevice(self, ext_left, l0, ls, ext_right, r0, rs, pairs, d_kps_l, d_desc_l, d_n_l, d_kps_r,
                                   d_desc_r, d_n_r, cap, mbf, mb, d_u_right, d_depth, d_nmatches):
        """Batched, device-resident ComputeStereoMatches (all d_* are device pointers)."""
        check(self._lib.orbhip_compute_stereo_matches_device(self._h, ext_left._h, l0, ls, ext_right._h, r0, rs, pairs,
                                                             d_kps_l, d_desc_l, d_n_l, d_kps_r, d_desc_r, d_n_r, cap, mbf,
                                                             mb, d_u_right, d_depth, d_nmatches),
              "orbhip_compute_stereo_matches_device")

    # -- Frame::ComputeStereoMatches (src/Frame.cc:466-640) --------------------
    def ComputeStereoMatches(self, extractor_left, extractor_right, keys_l, desc_l, keys_r, desc_r, mbf, mb,
                             frame_l=0, frame_r=0):
        """Pyramids are those held by the two extractor handles after their last call.
        Returns (nmatches, mvuRight, mvDepth)."""
        kl = np.ascontiguousarray(keys_l, KP_DTYPE)
        kr = np.ascontiguousarray(keys_r, KP_DTYPE)
        dl = np.ascontiguousarray(desc_l, np.uint8)
        dr = np.ascontiguousarray(desc_r, np.uint8)
        ur = np.full(max(len(kl), 1), -1, np.float32)
        dp = np.full(max(len(kl), 1), -1, np.float32)
        n = C.c_int()
        check(self._lib.orbhip_compute_stereo_matches(self._h, extractor_left._h, frame_l, extractor_right._h,
                                                      frame_r, ptr(kl), ptr(dl), len(kl), ptr(kr), ptr(dr),
                                                      len(kr), mbf, mb, ptr(ur), ptr(dp), C.byref(n)),
              "orbhip_compute_stereo_matches")
        return n.value, ur[:len(kl)].copy(), dp[:len(kl)].copy()


class SeedReplay:
    """The --seed option of the replay tools: what Tracking does with mvDepth when no pose estimation runs (identity pose).
    The first frame with N > 500 is Tracking::StereoInitialization (src/Tracking.cc:509-540): mode SEED_ALL and the
    reference's line "New map created with <n> points"; every later frame is the depth-sorted creation loop of
    UpdateLastFrame / CreateNewKeyFrame (:812-864, :1073-1133) on a frame without map points: mode SEED_CLOSEST, empty flags.
    summary() is the line the tools print at the end."""

    def __init__(self, matcher, settings):
        from .settings import th_depth
        self.matcher = matcher
        fx, fy, cx, cy = (float(settings["Camera." + k]) for k in ("fx", "fy", "cx", "cy"))
        self.cam = make_camera(fx, fy, cx, cy, (0.0, 0.0, 1.0, 1.0), [1.0], mbf=float(settings["Camera.bf"]))
        self.th_depth = th_depth(settings)
        self.Tcw = np.eye(4, dtype=np.float32)
        self.initialised = False
        self.close = []

    def frame(self, keys_un, depth):
        n = len(keys_un)
        world, flags = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        if not self.initialised:
            if n > 500:                                                  # src/Tracking.cc:511
                counts = self.matcher.SeedStereoPoints(self.cam, self.Tcw, keys_un, depth, self.th_depth, capi.SEED_ALL,
                                                       capi.POINT_PRESENT | capi.POINT_OBSERVED, world, flags)[4]
                print("New map created with %d points" % counts[2])
                self.initialised = True
            return
        counts = self.matcher.SeedStereoPoints(self.cam, self.Tcw, keys_un, depth, self.th_depth, capi.SEED_CLOSEST,
                                               capi.POINT_PRESENT, world, flags)[4]
        self.close.append(counts[2])

    def summary(self):
        return "mean close points per frame: %.2f" % (sum(self.close) / len(self.close) if self.close else 0.0)


def sim3_draws(C_, max_its, n_corr, seed):
    """Valid draws for Sim3Iterate / Sim3Ransac: [C, max_its, 3] int32 from numpy.random.default_rng(seed), draw k of
    candidate c uniform in [0, n_corr[c] - 1 - k], which is what DUtils::Random::RandomInt(0, size - 1) returns for the
    shrinking list (src/Sim3Solver.cc:168).  Candidates with fewer than three correspondences get zeros (never read)."""
    rng = np.random.default_rng(seed)
    n = np.broadcast_to(np.asarray(n_corr, np.int64).reshape(-1), (int(C_),))
    out = np.zeros((int(C_), int(max_its), 3), np.int32)
    for c in range(int(C_)):
        if n[c] >= 3:
            for k in range(3):
                out[c, :, k] = rng.integers(0, n[c] - k, int(max_its))
    return out


def RadiusByViewingCos(viewCos):
    """src/ORBmatcher.cc:131-137"""
    return 2.5 if viewCos > 0.998 else 4.0


def make_camera(fx, fy, cx, cy, bounds, scale_factors, mbf=0.0, mb=0.0):
    """orbhip_camera from plain numbers.  bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY); mfLogScaleFactor =
    log(mfScaleFactor) as the Frame constructor computes it (src/Frame.cc:71: float log of the float scale factor)."""
    cam = capi.Camera()
    cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf, cam.mb = fx, fy, cx, cy, mbf, mb
    cam.min_x, cam.min_y, cam.max_x, cam.max_y = bounds
    sf = np.asarray(scale_factors, np.float32)
    cam.n_levels = len(sf)
    cam.log_scale_factor = float(np.log(np.float32(sf[1] if len(sf) > 1 else 1.2), dtype=np.float32))
    for i, v in enumerate(sf):
        cam.scale_factors[i] = float(v)
    return cam


def project_last_frame(Tcw, K, bounds, world_pts, last_octaves, last_angles, valid, observed, scale_factors,
                       th, mbf=0.0, bForward=False, bBackward=False):
    """Projection prologue of SearchByProjection(CurrentFrame, LastFrame, th, bMono)
    (src/ORBmatcher.cc:1360-1390) in float32, one operation at a time.
    K = (fx, fy, cx, cy); Tcw 4x4; world_pts [n,3].  Returns QUERY_DTYPE[n]."""
    f32 = np.float32
    Tcw = np.asarray(Tcw, f32)
    P = np.asarray(world_pts, f32)
    fx, fy, cx, cy = (f32(v) for v in K)
    n = len(P)
    q = np.zeros(n, QUERY_DTYPE)
    R, t = Tcw[:3, :3], Tcw[:3, 3]
    for i in range(n):
        if not valid[i]:
            continue
        xc = f32(f32(f32(R[0, 0] * P[i, 0]) + f32(R[0, 1] * P[i, 1])) + f32(R[0, 2] * P[i, 2])) + t[0]
        yc = f32(f32(f32(R[1, 0] * P[i, 0]) + f32(R[1, 1] * P[i, 1])) + f32(R[1, 2] * P[i, 2])) + t[1]
        zc = f32(f32(f32(R[2, 0] * P[i, 0]) + f32(R[2, 1] * P[i, 1])) + f32(R[2, 2] * P[i, 2])) + t[2]
        if zc == 0:
            continue
        invzc = f32(1.0 / np.float64(zc))
        if invzc < 0:
            continue
        u = f32(f32(f32(fx * xc) * invzc) + cx)
        v = f32(f32(f32(fy * yc) * invzc) + cy)
        if u < bounds[0] or u > bounds[2] or v < bounds[1] or v > bounds[3]:
            continue
        o = int(last_octaves[i])
        q[i]["valid"] = 1
        q[i]["u"], q[i]["v"] = u, v
        q[i]["radius"] = f32(f32(th) * f32(scale_factors[o]))
        if bForward:
            q[i]["min_level"], q[i]["max_level"] = o, -1
        elif bBackward:
            q[i]["min_level"], q[i]["max_level"] = 0, o
        else:
            q[i]["min_level"], q[i]["max_level"] = o - 1, o + 1
        q[i]["ur"] = f32(u - f32(f32(mbf) * invzc))
        q[i]["level_aux"] = o
        q[i]["angle"] = last_angles[i]
        q[i]["observed"] = int(observed[i])
    return q


def pnp_draws(n_corr, draw_rows, seed):
    """Valid draws for PnpIterate / PnpRansac: [C, draw_rows, 4] int32 from numpy.random.default_rng(seed), draw k of
    candidate c uniform in [0, n_corr[c] - 1 - k], which is what DUtils::Random::RandomInt(0, size - 1) ranges over for the
    shrinking list (src/PnPsolver.cc:193).  Candidates with fewer than four correspondences get zeros (never read)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(n_corr), draw_rows, 4), np.int32)
    for c, N in enumerate(n_corr):
        if N >= 4:
            for k in range(4):
                out[c, :, k] = rng.integers(0, N - k, draw_rows)
    return out
