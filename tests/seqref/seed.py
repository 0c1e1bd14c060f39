"""Sequential restatement of the stereo / RGB-D map-point seeding of the reference, loop for loop from the cited lines:

  Tracking::UpdateLastFrame      src/Tracking.cc:812-864     (depth sort, stop rule, bCreateNew)
  Tracking::CreateNewKeyFrame    src/Tracking.cc:1073-1133   (the same loop)
  Tracking::StereoInitialization src/Tracking.cc:523-538     (every keypoint with z > 0)
  Frame::UnprojectStereo         src/Frame.cc:666-680        (invfx = 1.0f / fx: src/Frame.cc:108-109)
  Frame::UpdatePoseMatrices      src/Frame.cc:258-264        (mRwc = mRcw.t(), mOw = -mRcw.t() * mtcw)
  Tracking::NeedNewKeyFrame      src/Tracking.cc:1001-1018   (close-point counts)
  Tracking::Tracking             src/Tracking.cc:134-138     (mThDepth)

Plain Python over numpy scalars: every float operation is one np.float32 operation, in the order DESIGN.md section 3
states for the cv::Mat products (per row ((r0*x + r1*y) + r2*z) + t).  Loads no shared library and imports neither the
package nor the oracle."""
import numpy as np

f32 = np.float32
POINT_PRESENT, POINT_OBSERVED = 1, 2
SEED_ALL, SEED_CLOSEST = 0, 1


def th_depth(bf, th_depth_setting, fx):
    """mThDepth = mbf*(float)fSettings["ThDepth"]/fx with float mbf and fx (src/Tracking.cc:136)."""
    return f32(f32(f32(bf) * f32(th_depth_setting)) / f32(fx))


def pose_matrices(Tcw):
    """(mRwc, mOw) of Frame::UpdatePoseMatrices from the top three rows of mTcw."""
    T = np.asarray(Tcw, f32).reshape(-1)[:12].reshape(3, 4)
    Rwc = [[T[c, r] for c in range(3)] for r in range(3)]            # mRcw.t()
    with np.errstate(all="ignore"):
        Ow = [-f32(f32(f32(T[0, i] * T[0, 3]) + f32(T[1, i] * T[1, 3])) + f32(T[2, i] * T[2, 3])) for i in range(3)]
    return Rwc, Ow


def unproject_stereo(u, v, z, K, Tcw, pose=None):
    """Frame::UnprojectStereo for one keypoint with z > 0.  K = (fx, fy, cx, cy); pose = pose_matrices(Tcw) where the
    caller has it already.  Returns three np.float32."""
    fx, fy, cx, cy = (f32(a) for a in K)
    u, v, z = f32(u), f32(v), f32(z)
    Rwc, Ow = pose if pose is not None else pose_matrices(Tcw)
    with np.errstate(all="ignore"):
        invfx = f32(1.0) / fx
        invfy = f32(1.0) / fy
        x = f32(f32(f32(u - cx) * z) * invfx)
        y = f32(f32(f32(v - cy) * z) * invfy)
        return [f32(f32(f32(f32(Rwc[r][0] * x) + f32(Rwc[r][1] * y)) + f32(Rwc[r][2] * z)) + Ow[r]) for r in range(3)]


def seed_stereo_points(K, Tcw, keys_xy, depth, th, mode, created_flags, world, flags):
    """keys_xy [n][2] (mvKeysUn pt), depth [n] (mvDepth), world [n][3], flags [n] (POINT_* bits of the slot's map point).
    Returns (world, flags, order, created, (n_valid, n_visited, n_created)); world / flags are updated copies."""
    depth = np.asarray(depth, f32)
    n = len(depth)
    world = np.array(world, f32).reshape(-1, 3).copy()
    flags = np.array(flags, np.uint8).copy()
    created = np.zeros(n, np.uint8)
    th = f32(th)
    vDepthIdx = []
    for i in range(n):
        z = depth[i]
        if z > 0:
            vDepthIdx.append((z, i))
    order = []
    n_created = 0
    pose = pose_matrices(Tcw)                 # Frame::UpdatePoseMatrices ran when the pose was set

    def create(i, z):
        X = unproject_stereo(keys_xy[i][0], keys_xy[i][1], z, K, Tcw, pose)
        world[i, 0], world[i, 1], world[i, 2] = X
        flags[i] = created_flags
        created[i] = 1

    if mode == SEED_ALL:                      # src/Tracking.cc:523-538
        for z, i in vDepthIdx:
            order.append(i)
            create(i, z)
            n_created += 1
        return world, flags, np.array(order, np.int32), created, (len(vDepthIdx), len(order), n_created)

    if not vDepthIdx:
        return world, flags, np.zeros(0, np.int32), created, (0, 0, 0)
    vDepthIdx = sorted(vDepthIdx)
    nPoints = 0
    for j in range(len(vDepthIdx)):
        i = vDepthIdx[j][1]
        order.append(i)
        bCreateNew = False
        if not (flags[i] & POINT_PRESENT):            # !pMP
            bCreateNew = True
        elif not (flags[i] & POINT_OBSERVED):         # pMP->Observations() < 1
            bCreateNew = True
        if bCreateNew:
            create(i, vDepthIdx[j][0])
            n_created += 1
            nPoints += 1
        else:
            nPoints += 1
        if vDepthIdx[j][0] > th and nPoints > 100:
            break
    return world, flags, np.array(order, np.int32), created, (len(vDepthIdx), len(order), n_created)


def count_close_points(depth, flags, th):
    """(nTrackedClose, nNonTrackedClose), src/Tracking.cc:1006-1015; POINT_PRESENT = map point && !outlier."""
    depth = np.asarray(depth, f32)
    th = f32(th)
    nTrackedClose = nNonTrackedClose = 0
    for i in range(len(depth)):
        if depth[i] > 0 and depth[i] < th:
            if flags[i] & POINT_PRESENT:
                nTrackedClose += 1
            else:
                nNonTrackedClose += 1
    return nTrackedClose, nNonTrackedClose
