// C++ host-side mirror of ORB_SLAM2::Optimizer (include/Optimizer.h) above orbhip_pose_optimization of orbhip.h: the one
// function of it the library has, PoseOptimization.  Header-only, no OpenCV and no g2o: a frame is the arrays the
// reference's Frame holds (mvKeysUn, mvuRight, mvpMapPoints as indices into the map arrays, mvbOutlier, mTcw).
#pragma once
#include <cstdint>
#include <vector>

#include "ORBextractor.hpp"

namespace orbhip {

// What PoseOptimization reads and writes of a Frame.  mvpMapPoints holds indices into `world` / `pointFlags` (-1 = none).
struct PoseFrame {
    std::vector<orbhip_keypoint> mvKeysUn;
    std::vector<float> mvuRight;            // empty: a monocular frame
    std::vector<int32_t> mvpMapPoints;
    std::vector<uint8_t> mvbOutlier;
    float mTcw[12];                         // [Rcw | tcw], row-major
};

class Optimizer {
public:
    // int Optimizer::PoseOptimization(Frame *pFrame): returns nInitialCorrespondences - nBad (0 with fewer than three edges).
    // world [np][3] = mWorldPos, pointFlags [np] (ORBHIP_POINT_OBSERVED is read by the two epilogue modes), invLevelSigma2 =
    // mvInvLevelSigma2.  mode / flags: ORBHIP_POSEOPT_PLAIN is the function alone; DISCARD and LOCAL_MAP also run the loop
    // of Tracking that follows the call (src/Tracking.cc:900-919, :941-963), `discarded` then receives, per slot, the point
    // the loop took out (-1: none).  report [8] as orbhip_pose_optimization_device lists it.
    static int PoseOptimization(ORBmatcher &matcher, const orbhip_camera &cam, PoseFrame &F, const std::vector<float> &world,
                                const std::vector<uint8_t> &pointFlags, const std::vector<float> &invLevelSigma2,
                                int mode = ORBHIP_POSEOPT_PLAIN, int flags = 0, std::vector<int32_t> *discarded = nullptr,
                                int32_t *report = nullptr)
    {
        const int32_t n = (int32_t)F.mvKeysUn.size();
        const int cap = n > 0 ? n : 1, np = (int)(world.size() / 3);
        std::vector<orbhip_keypoint> keys(F.mvKeysUn);
        keys.resize((size_t)cap);
        F.mvpMapPoints.resize((size_t)cap, -1);
        F.mvbOutlier.resize((size_t)cap, 0);
        std::vector<float> ur(F.mvuRight);
        if (!ur.empty()) ur.resize((size_t)cap, -1.f);
        std::vector<int32_t> dis((size_t)cap, -1);
        int32_t rep[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // the entry stages pcap points: an empty map becomes one unused point, and the flags must cover the map
        if (!pointFlags.empty() && pointFlags.size() < (size_t)np)
            throw Error(ORBHIP_E_ARG, "Optimizer::PoseOptimization (pointFlags is shorter than world)");
        const std::vector<float> none(3, 0.f);
        const std::vector<uint8_t> noFlags(1, 0);
        const float *w = np > 0 ? world.data() : none.data();
        const uint8_t *pf = pointFlags.empty() ? nullptr : (np > 0 ? pointFlags.data() : noFlags.data());
        check(orbhip_pose_optimization(matcher.handle(), 1, keys.data(), &n, cap, ur.empty() ? nullptr : ur.data(), w,
                                       pf, 1, np > 0 ? np : 1, nullptr, &cam,
                                       invLevelSigma2.data(), mode, flags, F.mTcw, F.mvpMapPoints.data(), F.mvbOutlier.data(),
                                       dis.data(), rep), "orbhip_pose_optimization");
        F.mvpMapPoints.resize((size_t)n);
        F.mvbOutlier.resize((size_t)n);
        if (discarded) { dis.resize((size_t)n); *discarded = dis; }
        if (report) for (int i = 0; i < 8; ++i) report[i] = rep[i];
        return rep[3];
    }

    // The same over device arrays for `frames` frames at once, asynchronous on the matcher's stream: the arguments of
    // orbhip_pose_optimization_device, which see.
    static void PoseOptimizationDevice(ORBmatcher &matcher, int frames, const void *d_kps, const void *d_n, int cap, const void *d_u_right,
                                       const void *d_world, const void *d_point_flags, int wrows, int pcap, const void *d_world_row,
                                       const orbhip_camera &cam, const std::vector<float> &invLevelSigma2, int mode, int flags,
                                       void *d_Tcw, void *d_frame_point, void *d_outlier, void *d_discarded, void *d_report)
    {
        check(orbhip_pose_optimization_device(matcher.handle(), frames, d_kps, d_n, cap, d_u_right, d_world, d_point_flags, wrows, pcap,
                                              d_world_row, &cam, invLevelSigma2.data(), mode, flags, d_Tcw, d_frame_point, d_outlier,
                                              d_discarded, d_report), "orbhip_pose_optimization_device");
    }
};

}  // namespace orbhip
