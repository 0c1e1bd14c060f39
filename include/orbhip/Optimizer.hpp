// C++ host-side mirror of ORB_SLAM2::Optimizer (include/Optimizer.h) above orbhip_pose_optimization, orbhip_optimize_sim3,
// orbhip_local_bundle_adjustment, orbhip_optimize_essential_graph and orbhip_global_bundle_adjustment of orbhip.h: all of its
// functions, PoseOptimization, OptimizeSim3, LocalBundleAdjustment (whose key frames and map points are the tables of
// orbhip_lba_tables), OptimizeEssentialGraph (the tables of orbhip_eg_tables), BundleAdjustment and GlobalBundleAdjustemnt (the
// tables of orbhip_gba_tables), and ApplyGlobalBA, the map update LoopClosing runs after the last.  Header-only,
// no OpenCV and no g2o: a frame is the arrays the reference's Frame holds (mvKeysUn, mvuRight, mvpMapPoints as indices
// into the map arrays, mvbOutlier, mTcw); key frames and map points of OptimizeSim3 are the tables of orbhip_sim3_tables.
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

// g2o::Sim3 as OptimizeSim3 takes and leaves it: the quaternion as g2o keeps it (x, y, z, w; not normalised), t, s.
struct Sim3 {
    double r[4], t[3], s;
};

// What LocalBundleAdjustment leaves besides the poses and points it writes into the tables: the three lists in push_back
// order (key-frame rows, point indices), vToErase as (key-frame row, key-point index, point) triples in the reference's
// order, and the report of orbhip_local_bundle_adjustment_device.
struct LocalBA {
    std::vector<int32_t> lLocalKeyFrames, lFixedCameras, lLocalMapPoints, vToErase;
    int32_t report[16];
};

// What OptimizeEssentialGraph leaves besides the poses and points it writes into the tables: the present points in index
// order (the list UpdateNormalAndDepth is then run over), vScw and vCorrectedSwc per bank row as Sim3 records (rows that are
// bad keep Sim3{{0, 0, 0, 1}, {0, 0, 0}, 1}), and the report of orbhip_optimize_essential_graph_device.
struct EssentialGraph {
    std::vector<int32_t> vpCorrectedPoints;
    std::vector<Sim3> vScw, vCorrectedSwc;
    int32_t report[16];
};

// What BundleAdjustment leaves besides the poses and points it writes into the tables when nLoopKF == 0: the written points
// in list order (vpUpdatedPoints); when nLoopKF != 0: mTcwGBA / mPosGBA per bank row / point with their marks
// (mnBAGlobalForKF == nLoopKF); and the report of orbhip_global_bundle_adjustment_device.
struct GlobalBA {
    std::vector<float> TcwGBA, posGBA;      // [rows][12], [pcap][3]
    std::vector<uint8_t> kfMark, ptMark;    // [rows], [pcap]
    std::vector<int32_t> vpUpdatedPoints;
    int32_t report[16];
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

    // int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches1, g2o::Sim3 &g2oS12, const float
    // th2, const bool bFixScale): pKF1 is bank row `cur`, pKF2 bank row `kf` of the tables (host pointers), vpMatches1 one
    // entry per slot of pKF1 (point indices or slots of pKF2, see matchForm; negative = none), nulled entries become -1.
    // sim3 [16] is what Sim3Solver leaves (GetEstimatedRotation is its start: R (9), t (3), s): the start, as
    // g2o::Sim3(toMatrix3d(R), toVector3d(t), s).  g2oS12 receives the estimate (the start on the early return).  Scw [12],
    // if given, receives Converter::toCvMat(g2oS12 * Sim3(R2w, t2w, 1)) unless the function returned early.  report [8] as
    // orbhip_optimize_sim3_device lists it.  Returns nIn.
    static int OptimizeSim3(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap,
                            const orbhip_sim3_tables &tables, int cur, int kf, std::vector<int32_t> &vpMatches1, int matchForm,
                            const std::vector<float> &invLevelSigma2, const float *sim3, Sim3 &g2oS12, float th2, bool bFixScale,
                            float *Scw = nullptr, int32_t *report = nullptr)
    {
        std::vector<int32_t> matched((size_t)(cap > 0 ? cap : 1), -1);
        for (size_t i = 0; i < vpMatches1.size() && i < matched.size(); ++i) matched[i] = vpMatches1[i];
        const int32_t row = kf;
        double S12[8] = {0, 0, 0, 1, 0, 0, 0, 1};
        int32_t rep[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(orbhip_optimize_sim3(matcher.handle(), 1, cur, &row, &cam, rows, cap, np, pcap, &tables, matchForm, invLevelSigma2.data(),
                                   th2, bFixScale ? 1 : 0, nullptr, matched.data(), sim3, S12, Scw, rep), "orbhip_optimize_sim3");
        for (size_t i = 0; i < vpMatches1.size() && i < matched.size(); ++i) vpMatches1[i] = matched[i];
        for (int i = 0; i < 4; ++i) g2oS12.r[i] = S12[i];
        for (int i = 0; i < 3; ++i) g2oS12.t[i] = S12[4 + i];
        g2oS12.s = S12[7];
        if (report) for (int i = 0; i < 8; ++i) report[i] = rep[i];
        return rep[3];
    }

    // The same over device arrays for C candidates at once, asynchronous on the matcher's stream: the arguments of
    // orbhip_optimize_sim3_device, which see.
    static void OptimizeSim3Device(ORBmatcher &matcher, int C, int cur, const void *d_kf_index, const orbhip_camera &cam, int rows, int cap,
                                   int np, int pcap, const orbhip_sim3_tables &tables, int matchForm,
                                   const std::vector<float> &invLevelSigma2, float th2, bool bFixScale, const void *d_select,
                                   void *d_matched12, const void *d_sim3, void *d_S12, void *d_Scw, void *d_report)
    {
        check(orbhip_optimize_sim3_device(matcher.handle(), C, cur, d_kf_index, &cam, rows, cap, np, pcap, &tables, matchForm,
                                          invLevelSigma2.data(), th2, bFixScale ? 1 : 0, d_select, d_matched12, d_sim3, d_S12, d_Scw,
                                          d_report), "orbhip_optimize_sim3_device");
    }

    // void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap): pKF is bank row `cur` of the tables
    // (host pointers; Tcw and world are updated in place), id0Row the row whose mnId is 0 (or -1), pbStopFlag may be null.
    // `out` receives lLocalKeyFrames, lFixedCameras, lLocalMapPoints and vToErase; applying vToErase (:748-757) and
    // UpdateNormalAndDepth of the local points (:776) stay with the caller.  Returns the status (ORBHIP_LBA_*): on
    // ORBHIP_LBA_STOPPED and ORBHIP_LBA_CAPACITY nothing but out.report is written and the lists are empty.
    static int LocalBundleAdjustment(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap,
                                     const orbhip_lba_tables &tables, int cur, int id0Row, const std::vector<float> &invLevelSigma2,
                                     int maxPoints, int maxEdges, const bool *pbStopFlag, LocalBA &out)
    {
        std::vector<int32_t> lkf((size_t)(rows > 0 ? rows : 1), -1), fkf(lkf), lpt((size_t)(maxPoints > 0 ? maxPoints : 1), -1),
            er((size_t)(maxEdges > 0 ? maxEdges : 1) * 3, -1);
        for (int i = 0; i < 16; ++i) out.report[i] = 0;
        const uint8_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
        orbhip_lba_out o;
        o.local_kf = lkf.data(); o.fixed_kf = fkf.data(); o.local_point = lpt.data(); o.erase = er.data(); o.report = out.report;
        check(orbhip_local_bundle_adjustment(matcher.handle(), cur, id0Row, &cam, rows, cap, np, pcap, &tables, invLevelSigma2.data(),
                                             maxPoints, maxEdges, pbStopFlag ? &stop : nullptr, &o), "orbhip_local_bundle_adjustment");
        const bool wrote = out.report[0] == ORBHIP_LBA_OK || out.report[0] == ORBHIP_LBA_ONE_ROUND;
        out.lLocalKeyFrames.assign(lkf.begin(), lkf.begin() + (wrote ? out.report[1] : 0));
        out.lFixedCameras.assign(fkf.begin(), fkf.begin() + (wrote ? out.report[2] : 0));
        out.lLocalMapPoints.assign(lpt.begin(), lpt.begin() + (wrote ? out.report[3] : 0));
        out.vToErase.assign(er.begin(), er.begin() + (wrote ? 3 * (size_t)out.report[7] : 0));
        return out.report[0];
    }

    // The same over device arrays, asynchronous on the matcher's stream, no host synchronisation: the arguments of
    // orbhip_local_bundle_adjustment_device, which see.
    static void LocalBundleAdjustmentDevice(ORBmatcher &matcher, int cur, int id0Row, const orbhip_camera &cam, int rows, int cap, int np,
                                            int pcap, const orbhip_lba_tables &tables, const std::vector<float> &invLevelSigma2,
                                            int maxPoints, int maxEdges, const void *d_stop, const orbhip_lba_out &out)
    {
        check(orbhip_local_bundle_adjustment_device(matcher.handle(), cur, id0Row, &cam, rows, cap, np, pcap, &tables,
                                                    invLevelSigma2.data(), maxPoints, maxEdges, d_stop, &out),
              "orbhip_local_bundle_adjustment_device");
    }

    // void Optimizer::OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const KeyFrameAndPose &NonCorrectedSim3,
    // const KeyFrameAndPose &CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>> &LoopConnections, const bool &bFixScale): the map
    // is the tables (host pointers; Tcw and world are updated in place), pLoopKF / pCurKF are bank rows loopRow / cur, the two
    // KeyFrameAndPose maps are tables.corrected / non_corrected with their marks, LoopConnections is tables.lc_start / lc_kf.
    // UpdateNormalAndDepth of out.vpCorrectedPoints (:1042) stays with the caller.  Returns the status (ORBHIP_EG_*): on
    // ORBHIP_EG_CAPACITY nothing but out.report is written and the lists are empty.
    static int OptimizeEssentialGraph(ORBmatcher &matcher, int rows, int pcap, const orbhip_eg_tables &tables, int loopRow, int cur,
                                      bool bFixScale, int maxEdges, EssentialGraph &out)
    {
        const size_t R = (size_t)(rows > 0 ? rows : 1), P = (size_t)(pcap > 0 ? pcap : 1);
        std::vector<int32_t> pl(P, -1);
        std::vector<double> scw(R * 8, 0.0), swc(R * 8, 0.0);
        for (size_t r = 0; r < R; ++r) scw[r * 8 + 3] = scw[r * 8 + 7] = swc[r * 8 + 3] = swc[r * 8 + 7] = 1.0;
        for (int i = 0; i < 16; ++i) out.report[i] = 0;
        orbhip_eg_out o;
        o.point_list = pl.data(); o.Scw = scw.data(); o.Swc = swc.data(); o.report = out.report;
        check(orbhip_optimize_essential_graph(matcher.handle(), cur, loopRow, rows, pcap, &tables, bFixScale ? 1 : 0, maxEdges, &o),
              "orbhip_optimize_essential_graph");
        const bool wrote = out.report[0] != ORBHIP_EG_CAPACITY;
        out.vpCorrectedPoints.assign(pl.begin(), pl.begin() + (wrote ? out.report[11] : 0));
        out.vScw.assign((size_t)(rows > 0 ? rows : 0), Sim3());
        out.vCorrectedSwc = out.vScw;
        for (size_t r = 0; r < out.vScw.size(); ++r)
            for (int k = 0; k < 2; ++k) {
                const double *src = (k ? swc.data() : scw.data()) + r * 8;
                Sim3 &dst = k ? out.vCorrectedSwc[r] : out.vScw[r];
                for (int i = 0; i < 4; ++i) dst.r[i] = src[i];
                for (int i = 0; i < 3; ++i) dst.t[i] = src[4 + i];
                dst.s = src[7];
            }
        return out.report[0];
    }

    // The same over device arrays: the arguments of orbhip_optimize_essential_graph_device, which see.  The call synchronises the
    // matcher's stream once per Levenberg-Marquardt trial.
    static void OptimizeEssentialGraphDevice(ORBmatcher &matcher, int cur, int loopRow, int rows, int pcap, const orbhip_eg_tables &tables,
                                             bool bFixScale, int maxEdges, const orbhip_eg_out &out)
    {
        check(orbhip_optimize_essential_graph_device(matcher.handle(), cur, loopRow, rows, pcap, &tables, bFixScale ? 1 : 0, maxEdges,
                                                     &out), "orbhip_optimize_essential_graph_device");
    }

    // void Optimizer::BundleAdjustment(const vector<KeyFrame*> &vpKFs, const vector<MapPoint*> &vpMP, int nIterations, bool
    // *pbStopFlag, const unsigned long nLoopKF, const bool bRobust): the map is the tables (host pointers), vpKFs / vpMP are bank
    // rows / point indices (a null pointer: all of them, ascending), pbStopFlag may be null.  nLoopKF == 0 writes tables.Tcw and
    // tables.world and fills out.vpUpdatedPoints (UpdateNormalAndDepth of them, :227, stays with the caller); nLoopKF != 0 fills
    // out.TcwGBA / posGBA and the marks (mnBAGlobalForKF == nLoopKF), which ApplyGlobalBA takes.  Returns the status
    // (ORBHIP_GBA_*): on ORBHIP_GBA_CAPACITY nothing but out.report is written.
    static int BundleAdjustment(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap,
                                const orbhip_gba_tables &tables, const std::vector<int32_t> *vpKFs, const std::vector<int32_t> *vpMP,
                                const std::vector<float> &invLevelSigma2, int nIterations, const bool *pbStopFlag, unsigned long nLoopKF,
                                bool bRobust, int maxPoints, int maxEdges, GlobalBA &out)
    {
        const size_t R = (size_t)(rows > 0 ? rows : 1), P = (size_t)(pcap > 0 ? pcap : 1);
        out.TcwGBA.assign(R * 12, 0.f); out.posGBA.assign(P * 3, 0.f); out.kfMark.assign(R, 0); out.ptMark.assign(P, 0);
        std::vector<int32_t> pl((size_t)(maxPoints > 0 ? maxPoints : 1), -1);
        for (int i = 0; i < 16; ++i) out.report[i] = 0;
        const uint8_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
        const int32_t none = 0;
        orbhip_gba_out o;
        o.TcwGBA = out.TcwGBA.data(); o.posGBA = out.posGBA.data(); o.kf_mark = out.kfMark.data(); o.pt_mark = out.ptMark.data();
        o.point_list = pl.data(); o.report = out.report;
        check(orbhip_global_bundle_adjustment(matcher.handle(), &cam, rows, cap, np, pcap, &tables, invLevelSigma2.data(),
                                              vpKFs ? (vpKFs->empty() ? &none : vpKFs->data()) : nullptr, vpKFs ? (int)vpKFs->size() : 0,
                                              vpMP ? (vpMP->empty() ? &none : vpMP->data()) : nullptr, vpMP ? (int)vpMP->size() : 0,
                                              nIterations, bRobust ? 1 : 0, nLoopKF == 0 ? ORBHIP_GBA_IN_PLACE : ORBHIP_GBA_STAGED,
                                              maxPoints, maxEdges, pbStopFlag ? &stop : nullptr, &o), "orbhip_global_bundle_adjustment");
        out.vpUpdatedPoints.assign(pl.begin(), pl.begin() + (out.report[0] != ORBHIP_GBA_CAPACITY ? out.report[12] : 0));
        return out.report[0];
    }

    // void Optimizer::GlobalBundleAdjustemnt(Map *pMap, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool
    // bRobust) -- the reference's spelling: BundleAdjustment over every key frame and every map point of the tables.
    static int GlobalBundleAdjustemnt(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap,
                                      const orbhip_gba_tables &tables, const std::vector<float> &invLevelSigma2, int nIterations,
                                      const bool *pbStopFlag, unsigned long nLoopKF, bool bRobust, int maxPoints, int maxEdges,
                                      GlobalBA &out)
    {
        return BundleAdjustment(matcher, cam, rows, cap, np, pcap, tables, nullptr, nullptr, invLevelSigma2, nIterations, pbStopFlag,
                                nLoopKF, bRobust, maxPoints, maxEdges, out);
    }

    // The same over device arrays: the arguments of orbhip_global_bundle_adjustment_device, which see.  The call synchronises the
    // matcher's stream once per Levenberg-Marquardt trial.
    static void BundleAdjustmentDevice(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap,
                                       const orbhip_gba_tables &tables, const std::vector<float> &invLevelSigma2, const void *d_kf_list,
                                       int nkf, const void *d_pt_list, int npt, int nIterations, bool bRobust, int mode, int maxPoints,
                                       int maxEdges, const void *d_stop, const orbhip_gba_out &out)
    {
        check(orbhip_global_bundle_adjustment_device(matcher.handle(), &cam, rows, cap, np, pcap, &tables, invLevelSigma2.data(), d_kf_list,
                                                     nkf, d_pt_list, npt, nIterations, bRobust ? 1 : 0, mode, maxPoints, maxEdges, d_stop,
                                                     &out), "orbhip_global_bundle_adjustment_device");
    }
    static void GlobalBundleAdjustemntDevice(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap,
                                             const orbhip_gba_tables &tables, const std::vector<float> &invLevelSigma2, int nIterations,
                                             bool bRobust, int mode, int maxPoints, int maxEdges, const void *d_stop,
                                             const orbhip_gba_out &out)
    {
        BundleAdjustmentDevice(matcher, cam, rows, cap, np, pcap, tables, invLevelSigma2, nullptr, 0, nullptr, 0, nIterations, bRobust, mode,
                               maxPoints, maxEdges, d_stop, out);
    }

    // The map update of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:676-737) over host arrays: the arguments of
    // orbhip_apply_global_ba, which see; a.report receives the eight counts.
    static void ApplyGlobalBA(ORBmatcher &matcher, int nOrigins, int rows, int pcap, const orbhip_gba_apply &a)
    {
        check(orbhip_apply_global_ba(matcher.handle(), nOrigins, rows, pcap, &a), "orbhip_apply_global_ba");
    }
    // The same over device arrays, asynchronous on the matcher's stream, two launches.
    static void ApplyGlobalBADevice(ORBmatcher &matcher, int nOrigins, int rows, int pcap, const orbhip_gba_apply &a)
    {
        check(orbhip_apply_global_ba_device(matcher.handle(), nOrigins, rows, pcap, &a), "orbhip_apply_global_ba_device");
    }
};

}  // namespace orbhip
