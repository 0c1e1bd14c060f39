// C++ host-side mirror of ORB_SLAM2::PnPsolver (include/PnPsolver.h) above orbhip_pnp_ransac of orbhip.h, for one candidate
// key frame.  Header-only, no OpenCV: the frame is its undistorted key points, the map the arrays of orbhip_pnp_map (host
// pointers), matrices are float arrays.  The reference draws its samples with DUtils::Random; here the draws are data the
// caller sets (SetDraws), row `it` serving iteration number `it`.
#pragma once
#include <cstdint>
#include <vector>

#include "ORBextractor.hpp"

namespace orbhip {

class PnPsolver {
public:
    // PnPsolver(const Frame &F, const vector<MapPoint*> &vpMapPointMatches): F is mvKeysUn (x, y and octave are read) with the
    // camera, vpMapPointMatches one entry per key point: point indices (ORBHIP_PNP_MATCH_POINTS), negative = none.  The map
    // must outlive the solver.  The correspondences are rebuilt from it by every iterate call (they are a function of the
    // inputs), the RANSAC state (mnIterations, mnBestInliers, mvbBestInliers, mBestTcw) is kept here.
    PnPsolver(ORBmatcher &matcher, const orbhip_camera &cam, const std::vector<orbhip_keypoint> &keysUn, int np, int pcap,
              const orbhip_pnp_map &map, const std::vector<int32_t> &vpMapPointMatches, const std::vector<float> &levelSigma2)
        : m_(matcher.handle()), cam_(cam), keys_(keysUn), np_(np), pcap_(pcap), map_(map), sigma2_(levelSigma2),
          cap_((int)(keysUn.empty() ? 1 : keysUn.size())), matches_((size_t)cap_, -1), inliers_((size_t)cap_, 0),
          best_((size_t)cap_, 0)
    {
        for (size_t i = 0; i < vpMapPointMatches.size() && i < matches_.size(); ++i) matches_[i] = vpMapPointMatches[i];
        for (int i = 0; i < 12; ++i) tcw_[i] = bestTcw_[i] = 0.f;
        for (int i = 0; i < 8; ++i) report_[i] = 0;
        SetRansacParameters();
    }

    // void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
    //                          float epsilon = 0.4, float th2 = 5.991); restarts the solver.  minSet other than 4 is refused
    // by the library when iterate runs.
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4f, float th2 = 5.991f)
    {
        prm_.prob = probability; prm_.min_inliers = minInliers; prm_.max_its = maxIterations; prm_.min_set = minSet;
        prm_.epsilon = epsilon; prm_.th2 = th2;
        state_[0] = 0; state_[1] = 0;
    }
    // [rows][4] int32, draw k in [0, N-1-k]; checked by the library against N.  A call runs the iterations mnIterations ...
    // max(limit, mnIterations + nIterations) - 1 and needs that many rows.
    void SetDraws(const std::vector<int32_t> &draws) { draws_ = draws; }

    // cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): true where the reference
    // returns a non-empty matrix (a refined pose, or the unrefined best at the limit); read it with GetTcw.  vbInliers has
    // one entry per key point of the frame, and is empty where nothing is returned.
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        const int n = (int)keys_.size();
        check(orbhip_pnp_ransac(m_, 1, keys_.data(), n, cap_, matches_.data(), ORBHIP_PNP_MATCH_POINTS, nullptr, 0, np_, pcap_, &map_,
                                &cam_, sigma2_.data(), &prm_, draws_.data(), (int)(draws_.size() / 4), nIterations, state_, best_.data(),
                                bestTcw_, tcw_, inliers_.data(), report_), "orbhip_pnp_ransac");
        const bool got = report_[0] == ORBHIP_PNP_REFINED || report_[0] == ORBHIP_PNP_BEST;
        vbInliers.clear();
        if (got) {
            vbInliers.assign((size_t)n, false);
            for (int i = 0; i < n; ++i) vbInliers[(size_t)i] = inliers_[(size_t)i] != 0;
        }
        bNoMore = report_[0] != ORBHIP_PNP_REFINED;
        nInliers = report_[6];
        return got;
    }
    // cv::Mat find(vector<bool> &vbInliers, int &nInliers) is iterate(mRansacMaxIts) (:159-163)
    bool find(std::vector<bool> &vbInliers, int &nInliers)
    {
        bool bFlag;
        return iterate(prm_.max_its, bFlag, vbInliers, nInliers);
    }

    // [Rcw | tcw], 12 floats row-major, of the last iterate call that returned one
    const float *GetTcw() const { return tcw_; }
    // {status, N, limit, mnIterations, mnBestInliers, returned iteration or -1, nInliers, adjusted min inliers}
    const int32_t *Report() const { return report_; }

private:
    orbhip_matcher *m_;
    orbhip_camera cam_;
    std::vector<orbhip_keypoint> keys_;
    int np_, pcap_;
    orbhip_pnp_map map_;
    std::vector<float> sigma2_;
    int cap_;
    std::vector<int32_t> matches_, draws_;
    std::vector<uint8_t> inliers_, best_;
    orbhip_pnp_params prm_;
    int32_t state_[2], report_[8];
    float tcw_[12], bestTcw_[12];
};

}  // namespace orbhip
