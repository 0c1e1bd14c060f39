// C++ host-side mirror of ORB_SLAM2::Sim3Solver (include/Sim3Solver.h) above orbhip_sim3_ransac of orbhip.h, for one
// candidate key frame.  Header-only, no OpenCV: key frames and map points are the tables of orbhip_sim3_tables (host
// pointers), matrices are float arrays.  The reference draws its samples with rand(); here the draws are data the caller
// sets (SetDraws), row `it` serving iteration number `it`.
#pragma once
#include <cstdint>
#include <vector>

#include "ORBextractor.hpp"

namespace orbhip {

class Sim3Solver {
public:
    // Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const vector<MapPoint*> &vpMatched12, const bool bFixScale): pKF1 is bank row
    // `cur`, pKF2 bank row `kf`, vpMatched12 one entry per slot of pKF1 (point indices or slots of pKF2, see matchForm;
    // negative = none).  The tables must outlive the solver.  The correspondences are rebuilt from them by every iterate
    // call (they are a function of the tables), the RANSAC state is kept here.
    Sim3Solver(ORBmatcher &matcher, const orbhip_camera &cam, int rows, int cap, int np, int pcap, const orbhip_sim3_tables &tables, int cur,
               int kf, const std::vector<int32_t> &vpMatched12, int matchForm, const std::vector<float> &levelSigma2, bool bFixScale)
        : m_(matcher.handle()), cam_(cam), rows_(rows), cap_(cap), np_(np), pcap_(pcap), tables_(tables), cur_(cur), kf_(kf),
          matchForm_(matchForm), sigma2_(levelSigma2), fixScale_(bFixScale), matched_((size_t)(cap > 0 ? cap : 1), -1),
          inliers_((size_t)(cap > 0 ? cap : 1), 0)
    {
        for (size_t i = 0; i < vpMatched12.size() && i < matched_.size(); ++i) matched_[i] = vpMatched12[i];
        for (int i = 0; i < 16; ++i) sim3_[i] = 0.f;
        for (int i = 0; i < 8; ++i) report_[i] = 0;
        SetRansacParameters();
    }

    // void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300); restarts the solver
    // (mnIterations = 0, :137).  minInliers below 3 is refused by the library when iterate runs.
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        prob_ = probability; minInliers_ = minInliers; maxIts_ = maxIterations;
        state_[0] = 0; state_[1] = 0;
    }
    // [maxIterations][3] int32, draw k in [0, N-1-k]; checked by the library against the N of the tables
    void SetDraws(const std::vector<int32_t> &draws) { draws_ = draws; }

    // cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): true where the reference
    // returns a non-empty matrix; the estimate is then read with GetEstimated*.  vbInliers has one entry per slot of pKF1.
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        if (draws_.size() < (size_t)maxIts_ * 3) draws_.resize((size_t)maxIts_ * 3, 0);
        check(orbhip_sim3_ransac(m_, 1, cur_, &kf_, &cam_, rows_, cap_, np_, pcap_, &tables_, matched_.data(), matchForm_, sigma2_.data(),
                                 prob_, minInliers_, maxIts_, fixScale_ ? 1 : 0, draws_.data(), nIterations, state_, sim3_, inliers_.data(),
                                 report_), "orbhip_sim3_ransac");
        const int n1 = ((const int32_t *)tables_.n)[cur_];
        vbInliers.assign((size_t)n1, false);
        for (int i = 0; i < n1; ++i) vbInliers[(size_t)i] = inliers_[(size_t)i] != 0;
        bNoMore = report_[0] == ORBHIP_SIM3_NO_MORE || report_[0] == ORBHIP_SIM3_TOO_FEW;
        nInliers = report_[6];
        return report_[0] == ORBHIP_SIM3_RETURNED;
    }
    // cv::Mat find(vector<bool> &vbInliers12, int &nInliers)
    bool find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        return iterate(maxIts_, bFlag, vbInliers12, nInliers);
    }

    // The estimate of the last iterate call that returned one (the reference's mBest* also move on a best-so-far
    // hypothesis that is not returned; the library reports returned ones only).  R12 row-major.
    const float *GetEstimatedRotation() const { return sim3_; }
    const float *GetEstimatedTranslation() const { return sim3_ + 9; }
    float GetEstimatedScale() const { return sim3_[12]; }
    // {status, N, limit, mnIterations, mnBestInliers, returned iteration or -1, nInliers, 0} of the last iterate call
    const int32_t *Report() const { return report_; }

private:
    orbhip_matcher *m_;
    orbhip_camera cam_;
    int rows_, cap_, np_, pcap_;
    orbhip_sim3_tables tables_;
    int cur_;
    int32_t kf_;
    int matchForm_;
    std::vector<float> sigma2_;
    bool fixScale_;
    std::vector<int32_t> matched_, draws_;
    std::vector<uint8_t> inliers_;
    double prob_;
    int minInliers_, maxIts_;
    int32_t state_[2], report_[8];
    float sim3_[16];
};

}  // namespace orbhip
