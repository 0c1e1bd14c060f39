// C++ host-side mirror of ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-110) and
// ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:37-103) above the C ABI of orbhip.h.
// Header-only; no OpenCV dependency: images are (pointer, rows, cols, step) views and keypoints
// are orbhip_keypoint PODs, which have the memory layout of cv::KeyPoint.  INTEGRATION.md shows
// the 20-line adapter that gives these classes the reference's cv::InputArray/OutputArray
// signatures inside the ORB-SLAM2 tree.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../orbhip.h"

namespace orbhip {

typedef orbhip_keypoint KeyPoint;

struct ImageView {   // the part of cv::Mat the extractor reads (CV_8UC1)
    const uint8_t *data;
    int rows, cols;
    size_t step;
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
};

struct ColorImageView {   // a CV_8UC3 / CV_8UC4 cv::Mat as Tracking::GrabImage* receives it (src/Tracking.cc:167-260)
    const uint8_t *data;
    int rows, cols, channels;
    size_t step;
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
};

struct Error : std::runtime_error {
    int code;
    Error(int c, const char *where) : std::runtime_error(std::string(where) + ": " + orbhip_last_error()), code(c) {}
};
inline void check(int rc, const char *where) { if (rc != ORBHIP_OK) throw Error(rc, where); }

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    // ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
        : h_(nullptr), nlevels_(nlevels)
    {
        check(orbhip_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, &h_),
              "orbhip_extractor_create");
    }
    ~ORBextractor() { orbhip_extractor_destroy(h_); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;

    // void operator()(InputArray image, InputArray mask, vector<KeyPoint>& keypoints, OutputArray descriptors)
    // `mask` is ignored, as in the reference.  descriptors: keypoints.size() x 32 bytes, row-major.
    void operator()(const ImageView &image, const ImageView * /*mask*/, std::vector<KeyPoint> &keypoints,
                    std::vector<uint8_t> &descriptors)
    {
        keypoints.clear();
        descriptors.clear();
        if (image.empty()) return;   // src/ORBextractor.cc:1046-1047
        int cap = 0;
        check(orbhip_extractor_capacity(h_, image.rows, image.cols, &cap), "orbhip_extractor_capacity");
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(orbhip_extract(h_, image.data, image.rows, image.cols, (int)image.step, keypoints.data(),
                             descriptors.data(), cap, &n), "orbhip_extract");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);   // n == 0: descriptors.release() (:1064-1065)
    }

    // A batch of same-size frames in one call (one ORBextractor::operator() per frame in the reference): frame b starts at
    // images + b * frame_stride.  keypoints[b] / descriptors[b] as operator() fills them.
    void ExtractBatch(const uint8_t *images, int batch, int rows, int cols, size_t step, size_t frame_stride,
                      std::vector<std::vector<KeyPoint> > &keypoints, std::vector<std::vector<uint8_t> > &descriptors)
    {
        keypoints.assign(batch, std::vector<KeyPoint>());
        descriptors.assign(batch, std::vector<uint8_t>());
        if (!images || batch <= 0 || rows <= 0 || cols <= 0) return;
        int cap = 0;
        check(orbhip_extractor_capacity(h_, rows, cols, &cap), "orbhip_extractor_capacity");
        std::vector<KeyPoint> k((size_t)batch * cap);
        std::vector<uint8_t> d((size_t)batch * cap * 32);
        std::vector<int32_t> n(batch, 0);
        check(orbhip_extract_batch(h_, images, batch, rows, cols, (int)step, frame_stride, k.data(), d.data(), cap, n.data()),
              "orbhip_extract_batch");
        for (int b = 0; b < batch; ++b) {
            keypoints[b].assign(k.begin() + (size_t)b * cap, k.begin() + (size_t)b * cap + n[b]);
            descriptors[b].assign(d.begin() + (size_t)b * cap * 32, d.begin() + ((size_t)b * cap + n[b]) * 32);
        }
    }

    // cvtColor(mImGray, mImGray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) (src/Tracking.cc:172-197, 212-225,
    // 242-256; rgb = mbRGB) followed by operator(), in one call: the conversion runs on the device in front of the pyramid.
    void ExtractColor(const ColorImageView &image, bool rgb, std::vector<KeyPoint> &keypoints, std::vector<uint8_t> &descriptors)
    {
        keypoints.clear();
        descriptors.clear();
        if (image.empty()) return;
        int cap = 0;
        check(orbhip_extractor_capacity(h_, image.rows, image.cols, &cap), "orbhip_extractor_capacity");
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(orbhip_extract_color(h_, image.data, image.rows, image.cols, image.channels, rgb ? ORBHIP_COLOR_RGB : ORBHIP_COLOR_BGR,
                                   (int)image.step, keypoints.data(), descriptors.data(), cap, &n), "orbhip_extract_color");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }
    void ExtractColorBatch(const uint8_t *images, int batch, int rows, int cols, int channels, bool rgb, size_t step,
                           size_t frame_stride, std::vector<std::vector<KeyPoint> > &keypoints,
                           std::vector<std::vector<uint8_t> > &descriptors)
    {
        keypoints.assign(batch, std::vector<KeyPoint>());
        descriptors.assign(batch, std::vector<uint8_t>());
        if (!images || batch <= 0 || rows <= 0 || cols <= 0) return;
        int cap = 0;
        check(orbhip_extractor_capacity(h_, rows, cols, &cap), "orbhip_extractor_capacity");
        std::vector<KeyPoint> k((size_t)batch * cap);
        std::vector<uint8_t> d((size_t)batch * cap * 32);
        std::vector<int32_t> n(batch, 0);
        check(orbhip_extract_color_batch(h_, images, batch, rows, cols, channels, rgb ? ORBHIP_COLOR_RGB : ORBHIP_COLOR_BGR, (int)step,
                                         frame_stride, k.data(), d.data(), cap, n.data()), "orbhip_extract_color_batch");
        for (int b = 0; b < batch; ++b) {
            keypoints[b].assign(k.begin() + (size_t)b * cap, k.begin() + (size_t)b * cap + n[b]);
            descriptors[b].assign(d.begin() + (size_t)b * cap * 32, d.begin() + ((size_t)b * cap + n[b]) * 32);
        }
    }
    // the grey weights are data (default: OpenCV 2.4 - 3.3's 4899, 9617, 1868 >> 14)
    void SetGrayWeights(const int32_t wRGB[3], int shift) { check(orbhip_extractor_set_gray_weights(h_, wRGB, shift), "orbhip_extractor_set_gray_weights"); }

    // Stereo rectification (Examples/Stereo/stereo_euroc.cc:96-98, 136-137).  SetRemap installs M1, M2 (CV_32F, dstRows x
    // dstCols) for raw frames of srcRows x srcCols; ExtractRemap is cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) followed
    // by operator() in one call, the remap running on the device in front of the pyramid.  Grey frames only.
    void SetRemap(int dstRows, int dstCols, int srcRows, int srcCols, const float *map1, const float *map2)
    {
        check(orbhip_extractor_set_remap(h_, dstRows, dstCols, srcRows, srcCols, map1, map2), "orbhip_extractor_set_remap");
        remapRows_ = map1 ? dstRows : 0;
        remapCols_ = map1 ? dstCols : 0;
    }
    void ClearRemap() { SetRemap(0, 0, 0, 0, nullptr, nullptr); }
    // the 1024 x 4 bilinear weights are data (NULL: the default table)
    void SetRemapTable(const int32_t *w) { check(orbhip_extractor_set_remap_table(h_, w), "orbhip_extractor_set_remap_table"); }
    void ExtractRemap(const ImageView &image, std::vector<KeyPoint> &keypoints, std::vector<uint8_t> &descriptors)
    {
        keypoints.clear();
        descriptors.clear();
        if (image.empty()) return;
        int cap = 0;
        check(orbhip_extractor_capacity(h_, remapRows_ ? remapRows_ : image.rows, remapCols_ ? remapCols_ : image.cols, &cap),
              "orbhip_extractor_capacity");
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(orbhip_extract_remap(h_, image.data, image.rows, image.cols, 1, (int)image.step, keypoints.data(), descriptors.data(),
                                   cap, &n), "orbhip_extract_remap");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }
    void ExtractRemapBatch(const uint8_t *images, int batch, int rows, int cols, size_t step, size_t frame_stride,
                           std::vector<std::vector<KeyPoint> > &keypoints, std::vector<std::vector<uint8_t> > &descriptors)
    {
        keypoints.assign(batch, std::vector<KeyPoint>());
        descriptors.assign(batch, std::vector<uint8_t>());
        if (!images || batch <= 0 || rows <= 0 || cols <= 0) return;
        int cap = 0;
        check(orbhip_extractor_capacity(h_, remapRows_ ? remapRows_ : rows, remapCols_ ? remapCols_ : cols, &cap),
              "orbhip_extractor_capacity");
        std::vector<KeyPoint> k((size_t)batch * cap);
        std::vector<uint8_t> d((size_t)batch * cap * 32);
        std::vector<int32_t> n(batch, 0);
        check(orbhip_extract_remap_batch(h_, images, batch, rows, cols, 1, (int)step, frame_stride, k.data(), d.data(), cap, n.data()),
              "orbhip_extract_remap_batch");
        for (int b = 0; b < batch; ++b) {
            keypoints[b].assign(k.begin() + (size_t)b * cap, k.begin() + (size_t)b * cap + n[b]);
            descriptors[b].assign(d.begin() + (size_t)b * cap * 32, d.begin() + ((size_t)b * cap + n[b]) * 32);
        }
    }
    // device frames: orbhip_extract_remap_batch_device with the mirror's handle
    void ExtractRemapBatchDevice(const void *dImages, int batch, int rows, int cols, size_t step, size_t frame_stride, void *dKps,
                                 void *dDesc, int cap, void *dN, void *dStatus)
    {
        check(orbhip_extract_remap_batch_device(h_, dImages, batch, rows, cols, 1, (int)step, frame_stride, dKps, dDesc, cap, dN,
                                                dStatus), "orbhip_extract_remap_batch_device");
    }
    // cv::initUndistortRectifyMap(K, D, R, P.rowRange(0,3).colRange(0,3), Size(cols, rows), CV_32F, M1, M2); host code
    static void InitUndistortRectifyMap(const double K[9], const std::vector<double> &D, const double *R, const double P3x3[9], int cols,
                                        int rows, std::vector<float> &map1, std::vector<float> &map2)
    {
        map1.assign((size_t)(rows > 0 ? rows : 0) * (cols > 0 ? cols : 0), 0.f);
        map2 = map1;
        check(orbhip_init_undistort_rectify_map(K, D.data(), (int)D.size(), R, P3x3, cols, rows, map1.data(), map2.data()),
              "orbhip_init_undistort_rectify_map");
    }

    // mvImagePyramid[0] on demand: a monocular Tracking thread never reads it (only Frame::ComputeStereoMatches does)
    void SetLazyLevel0(bool on) { check(orbhip_extractor_set_lazy_level0(h_, on ? 1 : 0), "orbhip_extractor_set_lazy_level0"); }

    // several extractors on several streams: chain a stage (0 pyramid, 1 FAST, 2 octree, 3 descriptors) behind another
    // handle's through hipEvent_t handles (scheduling only, see orbhip_extractor_set_stage_gate)
    void SetStageGate(int stage, void *waitEvent, void *recordEvent)
    {
        check(orbhip_extractor_set_stage_gate(h_, stage, waitEvent, recordEvent), "orbhip_extractor_set_stage_gate");
    }

    int GetLevels() { return nlevels_; }
    float GetScaleFactor() { return tab(0).size() > 1 ? tab(0)[1] : 1.f; }
    std::vector<float> GetScaleFactors() { return tab(0); }
    std::vector<float> GetInverseScaleFactors() { return tab(1); }
    std::vector<float> GetScaleSigmaSquares() { return tab(2); }
    std::vector<float> GetInverseScaleSigmaSquares() { return tab(3); }

    // mvImagePyramid[level] of the last call: host copy of the level (rows x cols, tightly packed)
    std::vector<uint8_t> ImagePyramidLevel(int level, int &rows, int &cols)
    {
        int stride = 0;
        const void *d = nullptr;
        check(orbhip_pyramid_level(h_, 0, level, &rows, &cols, &stride, &d), "orbhip_pyramid_level");
        std::vector<uint8_t> out((size_t)rows * cols);
        check(orbhip_pyramid_level_download(h_, 0, level, 0, out.data(), cols), "orbhip_pyramid_level_download");
        return out;
    }
    orbhip_extractor *handle() { return h_; }

private:
    std::vector<float> tab(int which)
    {
        std::vector<float> t[4];
        for (auto &v : t) v.resize(nlevels_);
        check(orbhip_extractor_tables(h_, t[0].data(), t[1].data(), t[2].data(), t[3].data(), nullptr),
              "orbhip_extractor_tables");
        return t[which];
    }
    orbhip_extractor *h_;
    int nlevels_;
    int remapRows_ = 0, remapCols_ = 0;   // destination size of the installed remap (0: none)
};

class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;

    ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0)
        : m_(nullptr), mfNNratio(nnratio), mbCheckOrientation(checkOri)
    {
        check(orbhip_matcher_create(device, &m_), "orbhip_matcher_create");
    }
    ~ORBmatcher() { orbhip_matcher_destroy(m_); }
    ORBmatcher(const ORBmatcher &) = delete;
    ORBmatcher &operator=(const ORBmatcher &) = delete;
    orbhip_matcher *handle() { return m_; }   // for the classes that work over the same handle (orbhip/Sim3Solver.hpp)

    // static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b): host popcount, same result
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b)
    {
        int d = 0;
        for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
        return d;
    }

    // int SearchForInitialization(Frame &F1, Frame &F2, vector<Point2f> &vbPrevMatched, vector<int> &vnMatches12, int windowSize)
    int SearchForInitialization(const orbhip_frame_view &F1, const orbhip_frame_view &F2, std::vector<float> &vbPrevMatchedXY,
                                std::vector<int> &vnMatches12, int windowSize = 10)
    {
        vnMatches12.assign(F1.n > 0 ? F1.n : 1, -1);
        int n = 0;
        check(orbhip_search_for_initialization(m_, &F1, &F2, vbPrevMatchedXY.data(), vnMatches12.data(), windowSize,
                                               mfNNratio, mbCheckOrientation, &n), "orbhip_search_for_initialization");
        vnMatches12.resize(F1.n);
        return n;
    }

    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, float th, bool bMono) after projection
    int SearchByProjection(const orbhip_frame_view &CurrentFrame, const std::vector<orbhip_query> &q,
                           const uint8_t *qdesc, const uint8_t *taken, std::vector<int> &assign)
    {
        assign.assign(CurrentFrame.n > 0 ? CurrentFrame.n : 1, -1);
        int n = 0;
        check(orbhip_search_by_projection_frame(m_, &CurrentFrame, q.data(), qdesc, (int)q.size(), taken, assign.data(),
                                                mbCheckOrientation, &n), "orbhip_search_by_projection_frame");
        assign.resize(CurrentFrame.n);
        return n;
    }

    // int SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, float th) after isInFrustum
    int SearchByProjectionPoints(const orbhip_frame_view &F, const std::vector<orbhip_query> &q, const uint8_t *qdesc,
                                 const uint8_t *taken, std::vector<int> &assign)
    {
        assign.assign(F.n > 0 ? F.n : 1, -1);
        int n = 0;
        check(orbhip_search_by_projection_points(m_, &F, q.data(), qdesc, (int)q.size(), taken, assign.data(), mfNNratio,
                                                 &n), "orbhip_search_by_projection_points");
        assign.resize(F.n);
        return n;
    }

    // int SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches)   (max_dist = TH_LOW)
    // int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (max_dist = TH_LOW - 1)
    // node1/node2: FeatureVector node id per keypoint; matches12[i1] = i2 or -1
    int SearchByBoW(const orbhip_frame_view &F1, const uint32_t *node1, const uint8_t *valid1, const orbhip_frame_view &F2,
                    const uint32_t *node2, const uint8_t *blocked2, std::vector<int> &matches12, int max_dist = TH_LOW)
    {
        matches12.assign(F1.n > 0 ? F1.n : 1, -1);
        int n = 0;
        check(orbhip_search_by_bow(m_, &F1, node1, valid1, &F2, node2, blocked2, max_dist, mfNNratio, mbCheckOrientation,
                                   matches12.data(), &n), "orbhip_search_by_bow");
        matches12.resize(F1.n);
        return n;
    }

    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs,
    //                            bool bOnlyStereo)
    int SearchForTriangulation(const orbhip_frame_view &F1, const uint32_t *node1, const uint8_t *valid1,
                               const orbhip_frame_view &F2, const uint32_t *node2, const uint8_t *valid2, const float F12[9],
                               float ex, float ey, const float *level_sigma2,
                               std::vector<std::pair<size_t, size_t> > &vMatchedPairs, bool bOnlyStereo)
    {
        std::vector<int> m12(F1.n > 0 ? F1.n : 1, -1);
        int n = 0;
        check(orbhip_search_for_triangulation(m_, &F1, node1, valid1, &F2, node2, valid2, F12, ex, ey, level_sigma2,
                                              bOnlyStereo, mbCheckOrientation, m12.data(), &n),
              "orbhip_search_for_triangulation");
        vMatchedPairs.clear();
        vMatchedPairs.reserve(n);
        for (int i = 0; i < F1.n; ++i)
            if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
        return n;
    }

    // ---- projection prologues (the cv::Mat arithmetic in front of the searches, on the device) ---------------------
    // SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1339-1390: Tcw / Tlw = top three rows of
    // the two mTcw (12 floats, row-major); world[n][3], flags[n] (ORBHIP_POINT_*) per LastFrame.mvpMapPoints[i]
    std::vector<orbhip_query> ProjectLastFrame(const orbhip_camera &cam, const float *Tcw, const float *Tlw, int n,
                                               const float *world, const uint8_t *flags, const KeyPoint *lastKeysUn, float th,
                                               bool bMono)
    {
        std::vector<orbhip_query> q(n > 0 ? n : 1);
        check(orbhip_project_last_frame(m_, &cam, Tcw, Tlw, n, world, flags, lastKeysUn, th, bMono ? 1 : 0, q.data()),
              "orbhip_project_last_frame");
        q.resize(n);
        return q;
    }

    // Frame::isInFrustum + MapPoint::PredictScale for the local map (src/Frame.cc:269-325, src/MapPoint.cc:400-418) and
    // the window of SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:52-69)
    std::vector<orbhip_query> FrustumQueries(const orbhip_camera &cam, const float *Tcw, int n, const float *world,
                                             const float *normal, const float *maxDist, const float *minDist,
                                             const uint8_t *flags, float viewingCosLimit, float th,
                                             std::vector<float> *viewCos = nullptr)
    {
        std::vector<orbhip_query> q(n > 0 ? n : 1);
        if (viewCos) viewCos->assign(n > 0 ? n : 1, 0.f);
        check(orbhip_frustum_queries(m_, &cam, Tcw, n, world, normal, maxDist, minDist, flags, viewingCosLimit, th, q.data(),
                                     viewCos ? viewCos->data() : nullptr), "orbhip_frustum_queries");
        q.resize(n);
        if (viewCos) viewCos->resize(n);
        return q;
    }

    // prologue of Fuse x2 (mode 0) and of one direction of SearchBySim3 (mode 1), src/ORBmatcher.cc:853-888, 1005-1048,
    // 1155-1180, 1235-1260
    std::vector<orbhip_query> KeyFrameQueries(const orbhip_camera &cam, int mode, bool doubleInvz, const float *T1,
                                              const float *T2, int n, const float *world, const float *normal,
                                              const float *maxDist, const float *minDist, const uint8_t *flags, float th)
    {
        std::vector<orbhip_query> q(n > 0 ? n : 1);
        check(orbhip_keyframe_queries(m_, &cam, mode, doubleInvz ? 1 : 0, T1, T2, n, world, normal, maxDist, minDist, flags, th,
                                      q.data()), "orbhip_keyframe_queries");
        q.resize(n);
        return q;
    }

    // int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, float th, int ORBdist)
    // (relocalisation, src/ORBmatcher.cc:1472-1599) after projection; taken[n] = CurrentFrame.mvpMapPoints[i] != NULL
    int SearchByProjectionKeyFrame(const orbhip_frame_view &CurrentFrame, const std::vector<orbhip_query> &q,
                                   const uint8_t *qdesc, const uint8_t *taken, std::vector<int> &assign, int ORBdist)
    {
        assign.assign(CurrentFrame.n > 0 ? CurrentFrame.n : 1, -1);
        int n = 0;
        check(orbhip_search_by_projection_keyframe(m_, &CurrentFrame, q.data(), qdesc, (int)q.size(), taken, assign.data(),
                                                   ORBdist, mbCheckOrientation, &n), "orbhip_search_by_projection_keyframe");
        assign.resize(CurrentFrame.n);
        return n;
    }

    // int SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched,
    // int th) (loop closing, src/ORBmatcher.cc:290-403) after the Sim3 projection; matched[n] = vpMatched[idx] != NULL
    int SearchByProjectionSim3(const orbhip_frame_view &KF, const std::vector<orbhip_query> &q, const uint8_t *qdesc,
                               const uint8_t *matched, std::vector<int> &assign)
    {
        assign.assign(KF.n > 0 ? KF.n : 1, -1);
        int n = 0;
        check(orbhip_search_by_projection_sim3(m_, &KF, q.data(), qdesc, (int)q.size(), matched, assign.data(), &n),
              "orbhip_search_by_projection_sim3");
        assign.resize(KF.n);
        return n;
    }

    // int Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, float th)            (sim3Form = false, :825-975)
    // int Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, ...) (sim3Form = true, :977-1100)
    // up to the replace-or-add decision, which touches the map graph and stays with the caller: bestIdx[i] / bestDist[i]
    // = the key point the i-th map point would fuse with (-1 / 256 when nothing passes the gates)
    void Fuse(const orbhip_frame_view &KF, const orbhip_camera &cam, const float *Tcw, bool sim3Form, int n, const float *world,
              const float *normal, const float *maxDist, const float *minDist, const uint8_t *flags, const uint8_t *pointDesc,
              float th, const float *invLevelSigma2, std::vector<int> &bestIdx, std::vector<int> &bestDist)
    {
        bestIdx.assign(n > 0 ? n : 1, -1);
        bestDist.assign(n > 0 ? n : 1, 256);
        check(orbhip_fuse(m_, &KF, &cam, Tcw, sim3Form ? 1 : 0, n, world, normal, maxDist, minDist, flags, pointDesc, th,
                          invLevelSigma2, bestIdx.data(), bestDist.data()), "orbhip_fuse");
        bestIdx.resize(n);
        bestDist.resize(n);
    }

    // Fuse for K key frames and one set of n map points in one call: the matching of LocalMapping::SearchInNeighbors
    // (src/LocalMapping.cc:454-515) and LoopClosing::SearchAndFuse (src/LoopClosing.cc:585-610), ORBmatcher::Fuse
    // src/ORBmatcher.cc:825-950 / :975-1075 up to the decision.  Tcw [K][12], flags [K][n] (!IsInKeyFrame per target);
    // bestIdx / bestDist [K][n], row k = what Fuse(*KFs[k], cam, Tcw + 12*k, ..., flags + n*k, ...) gives.  The caller
    // applies the rows in key-frame order ("Fusing into many key frames").
    void FuseBatch(const std::vector<const orbhip_frame_view *> &KFs, const orbhip_camera &cam, const float *Tcw, bool sim3Form,
                   int n, const float *world, const float *normal, const float *maxDist, const float *minDist,
                   const uint8_t *flags, const uint8_t *pointDesc, float th, const float *invLevelSigma2,
                   std::vector<int> &bestIdx, std::vector<int> &bestDist)
    {
        const size_t total = KFs.size() * (size_t)(n > 0 ? n : 0);
        bestIdx.assign(total ? total : 1, -1);
        bestDist.assign(total ? total : 1, 256);
        check(orbhip_fuse_batch(m_, (int)KFs.size(), KFs.data(), &cam, Tcw, sim3Form ? 1 : 0, n, world, normal, maxDist, minDist,
                                flags, pointDesc, th, invLevelSigma2, bestIdx.data(), bestDist.data()), "orbhip_fuse_batch");
        bestIdx.resize(total);
        bestDist.resize(total);
    }
    // device frames and points, asynchronous on the matcher's stream: orbhip_fuse_device with the mirror's handle
    void FuseDevice(int K, const void *dKfIndex, const orbhip_camera &cam, const void *dTcw, bool sim3Form, const void *dKps,
                    const void *dDesc, const void *dN, int cap, const void *dURight, const void *dCellStart,
                    const void *dCellItems, int np, int pcap, const void *dWorld, const void *dNormal, const void *dMaxDist,
                    const void *dMinDist, const void *dPointDesc, const void *dFlags, float th, const float *invLevelSigma2,
                    void *dBestIdx, void *dBestDist, void *dQ = nullptr)
    {
        check(orbhip_fuse_device(m_, K, dKfIndex, &cam, dTcw, sim3Form ? 1 : 0, dKps, dDesc, dN, cap, dURight, dCellStart,
                                 dCellItems, np, pcap, dWorld, dNormal, dMaxDist, dMinDist, dPointDesc, dFlags, th,
                                 invLevelSigma2, dBestIdx, dBestDist, dQ), "orbhip_fuse_device");
    }

    // void LocalMapping::CreateNewMapPoints() (src/LocalMapping.cc:207-452) up to `new MapPoint`, for the current key frame
    // and its K neighbours in one call: baseline gate, ComputeF12 (:536-553), SearchForTriangulation and the loop body
    // :286-431.  Host buffers; per-key-point arrays as orbhip_create_new_map_points takes them (hasPoint* nullable, depth*
    // stereo only, medianDepth [K] monocular only).  Outputs are packed by the current key frame's count n: matches12 /
    // status [K][n], x3D [K][n][3], nmatches / skipped [K]; status holds ORBHIP_NEWPOINT_*.  The caller applies the rows
    // in neighbour order ("Creating new map points").
    struct NewMapPoints {
        std::vector<int> matches12, nmatches;
        std::vector<float> x3D, f12, epipole;
        std::vector<uint8_t> status, skipped;
    };
    void CreateNewMapPoints(const orbhip_frame_view &cur, const uint32_t *nodeCur, const uint8_t *hasPointCur,
                            const float *depthCur, const float *TcwCur, const std::vector<const orbhip_frame_view *> &KFs,
                            const std::vector<const uint32_t *> &node, const std::vector<const uint8_t *> &hasPoint,
                            const std::vector<const float *> &depth, const float *Tcw, const float *medianDepth,
                            const orbhip_camera &cam, bool onlyStereo, const float *levelSigma2, NewMapPoints &out)
    {
        const size_t K = KFs.size(), n = (size_t)(cur.n > 0 ? cur.n : 0), kn = K * n;
        out.matches12.assign(kn ? kn : 1, -1);
        out.status.assign(kn ? kn : 1, (uint8_t)ORBHIP_NEWPOINT_NO_MATCH);
        out.x3D.assign(kn ? kn * 3 : 1, 0.f);
        out.nmatches.assign(K ? K : 1, 0);
        out.skipped.assign(K ? K : 1, 0);
        out.f12.assign(K ? K * 9 : 1, 0.f);
        out.epipole.assign(K ? K * 2 : 1, 0.f);
        check(orbhip_create_new_map_points(m_, &cur, nodeCur, hasPointCur, depthCur, TcwCur, (int)K, KFs.data(), node.data(),
                                           hasPoint.empty() ? nullptr : hasPoint.data(), depth.empty() ? nullptr : depth.data(),
                                           Tcw, medianDepth, &cam, onlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0, levelSigma2,
                                           out.matches12.data(), out.nmatches.data(), out.x3D.data(), out.status.data(),
                                           out.skipped.data(), out.f12.data(), out.epipole.data()),
              "orbhip_create_new_map_points");
        out.matches12.resize(kn); out.status.resize(kn); out.x3D.resize(kn * 3);
        out.nmatches.resize(K); out.skipped.resize(K); out.f12.resize(K * 9); out.epipole.resize(K * 2);
    }
    // device frames, asynchronous on the matcher's stream: orbhip_create_new_map_points_device with the mirror's handle
    void CreateNewMapPointsDevice(int cur, int K, const void *dKfIndex, const orbhip_camera &cam, const void *dTcw,
                                  const void *dKps, const void *dDesc, const void *dN, int cap, const void *dURight,
                                  const void *dDepth, const void *dNode, const void *dHasPoint, const void *dMedianDepth,
                                  bool onlyStereo, const float *levelSigma2, void *dMatches12, void *dNMatches, void *dX3D,
                                  void *dStatus, void *dSkipped, void *dF12 = nullptr, void *dEpipole = nullptr)
    {
        check(orbhip_create_new_map_points_device(m_, cur, K, dKfIndex, &cam, dTcw, dKps, dDesc, dN, cap, dURight, dDepth, dNode,
                                                  dHasPoint, dMedianDepth, onlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0,
                                                  levelSigma2, dMatches12, dNMatches, dX3D, dStatus, dSkipped, dF12, dEpipole),
              "orbhip_create_new_map_points_device");
    }

    // int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12,
    // const cv::Mat &t12, const float th) (src/ORBmatcher.cc:1102-1326), complete.  T1w / T2w: [R | t] of the two key
    // frames; S21 = [sR21 | t21], S12 = [sR12 | t12] as the reference computes them (:1119-1121).  Per key-frame slot: the
    // slot's map point (world, mfMax/MinDistance, descriptor) and ORBHIP_POINT_PRESENT iff it takes part (:1132-1143).
    int SearchBySim3(const orbhip_frame_view &KF1, const orbhip_frame_view &KF2, const orbhip_camera &cam, const float *T1w,
                     const float *T2w, const float *S21, const float *S12, const float *world1, const float *maxDist1,
                     const float *minDist1, const uint8_t *flags1, const uint8_t *desc1, const float *world2,
                     const float *maxDist2, const float *minDist2, const uint8_t *flags2, const uint8_t *desc2, float th,
                     std::vector<int> &matches12)
    {
        matches12.assign(KF1.n > 0 ? KF1.n : 1, -1);
        int n = 0;
        check(orbhip_search_by_sim3(m_, &KF1, &KF2, &cam, T1w, T2w, S21, S12, world1, maxDist1, minDist1, flags1, desc1, world2,
                                    maxDist2, minDist2, flags2, desc2, th, matches12.data(), &n), "orbhip_search_by_sim3");
        matches12.resize(KF1.n);
        return n;
    }

    // the search loop of Fuse / SearchBySim3 on caller-made queries (src/ORBmatcher.cc:893-950, 1199-1219)
    void SearchBestInWindow(const orbhip_frame_view &KF, const std::vector<orbhip_query> &q, const uint8_t *qdesc, bool chi2Gate,
                            const float *invLevelSigma2, std::vector<int> &bestIdx, std::vector<int> &bestDist)
    {
        bestIdx.assign(q.size() ? q.size() : 1, -1);
        bestDist.assign(q.size() ? q.size() : 1, 256);
        check(orbhip_search_best_in_window(m_, &KF, q.data(), qdesc, (int)q.size(), chi2Gate ? 1 : 0, invLevelSigma2, bestIdx.data(),
                                           bestDist.data()), "orbhip_search_best_in_window");
        bestIdx.resize(q.size());
        bestDist.resize(q.size());
    }

    // MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307), batched over map points
    std::vector<int> DistinctiveDescriptors(const uint8_t *desc, const std::vector<int32_t> &offsets)
    {
        const int np = (int)offsets.size() - 1;
        std::vector<int> best(np > 0 ? np : 1, -1);
        if (np > 0) check(orbhip_distinctive_descriptors(m_, desc, offsets.data(), np, best.data()), "orbhip_distinctive_descriptors");
        best.resize(np > 0 ? np : 0);
        return best;
    }

    // Frame glue either side of the searches: UndistortKeyPoints, AssignFeaturesToGrid, ComputeStereoFromRGBD
    // (src/Frame.cc:404-434, 230-245, 643-664)
    std::vector<KeyPoint> UndistortKeyPoints(const std::vector<KeyPoint> &keys, float fx, float fy, float cx, float cy,
                                             const float dist5[5])
    {
        std::vector<KeyPoint> un(keys.size() ? keys.size() : 1);
        check(orbhip_undistort_keypoints(m_, keys.data(), (int)keys.size(), fx, fy, cx, cy, dist5, un.data()),
              "orbhip_undistort_keypoints");
        un.resize(keys.size());
        return un;
    }
    void ComputeStereoFromRGBD(const std::vector<KeyPoint> &keys, const std::vector<KeyPoint> &keysUn, const float *depth, int rows,
                               int cols, int strideFloats, float mbf, std::vector<float> &mvuRight, std::vector<float> &mvDepth)
    {
        mvuRight.assign(keys.size() ? keys.size() : 1, -1.f);
        mvDepth.assign(keys.size() ? keys.size() : 1, -1.f);
        check(orbhip_compute_stereo_from_rgbd(m_, keys.data(), keysUn.data(), (int)keys.size(), depth, rows, cols, strideFloats, mbf,
                                              mvuRight.data(), mvDepth.data()), "orbhip_compute_stereo_from_rgbd");
        mvuRight.resize(keys.size());
        mvDepth.resize(keys.size());
    }

    // the same on the sensor's depth image (CV_16U: depthType ORBHIP_DEPTH_U16, or CV_32F): the convertTo(CV_32F,
    // mDepthMapFactor) of src/Tracking.cc:227-228 is applied to the sampled values; depthFactor = mDepthMapFactor
    void ComputeStereoFromRGBD(const std::vector<KeyPoint> &keys, const std::vector<KeyPoint> &keysUn, const void *depth, int depthType,
                               int rows, int cols, int strideElems, float depthFactor, float mbf, std::vector<float> &mvuRight,
                               std::vector<float> &mvDepth)
    {
        mvuRight.assign(keys.size() ? keys.size() : 1, -1.f);
        mvDepth.assign(keys.size() ? keys.size() : 1, -1.f);
        check(orbhip_compute_stereo_from_rgbd_raw(m_, keys.data(), keysUn.data(), (int)keys.size(), depth, depthType, rows, cols,
                                                  strideElems, depthFactor, mbf, mvuRight.data(), mvDepth.data()),
              "orbhip_compute_stereo_from_rgbd_raw");
        mvuRight.resize(keys.size());
        mvDepth.resize(keys.size());
    }

    // Seeding stereo / RGB-D map points: the depth-sorted creation loop of Tracking::UpdateLastFrame (src/Tracking.cc:812-864)
    // and Tracking::CreateNewKeyFrame (:1073-1133) with mode ORBHIP_SEED_CLOSEST, Tracking::StereoInitialization (:523-538)
    // with ORBHIP_SEED_ALL, positions by Frame::UnprojectStereo (src/Frame.cc:666-680).  flags[i]: ORBHIP_POINT_PRESENT =
    // mvpMapPoints[i] != NULL, ORBHIP_POINT_OBSERVED = Observations() > 0.  world (3 floats per keypoint) and flags are
    // updated in place; order = the visited keypoints in the order the caller creates its MapPoints; created[i] = 0 / 1.
    // Returns the number of created points.  keysUn = mvKeysUn (the KeyFrame form, src/KeyFrame.cc:615-631, passes mvKeys).
    struct SeedCounts { int nValid, nVisited, nCreated; };
    int SeedStereoPoints(const orbhip_camera &cam, const float Tcw[12], const std::vector<KeyPoint> &keysUn,
                         const std::vector<float> &mvDepth, float thDepth, int mode, int createdFlags, std::vector<float> &world,
                         std::vector<uint8_t> &flags, std::vector<int> &order, std::vector<uint8_t> &created,
                         SeedCounts *countsOut = nullptr)
    {
        const size_t n = keysUn.size();
        if (mvDepth.size() != n || world.size() != 3 * n || flags.size() != n) throw Error(ORBHIP_E_ARG, "SeedStereoPoints");
        order.assign(n ? n : 1, -1);
        created.assign(n ? n : 1, 0);
        int32_t counts[3] = {0, 0, 0};
        check(orbhip_seed_stereo_points(m_, &cam, Tcw, keysUn.data(), mvDepth.data(), (int)n, thDepth, mode, createdFlags, world.data(),
                                        flags.data(), order.data(), created.data(), counts), "orbhip_seed_stereo_points");
        order.resize((size_t)counts[1]);
        created.resize(n);
        if (countsOut) { countsOut->nValid = counts[0]; countsOut->nVisited = counts[1]; countsOut->nCreated = counts[2]; }
        return counts[2];
    }
    // device frames, asynchronous on the matcher's stream: orbhip_seed_stereo_points_device with the mirror's handle
    void SeedStereoPointsDevice(int frames, const orbhip_camera &cam, const void *dTcw, const void *dKps, const void *dN, int cap,
                                int kpFirst, int kpStep, const void *dDepth, float thDepth, int mode, int createdFlags, void *dWorld,
                                void *dFlags, void *dOrder, void *dCreated, void *dCounts)
    {
        check(orbhip_seed_stereo_points_device(m_, frames, &cam, dTcw, dKps, dN, cap, kpFirst, kpStep, dDepth, thDepth, mode,
                                               createdFlags, dWorld, dFlags, dOrder, dCreated, dCounts),
              "orbhip_seed_stereo_points_device");
    }
    // cv::Mat Frame::UnprojectStereo(const int &i) (src/Frame.cc:666-680) for every keypoint: mode ORBHIP_SEED_ALL on scratch
    // arrays.  x3D holds 3 floats per keypoint; valid[i] = 0 where the reference returns an empty cv::Mat (z <= 0).
    void UnprojectStereo(const orbhip_camera &cam, const float Tcw[12], const std::vector<KeyPoint> &keysUn,
                         const std::vector<float> &mvDepth, std::vector<float> &x3D, std::vector<uint8_t> &valid)
    {
        std::vector<uint8_t> flags(keysUn.size(), 0);
        std::vector<int> order;
        x3D.assign(3 * keysUn.size(), 0.f);
        SeedStereoPoints(cam, Tcw, keysUn, mvDepth, 0.f, ORBHIP_SEED_ALL, ORBHIP_POINT_PRESENT, x3D, flags, order, valid);
    }
    // one keypoint, like the reference's signature; false = empty cv::Mat
    bool UnprojectStereo(int i, const orbhip_camera &cam, const float Tcw[12], const std::vector<KeyPoint> &keysUn,
                         const std::vector<float> &mvDepth, float x3D[3])
    {
        if (i < 0 || (size_t)i >= keysUn.size() || mvDepth.size() != keysUn.size()) throw Error(ORBHIP_E_ARG, "UnprojectStereo");
        const std::vector<KeyPoint> k(1, keysUn[(size_t)i]);
        const std::vector<float> z(1, mvDepth[(size_t)i]);
        std::vector<float> X;
        std::vector<uint8_t> valid;
        UnprojectStereo(cam, Tcw, k, z, X, valid);
        x3D[0] = X[0]; x3D[1] = X[1]; x3D[2] = X[2];
        return valid[0] != 0;
    }
    // Tracking::NeedNewKeyFrame's nTrackedClose / nNonTrackedClose (src/Tracking.cc:1001-1018).  Here ORBHIP_POINT_PRESENT
    // means mvpMapPoints[i] && !mvbOutlier[i].
    void CountClosePoints(const std::vector<float> &mvDepth, const std::vector<uint8_t> &flags, float thDepth, int &nTrackedClose,
                          int &nNonTrackedClose)
    {
        if (mvDepth.size() != flags.size()) throw Error(ORBHIP_E_ARG, "CountClosePoints");
        check(orbhip_count_close_points(m_, mvDepth.data(), flags.data(), (int)mvDepth.size(), thDepth, &nTrackedClose,
                                        &nNonTrackedClose), "orbhip_count_close_points");
    }
    void CountClosePointsDevice(int frames, const void *dDepth, const void *dFlags, const void *dN, int cap, float thDepth,
                                void *dCounts)
    {
        check(orbhip_count_close_points_device(m_, frames, dDepth, dFlags, dN, cap, thDepth, dCounts),
              "orbhip_count_close_points_device");
    }

    // MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307; what & ORBHIP_UPDATE_DESCRIPTOR) and
    // MapPoint::UpdateNormalAndDepth (:330-371; what & ORBHIP_UPDATE_NORMAL_DEPTH) for the obsStart.size() - 1 map points of an
    // observation table in CSR form: observation j of point p is key point obsIdx[o] of KFs[obsKf[o]], o = obsStart[p] + j;
    // refObs[p] is the position of mpRefKF's observation in the point's list.  Tcw: 12 floats per key frame; kfBad: one
    // byte per key frame (pKF->isBad()) or empty; flags: ORBHIP_POINT_PRESENT = !mbBad.  pointDesc (32 bytes per point),
    // normal (3 floats), maxDist and minDist are updated in place where the reference writes; bestObs = the position of
    // the chosen descriptor in each list (-1: none), status = one ORBHIP_MAPPOINT_* code per point.
    void UpdateMapPoints(const orbhip_camera &cam, int what, const std::vector<const orbhip_frame_view *> &KFs,
                         const std::vector<float> &Tcw, const std::vector<uint8_t> &kfBad, const std::vector<int32_t> &obsStart,
                         const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx, const std::vector<int32_t> &refObs,
                         const std::vector<float> &world, const std::vector<uint8_t> &flags, std::vector<uint8_t> &pointDesc,
                         std::vector<float> &normal, std::vector<float> &maxDist, std::vector<float> &minDist,
                         std::vector<int32_t> &bestObs, std::vector<uint8_t> &status)
    {
        if (obsStart.empty()) throw Error(ORBHIP_E_ARG, "UpdateMapPoints");
        const size_t n = obsStart.size() - 1, K = KFs.size();
        if (Tcw.size() != 12 * K || (!kfBad.empty() && kfBad.size() != K) || obsKf.size() != obsIdx.size() ||
            (n > 0 && (obsStart[n] < 0 || obsKf.size() < (size_t)obsStart[n])) || refObs.size() != n || world.size() != 3 * n ||
            flags.size() != n || pointDesc.size() != 32 * n || normal.size() != 3 * n || maxDist.size() != n || minDist.size() != n)
            throw Error(ORBHIP_E_ARG, "UpdateMapPoints");
        bestObs.assign(n ? n : 1, -1);
        status.assign(n ? n : 1, 0);
        check(orbhip_update_map_points(m_, &cam, what, (int)K, KFs.data(), Tcw.data(), kfBad.empty() ? nullptr : kfBad.data(), (int)n,
                                       obsStart.data(), obsKf.data(), obsIdx.data(), refObs.data(), world.data(), flags.data(),
                                       pointDesc.data(), normal.data(), maxDist.data(), minDist.data(), bestObs.data(),
                                       status.data()), "orbhip_update_map_points");
        bestObs.resize(n);
        status.resize(n);
    }
    // device-resident, asynchronous on the matcher's stream: orbhip_update_map_points_device with the mirror's handle; the
    // table indexes the rows of the bank the other *Device calls read, and the four arrays are the ones FuseDevice reads
    void UpdateMapPointsDevice(const orbhip_camera &cam, int what, const void *dTcw, const void *dKps, const void *dDesc,
                               const void *dN, int cap, const void *dKfBad, int np, int pcap, const void *dObsStart,
                               const void *dObsKf, const void *dObsIdx, const void *dRefObs, const void *dWorld, const void *dFlags,
                               void *dPointDesc, void *dNormal, void *dMaxDist, void *dMinDist, void *dBestObs, void *dStatus)
    {
        check(orbhip_update_map_points_device(m_, &cam, what, dTcw, dKps, dDesc, dN, cap, dKfBad, np, pcap, dObsStart, dObsKf,
                                              dObsIdx, dRefObs, dWorld, dFlags, dPointDesc, dNormal, dMaxDist, dMinDist, dBestObs,
                                              dStatus), "orbhip_update_map_points_device");
    }

    // Tracking::UpdateLocalKeyFrames, UpdateLocalPoints and the bookkeeping in front of SearchLocalPoints' search
    // (src/Tracking.cc:1146-1180, :1205-1339) for `frames` current frames over tables; the records and the report are
    // described at orbhip_update_local_map_device in orbhip.h.  Host pointers, synchronous and range-checked: io's
    // frame_point, local_kf and n_local_kf are updated in place, the outputs are written up to their counts.
    void UpdateLocalMap(int frames, int rows, int cap, int np, int pcap, const orbhip_local_map_tables &tables,
                        const orbhip_local_map_io &io)
    {
        check(orbhip_update_local_map(m_, frames, rows, cap, np, pcap, &tables, &io), "orbhip_update_local_map");
    }
    // device pointers, asynchronous on the matcher's stream, no range checks
    void UpdateLocalMapDevice(int frames, int rows, int cap, int np, int pcap, const orbhip_local_map_tables &dTables,
                              const orbhip_local_map_io &dIo)
    {
        check(orbhip_update_local_map_device(m_, frames, rows, cap, np, pcap, &dTables, &dIo), "orbhip_update_local_map_device");
    }
    // the same, then Frame::isInFrustum(pMP, viewingCosLimit) and SearchByProjection(F, vpMapPoints, th) with nnratio on the
    // same stream: the matching step of Tracking::TrackLocalMap
    void TrackLocalMapDevice(int frames, int rows, int cap, int np, int pcap, const orbhip_local_map_tables &dTables,
                             const orbhip_local_map_io &dIo, const orbhip_camera &cam, const orbhip_local_map_track &dTrack,
                             float viewingCosLimit, float th, float nnratio)
    {
        check(orbhip_track_local_map_device(m_, frames, rows, cap, np, pcap, &dTables, &dIo, &cam, &dTrack, viewingCosLimit, th,
                                            nnratio), "orbhip_track_local_map_device");
    }

    // KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379) with AddConnection / UpdateBestCovisibles (:123-157) for the U
    // bank rows of updateRows, in list order; the records, the order rules and the report are described at
    // orbhip_update_connections_device in orbhip.h.  Host pointers, synchronous and range-checked: the rows of `state` the
    // call reaches are updated in place, report [U][8] is written.
    void UpdateConnections(int rows, int cap, int np, int pcap, const orbhip_covis_tables &tables, const orbhip_covis_state &state,
                           int id0Row, int U, const int32_t *updateRows, int32_t *report)
    {
        check(orbhip_update_connections(m_, rows, cap, np, pcap, &tables, &state, id0Row, U, updateRows, report),
              "orbhip_update_connections");
    }
    // device pointers, asynchronous on the matcher's stream, no range checks
    void UpdateConnectionsDevice(int rows, int cap, int np, int pcap, const orbhip_covis_tables &dTables,
                                 const orbhip_covis_state &dState, int id0Row, int U, const void *dUpdateRows, void *dReport)
    {
        check(orbhip_update_connections_device(m_, rows, cap, np, pcap, &dTables, &dState, id0Row, U, dUpdateRows, dReport),
              "orbhip_update_connections_device");
    }
    // GetBestCovisibilityKeyFrames(nn) (nn2 == 0, :174-182) or vpTargetKFs of LocalMapping::SearchInNeighbors (nn2 > 0,
    // src/LocalMapping.cc:457-479) for Q current rows: targets [Q][nn * (1 + nn2)], -1 behind counts [Q]
    void CovisibleTargets(int rows, const int32_t *ordKf, const int32_t *nOrd, const uint8_t *kfBad, int Q, const int32_t *cur,
                          int nn, int nn2, int32_t *targets, int32_t *counts)
    {
        check(orbhip_covisible_targets(m_, rows, ordKf, nOrd, kfBad, Q, cur, nn, nn2, targets, counts), "orbhip_covisible_targets");
    }
    void CovisibleTargetsDevice(int rows, const void *dOrdKf, const void *dNOrd, const void *dKfBad, int Q, const void *dCur, int nn,
                                int nn2, void *dTargets, void *dCounts)
    {
        check(orbhip_covisible_targets_device(m_, rows, dOrdKf, dNOrd, dKfBad, Q, dCur, nn, nn2, dTargets, dCounts),
              "orbhip_covisible_targets_device");
    }
    // mspChildrens of every row as CSR from mpParent and isBad(), ascending row inside a list
    void ChildrenFromParentsDevice(int rows, const void *dParent, const void *dKfBad, void *dChildStart, void *dChild)
    {
        check(orbhip_children_from_parents_device(m_, rows, dParent, dKfBad, dChildStart, dChild),
              "orbhip_children_from_parents_device");
    }

    // LocalMapping::MapPointCulling (src/LocalMapping.cc:170-205) with MapPoint::SetBadFlag over the entries of `recent`; the
    // records, the table out and the status codes are described at orbhip_cull_map_points_device in orbhip.h.  Host pointers,
    // synchronous and range-checked: slot_point, flags and the table out of `io` are written, recentOut / nRecentOut hold
    // the list left, status [R] one ORBHIP_CULLPOINT_* code per entry.
    void CullMapPoints(int rows, int cap, int np, int pcap, int obsCap, const orbhip_cull_tables &tables, const orbhip_cull_io &io,
                       int R, const int32_t *recent, const int32_t *found, const int32_t *visible, const int32_t *firstKfId,
                       int curKfId, int thObs, int32_t *recentOut, int32_t *nRecentOut, uint8_t *status)
    {
        check(orbhip_cull_map_points(m_, rows, cap, np, pcap, obsCap, &tables, &io, R, recent, found, visible, firstKfId, curKfId,
                                     thObs, recentOut, nRecentOut, status), "orbhip_cull_map_points");
    }
    // device pointers, asynchronous on the matcher's stream, no range checks
    void CullMapPointsDevice(int rows, int cap, int np, int pcap, int obsCap, const orbhip_cull_tables &dTables,
                             const orbhip_cull_io &dIo, int R, const void *dRecent, const void *dFound, const void *dVisible,
                             const void *dFirstKfId, int curKfId, int thObs, void *dRecentOut, void *dNRecentOut, void *dStatus)
    {
        check(orbhip_cull_map_points_device(m_, rows, cap, np, pcap, obsCap, &dTables, &dIo, R, dRecent, dFound, dVisible, dFirstKfId,
                                            curKfId, thObs, dRecentOut, dNRecentOut, dStatus), "orbhip_cull_map_points_device");
    }
    // LocalMapping::KeyFrameCulling (:632-696) with KeyFrame::SetBadFlag, EraseConnection and MapPoint::EraseObservation over
    // the candidate rows `cand` (-1 entries are skipped), each decided against the state the candidates before it left;
    // report [U][8] as described at orbhip_cull_key_frames_device in orbhip.h.  Host pointers, synchronous, range-checked.
    void CullKeyFrames(int rows, int cap, int np, int pcap, int obsCap, const orbhip_cull_tables &tables, const orbhip_cull_io &io,
                       const orbhip_covis_state &state, int id0Row, int U, const int32_t *cand, bool mono, float thDepth,
                       int32_t *report)
    {
        check(orbhip_cull_key_frames(m_, rows, cap, np, pcap, obsCap, &tables, &io, &state, id0Row, U, cand, mono ? 1 : 0, thDepth,
                                     report), "orbhip_cull_key_frames");
    }
    void CullKeyFramesDevice(int rows, int cap, int np, int pcap, int obsCap, const orbhip_cull_tables &dTables,
                             const orbhip_cull_io &dIo, const orbhip_covis_state &dState, int id0Row, int U, const void *dCand,
                             bool mono, float thDepth, void *dReport)
    {
        check(orbhip_cull_key_frames_device(m_, rows, cap, np, pcap, obsCap, &dTables, &dIo, &dState, id0Row, U, dCand, mono ? 1 : 0,
                                            thDepth, dReport), "orbhip_cull_key_frames_device");
    }

    // the Frame statics the prologues read (src/Frame.cc:97-112), as one record
    static orbhip_camera MakeCamera(float fx, float fy, float cx, float cy, float mbf, float mb, float minX, float maxX, float minY,
                                    float maxY, const std::vector<float> &scaleFactors, float logScaleFactor)
    {
        orbhip_camera c = {};
        c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.mbf = mbf; c.mb = mb;
        c.min_x = minX; c.max_x = maxX; c.min_y = minY; c.max_y = maxY;
        c.n_levels = (int32_t)scaleFactors.size();
        c.log_scale_factor = logScaleFactor;
        for (size_t i = 0; i < scaleFactors.size() && i < (size_t)ORBHIP_MAX_LEVELS; ++i) c.scale_factors[i] = scaleFactors[i];
        return c;
    }
    // a Frame / KeyFrame as the searches see it (mvKeysUn, mDescriptors, mvuRight, image bounds, 64 x 48 grid scale)
    static orbhip_frame_view MakeFrameView(const std::vector<KeyPoint> &keysUn, const std::vector<uint8_t> &desc, const float *uRight,
                                           float minX, float minY, float maxX, float maxY, const std::vector<float> &scaleFactors)
    {
        orbhip_frame_view v = {};
        v.n = (int32_t)keysUn.size(); v.keys = keysUn.data(); v.desc = desc.data(); v.u_right = uRight;
        v.min_x = minX; v.min_y = minY; v.max_x = maxX; v.max_y = maxY;
        v.grid_inv_w = 64.f / (maxX - minX); v.grid_inv_h = 48.f / (maxY - minY);   // src/Frame.cc:101-102
        v.n_levels = (int32_t)scaleFactors.size(); v.scale_factors = scaleFactors.data();
        return v;
    }

    // void Frame::ComputeStereoMatches(): pyramids come from the two extractor objects
    int ComputeStereoMatches(ORBextractor &left, ORBextractor &right, const std::vector<KeyPoint> &keysL,
                             const std::vector<uint8_t> &descL, const std::vector<KeyPoint> &keysR,
                             const std::vector<uint8_t> &descR, float mbf, float mb, std::vector<float> &mvuRight,
                             std::vector<float> &mvDepth)
    {
        mvuRight.assign(keysL.size() ? keysL.size() : 1, -1.f);
        mvDepth.assign(keysL.size() ? keysL.size() : 1, -1.f);
        int n = 0;
        check(orbhip_compute_stereo_matches(m_, left.handle(), 0, right.handle(), 0, keysL.data(), descL.data(),
                                            (int)keysL.size(), keysR.data(), descR.data(), (int)keysR.size(), mbf, mb,
                                            mvuRight.data(), mvDepth.data(), &n), "orbhip_compute_stereo_matches");
        mvuRight.resize(keysL.size());
        mvDepth.resize(keysL.size());
        return n;
    }

protected:
    orbhip_matcher *m_;
    float mfNNratio;
    bool mbCheckOrientation;
};

}  // namespace orbhip
