/*
 * orbhip.h -- C ABI of the MI355X-native ORB front-end and descriptor matching.
 *
 * Drop-in boundary for ORB-SLAM2's hot path (citations are file:line in the
 * reference tree).  Every entry point is plain C: pointers + sizes, int status
 * (0 = ok, < 0 = error), never throws.  Host-pointer entry points are
 * synchronous; *_device entry points enqueue on the handle's HIP stream and
 * take/return device pointers.
 *
 *   orbhip_extractor_*        replaces class ORBextractor
 *                             (include/ORBextractor.h:45-110, src/ORBextractor.cc:410-1132)
 *   orbhip_extract            replaces ORBextractor::operator()  (include/ORBextractor.h:59-61)
 *   orbhip_extract_color*     the cvtColor(.., CV_{RGB,BGR,RGBA,BGRA}2GRAY) of Tracking::GrabImage{Monocular,Stereo,RGBD}
 *                             (src/Tracking.cc:172-197, 212-225, 242-256) followed by ORBextractor::operator()
 *   orbhip_init_undistort_rectify_map / orbhip_extract_remap*   the cv::initUndistortRectifyMap and cv::remap of the
 *                             stereo example (Examples/Stereo/stereo_euroc.cc:63-98, 136-137) followed by operator()
 *   orbhip_pyramid_level*     replaces the public member mvImagePyramid (include/ORBextractor.h:85)
 *   orbhip_matcher_*          replaces class ORBmatcher (include/ORBmatcher.h:37-103)
 *   orbhip_descriptor_distance  ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1647-1663)
 *   orbhip_search_for_initialization  ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520)
 *   orbhip_search_by_projection_frame ORBmatcher::SearchByProjection(Frame&,const Frame&,th,bMono)
 *                                     (src/ORBmatcher.cc:1328-1470)
 *   orbhip_search_by_projection_points ORBmatcher::SearchByProjection(Frame&,vector<MapPoint*>&,th)
 *                                     (src/ORBmatcher.cc:45-129)
 *   orbhip_compute_stereo_matches     Frame::ComputeStereoMatches (src/Frame.cc:466-640)
 *   orbhip_search_by_projection_keyframe ORBmatcher::SearchByProjection(Frame&,KeyFrame*,sAlreadyFound,th,ORBdist)
 *                                     (src/ORBmatcher.cc:1472-1599, relocalisation)
 *   orbhip_search_by_projection_sim3  ORBmatcher::SearchByProjection(KeyFrame*,Scw,vpPoints,vpMatched,th)
 *                                     (src/ORBmatcher.cc:290-403, loop closing)
 *   orbhip_search_best_in_window      inner search of ORBmatcher::Fuse x2 (src/ORBmatcher.cc:825-1100) and of both
 *                                     directions of SearchBySim3 (:1102-1326)
 *   orbhip_undistort_keypoints        Frame::UndistortKeyPoints (src/Frame.cc:404-434)
 *   orbhip_assign_features_to_grid    Frame::AssignFeaturesToGrid (src/Frame.cc:230-245)
 *   orbhip_compute_stereo_from_rgbd   Frame::ComputeStereoFromRGBD (src/Frame.cc:643-664)
 *   orbhip_compute_stereo_from_rgbd_raw  the same on the sensor's depth image: imDepth.convertTo(CV_32F, mDepthMapFactor)
 *                                     (src/Tracking.cc:227-228) applied to the samples the keypoints read
 *   orbhip_distinctive_descriptors    MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307), batched
 *   orbhip_update_map_points*         the same and MapPoint::UpdateNormalAndDepth (:330-371) from an observation table
 *   orbhip_update_local_map*          Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (src/Tracking.cc:1205-1339) over tables;
 *   orbhip_track_local_map_device     the same + SearchLocalPoints' frustum test and search (:1143-1193)
 *   orbhip_update_connections*        KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379) with AddConnection and
 *                                     UpdateBestCovisibles (:123-157) over tables
 *   orbhip_covisible_targets*         KeyFrame::GetBestCovisibilityKeyFrames (:174-182) and the target list of
 *                                     LocalMapping::SearchInNeighbors (src/LocalMapping.cc:457-479)
 *   orbhip_children_from_parents_device  mspChildrens of every row from mpParent and isBad()
 *   orbhip_cull_map_points*           LocalMapping::MapPointCulling (src/LocalMapping.cc:170-205) with MapPoint::SetBadFlag
 *   orbhip_cull_key_frames*           LocalMapping::KeyFrameCulling (:632-696) with KeyFrame::SetBadFlag, EraseConnection
 *                                     and MapPoint::EraseObservation, over tables
 *   orbhip_vocabulary_*               ORBVocabulary (DBoW2::TemplatedVocabulary<FORB>) loadFromTextFile + transform,
 *                                     i.e. Frame::ComputeBoW (src/Frame.cc:395-402)
 *   orbhip_search_by_bow              ORBmatcher::SearchByBoW(KeyFrame*,Frame&,..) (src/ORBmatcher.cc:159-288) and
 *                                     SearchByBoW(KeyFrame*,KeyFrame*,..) (:522-655); vocabulary node ids are inputs
 *   orbhip_search_for_triangulation   ORBmatcher::SearchForTriangulation (:657-823) incl. CheckDistEpipolarLine (:140-157)
 */
#ifndef ORBHIP_H
#define ORBHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBHIP_OK 0
#define ORBHIP_E_ARG (-1)       /* bad argument */
#define ORBHIP_E_HIP (-2)       /* HIP runtime error (see orbhip_last_error) */
#define ORBHIP_E_CAPACITY (-3)  /* caller buffer / internal capacity too small */
#define ORBHIP_E_SIZE (-4)      /* unsupported image geometry */
#define ORBHIP_E_NODEVICE (-5)  /* no usable gfx950 device */

#define ORBHIP_MAX_LEVELS 16

/* Same 28-byte layout as cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id). */
typedef struct orbhip_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbhip_keypoint;

typedef struct orbhip_extractor orbhip_extractor;
typedef struct orbhip_matcher orbhip_matcher;

const char *orbhip_last_error(void);      /* thread-local text of the last failure */
int orbhip_device_count(int *count);

/* ---- ORBextractor ------------------------------------------------------- */

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (src/ORBextractor.cc:410-470) on HIP device `device`. */
int orbhip_extractor_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast,
                            int min_th_fast, int device, orbhip_extractor **out);
void orbhip_extractor_destroy(orbhip_extractor *e);

/* GetLevels/GetScaleFactor(s)/GetInverseScaleFactors/GetScaleSigmaSquares/
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:63-83); arrays of nlevels floats,
 * any pointer may be NULL.  feat_per_level = mnFeaturesPerLevel. */
int orbhip_extractor_levels(const orbhip_extractor *e);
int orbhip_extractor_tables(const orbhip_extractor *e, float *scale, float *inv_scale,
                            float *sigma2, float *inv_sigma2, int32_t *feat_per_level);

/* Upper bound of keypoints one frame can return for images of rows x cols
 * (per level: max(quota + 3, 4 * initial nodes), src/ORBextractor.cc:669-737). */
int orbhip_extractor_capacity(orbhip_extractor *e, int rows, int cols, int *cap);

/* 7-tap blur weights (default {18,34,49,55,49,34,18}: OpenCV<=3.3 integer kernel for
 * GaussianBlur(7x7, sigma 2) on 8U; out = sat((sum_v sum_u w_v w_u p + 2^15) >> 16)). */
int orbhip_extractor_set_blur_kernel(orbhip_extractor *e, const int32_t w[7]);

/* mvImagePyramid[0] on demand (include/ORBextractor.h:85; only Frame::ComputeStereoMatches, src/Frame.cc:563-580, ever
 * reads it -- a monocular Tracking thread never does).  on != 0: extractions stop writing the padded level-0 plane
 * (copyMakeBorder of the image, src/ORBextractor.cc:1127); FAST and the descriptor kernel read level 0 from the caller's
 * image (BORDER_REFLECT_101 by index where a border keypoint's window overshoots it), results are bit-identical.  The
 * first accessor that needs the plane afterwards (orbhip_pyramid_level / _download / orbhip_blurred_level_download for
 * level 0, orbhip_compute_stereo_matches*) writes it then, from the image buffer of the last extraction: callers of
 * orbhip_extract_batch_device must leave that buffer untouched until then (host entry points keep their own copy, and
 * so do the colour entries orbhip_extract_color*: their level 0 comes from the handle's grey frames).
 * Default 0: every extraction materialises it, as the reference does. */
int orbhip_extractor_set_lazy_level0(orbhip_extractor *e, int on);

/* Several extractor handles on several streams (the reference runs two on two threads for a stereo sensor,
 * src/Frame.cc:78-81; a batch front-end runs a few pipelines side by side): which of their kernels meet on the GPU decides
 * how well they share it, and free-running streams settle into one of several phase patterns.  A stage gate pins the
 * pattern: before launching stage `stage` (0 pyramid, 1 FAST, 2 octree, 3 descriptors) the handle's stream waits for
 * `wait_event` (hipEvent_t, null = no wait), after it `record_event` is recorded (null = none).  Chaining the FAST stages
 * of N handles in a ring (handle h waits for the event handle h-1 records) keeps the N VALU-bound FAST kernels from
 * running beside each other.  Events are owned by the caller and must outlive their use; results never depend on gates.
 * ORBHIP_GATE_KEEP for either event leaves that side of the stage's gate as it is. */
#define ORBHIP_GATE_KEEP ((void *)(intptr_t)-1)
int orbhip_extractor_set_stage_gate(orbhip_extractor *e, int stage, void *wait_event, void *record_event);

/* ORBextractor::operator()(image, mask(ignored), keypoints, descriptors)
 * (src/ORBextractor.cc:1043-1105).  image: rows x cols uint8, row stride `stride` bytes (host).
 * kps[cap], desc[cap*32] host buffers; *n = number of keypoints (0 is success). */
int orbhip_extract(orbhip_extractor *e, const uint8_t *image, int rows, int cols, int stride,
                   orbhip_keypoint *kps, uint8_t *desc, int cap, int *n);

/* Batch of `batch` same-size frames, host buffers.  Frame b starts at
 * images + b*frame_stride; outputs of frame b at kps + b*cap, desc + b*cap*32, n[b].
 * ORBHIP_E_CAPACITY (cap smaller than orbhip_extractor_capacity()): every frame's n[b] <= cap and its first n[b]
 * keypoints / descriptors are still delivered (truncated in output order) before the error is returned. */
int orbhip_extract_batch(orbhip_extractor *e, const uint8_t *images, int batch, int rows, int cols,
                         int stride, size_t frame_stride, orbhip_keypoint *kps, uint8_t *desc,
                         int cap, int32_t *n);

/* Same with device pointers; asynchronous on the handle's stream. d_n: int32[batch].
 * d_status: int32[batch] (0 ok, ORBHIP_E_CAPACITY if cap was too small), may be NULL. */
int orbhip_extract_batch_device(orbhip_extractor *e, const void *d_images, int batch, int rows,
                                int cols, int stride, size_t frame_stride, void *d_kps,
                                void *d_desc, int cap, void *d_n, void *d_status);

/* ---- colour input ----
 * Tracking::GrabImage{Monocular,Stereo,RGBD} turn a 3- or 4-channel frame into grey with cvtColor(CV_RGB2GRAY /
 * CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY), chosen by the channel count and Camera.RGB (src/Tracking.cc:103-109,
 * 172-197, 212-225, 242-256), before the extractor sees it.  The orbhip_extract_color* entries do that conversion on the
 * device, into a grey buffer the handle owns, and run the unchanged pipeline on it:
 *     Y = min(255, (R*wR + G*wG + B*wB + (1 << (shift-1))) >> shift)
 * with wR, wG, wB = 4899, 9617, 1868 and shift = 14 by default: the integer RGB2Gray<uchar> of OpenCV 2.4 - 3.3, restated
 * from the published algorithm; parity with a given OpenCV build is unpinned.  A shim linked against
 * another OpenCV installs that build's table: 0 <= w < 65536, 1 <= shift <= 16 (ORBHIP_E_ARG otherwise). */
#define ORBHIP_COLOR_BGR 0
#define ORBHIP_COLOR_RGB 1          /* = Camera.RGB (src/Tracking.cc:103-104) */
int orbhip_extractor_set_gray_weights(orbhip_extractor *e, const int32_t w_rgb[3], int shift);

/* image: rows x cols pixels of `channels` (3 or 4) interleaved uint8, row stride `stride` bytes >= cols*channels; rgb:
 * ORBHIP_COLOR_RGB = byte 0 of a pixel is R, ORBHIP_COLOR_BGR = byte 0 is B; a fourth channel is ignored.  Anything else
 * about the call is orbhip_extract / orbhip_extract_batch / orbhip_extract_batch_device: outputs, capacity rule, an empty
 * host image gives zero keypoints.  channels other than 3 or 4 (1 is not an alias of the grey entries), a short stride or
 * a null pointer: ORBHIP_E_ARG before any device work.  No more than the last byte a frame's pixels occupy,
 * (rows-1)*stride + cols*channels, is read.
 * The host entries upload the packed colour bytes with one 1-D copy from page-locked staging the handle owns; they launch
 * eagerly and in one chunk (the graph replay and the chunk pipeline of the grey host entries are not reproduced).
 * The conversion belongs to stage 0: it runs behind that stage's gate (orbhip_extractor_set_stage_gate) and
 * orbhip_extractor_stage_times [0] includes it.
 * After a colour extraction the grey frames are "the image of the last extraction": every accessor
 * (orbhip_pyramid_level*, orbhip_blurred_level_download, orbhip_level_candidates, orbhip_compute_stereo_matches*) works
 * as after a grey one, and the level-0 ROI is the converted image.  With orbhip_extractor_set_lazy_level0 the level-0
 * plane is written later from the handle's grey frames, NOT from the caller's buffer: the lifetime rule stated there does
 * not apply to colour input, the colour buffer may be reused as soon as the work enqueued by the call has run (stream
 * order is enough). */
int orbhip_extract_color(orbhip_extractor *e, const uint8_t *image, int rows, int cols, int channels, int rgb, int stride,
                         orbhip_keypoint *kps, uint8_t *desc, int cap, int *n);
int orbhip_extract_color_batch(orbhip_extractor *e, const uint8_t *images, int batch, int rows, int cols, int channels,
                               int rgb, int stride, size_t frame_stride, orbhip_keypoint *kps, uint8_t *desc, int cap,
                               int32_t *n);
int orbhip_extract_color_batch_device(orbhip_extractor *e, const void *d_images, int batch, int rows, int cols,
                                      int channels, int rgb, int stride, size_t frame_stride, void *d_kps, void *d_desc,
                                      int cap, void *d_n, void *d_status);

/* ---- stereo rectification ----
 * Examples/Stereo/stereo_euroc.cc:63-98 builds two map pairs with cv::initUndistortRectifyMap(K, D, R, P(0:3,0:3), size,
 * CV_32F, M1, M2) and sends every left and right frame through cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) (:136-137)
 * before TrackStereo.  Both are restated here from the published OpenCV 2.4 - 3.3 algorithms; parity with a given OpenCV
 * build is unpinned.
 *
 * orbhip_init_undistort_rectify_map: host code, needs no device.  K, R, P3x3: row-major 3x3 doubles (P3x3 = the left 3x3 of
 * the 3x4 projection matrix; R may be NULL = identity); D: nD = 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]];
 * map1 / map2: rows x cols floats (x and y source coordinate of every destination pixel).  fp64 throughout,
 * iR = (P3x3 * R)^-1 by the adjugate, the homogeneous coordinates advance along a row by repeated addition, one rounding
 * to float at the end. */
int orbhip_init_undistort_rectify_map(const double K[9], const double *D, int nD, const double *R, const double P3x3[9],
                                      int cols, int rows, float *map1, float *map2);

/* Install (map1, map2: dst_rows x dst_cols floats, as above) or remove (both NULL) the remap of a handle.  The maps are
 * turned into what cv::remap computes from them for INTER_LINEAR on 8-bit data: sx = cvRound(map1 * 32), sy =
 * cvRound(map2 * 32) (round half to even, saturated to int; NaN counts as outside the source), integer tap (sx >> 5,
 * sy >> 5), weight row (sy & 31) * 32 + (sx & 31); the per-pixel records live on the device, belong to the handle and
 * serve every frame of every later batch.  1 <= src_rows, src_cols <= 32767, src_rows * src_cols < 2^31. */
int orbhip_extractor_set_remap(orbhip_extractor *e, int dst_rows, int dst_cols, int src_rows, int src_cols, const float *map1,
                               const float *map2);
/* The 1024 x 4 weight table is data: row (fy * 32 + fx) holds the weights of the taps (x, y), (x+1, y), (x, y+1),
 * (x+1, y+1).  Default: (32 - fx | fx) * (32 - fy | fy) * 32, the published fixed-point table of initInterTab2D, every
 * row summing to 32768 (row 0 is 32768, 0, 0, 0: DESIGN.md section 3).  0 <= w <= 65535; NULL restores the default. */
#define ORBHIP_REMAP_TABLE_SIZE 4096
int orbhip_extractor_set_remap_table(orbhip_extractor *e, const int32_t *w);

/* image: rows x cols uint8 grey source pixels (the RAW camera frame; rows, cols must equal the src_rows, src_cols of the
 * installed map), row stride `stride` bytes >= cols.  The device computes, for every pixel of the dst_rows x dst_cols
 * rectified image,
 *     min(255, (sum of 4 taps * weights + (1 << 14)) >> 15),    a tap outside the source = 0 (BORDER_CONSTANT, value 0)
 * into grey frames the handle owns and runs the unchanged pipeline on them; cap, outputs and the capacity rule are those
 * of orbhip_extract* at dst_rows x dst_cols.
 * Grey input only: channels must be 1.  A colour frame (channels 3 or 4) is ORBHIP_E_ARG; convert it first.
 * No map installed, a size other than the map's source size, a short stride or a null pointer: ORBHIP_E_ARG before any
 * device work; an empty host image gives zero keypoints.  No more than (rows-1)*stride + cols bytes of a frame are read.
 * Host entries: one 1-D upload from page-locked staging, eager launches, one chunk (as orbhip_extract_color*).  The remap
 * belongs to stage 0.  Afterwards the rectified frames are "the image of the last extraction" for every accessor
 * (orbhip_pyramid_level*, a lazy level 0, orbhip_compute_stereo_matches*), and the caller's buffer may be reused as soon
 * as the work enqueued by the call has run (stream order is enough). */
int orbhip_extract_remap(orbhip_extractor *e, const uint8_t *image, int rows, int cols, int channels, int stride,
                         orbhip_keypoint *kps, uint8_t *desc, int cap, int *n);
int orbhip_extract_remap_batch(orbhip_extractor *e, const uint8_t *images, int batch, int rows, int cols, int channels,
                               int stride, size_t frame_stride, orbhip_keypoint *kps, uint8_t *desc, int cap, int32_t *n);
int orbhip_extract_remap_batch_device(orbhip_extractor *e, const void *d_images, int batch, int rows, int cols, int channels,
                                      int stride, size_t frame_stride, void *d_kps, void *d_desc, int cap, void *d_n,
                                      void *d_status);

int orbhip_extractor_sync(orbhip_extractor *e);
void *orbhip_extractor_stream(orbhip_extractor *e); /* hipStream_t */
/* Launch on a caller-owned hipStream_t instead (NULL: back to the handle's own stream). */
int orbhip_extractor_set_stream(orbhip_extractor *e, void *stream);

/* mvImagePyramid[level] of frame `frame` of the last extract call: size and device pointer of
 * the level ROI (valid until the next extract on this handle); row stride in bytes.  The ROI is
 * surrounded by the 19-px BORDER_REFLECT_101 frame the reference allocates
 * (src/ORBextractor.cc:1113-1128), so d_roi[-19*stride-19] is addressable.
 * Frame rule: an extraction writes a level's interior and only the inner 8 px of its frame (level 0 of a handle with
 * orbhip_extractor_set_lazy_level0: nothing).  The rest of the frames is written by the first call after the extraction
 * that can read it -- this one when d_roi is asked for (enqueued on the handle's stream), orbhip_pyramid_level_download
 * with_border, orbhip_blurred_level_download -- so the ROI's surrounding frame is valid from this call on, for every
 * frame and level of the batch, until the next extraction.  A pointer kept from before that extraction addresses the
 * same plane, whose frame is then stale until one of these calls is made again.  orbhip_compute_stereo_matches* does
 * not need the frames of the levels >= 1 for keypoints the handles' extraction produced (16 px inside their level), and
 * does not ask for them. */
int orbhip_pyramid_level(orbhip_extractor *e, int frame, int level, int *rows, int *cols,
                         int *stride, const void **d_roi);
/* Copy a level to host.  with_border != 0 copies the (rows+38)x(cols+38) padded plane. */
int orbhip_pyramid_level_download(orbhip_extractor *e, int frame, int level, int with_border,
                                  uint8_t *dst, int dst_stride);
/* Debug/parity taps of the last call (host copies).  The blurred planes are not part of the pipeline (only the
 * keypoints' patches are blurred, inside the descriptor kernel): the first request after an extraction runs the
 * 7x7 Gaussian blur over the whole pyramid of the last batch. */
int orbhip_blurred_level_download(orbhip_extractor *e, int frame, int level, uint8_t *dst,
                                  int dst_stride);
/* FAST candidates of a level in reference order: x,y (relative to minBorder), score. */
int orbhip_level_candidates(orbhip_extractor *e, int frame, int level, int32_t *x, int32_t *y,
                            int32_t *score, int cap, int *n);
/* Host only, no device: the FAST kernel's cell records for an image size, six int32 per cell in table order -- level,
 * sub-image width and height (detection rectangle + 6), the row multiplier ceil(2^18 / groups of four columns), the
 * work items of a row band that cannot overflow the survivor list, the multiplier ceil(2^20 / detection columns) of
 * the banded non-maximum suppression -- and the survivor-list capacity they were made for.  *n is the number of cells;
 * ORBHIP_E_CAPACITY when cap is smaller (the first cap records are written). */
int orbhip_fast_cell_table(int nfeatures, float scale_factor, int nlevels, int rows, int cols,
                           int32_t *rec, int cap, int *n, int *list_cap);

/* Per-stage device time, microseconds, averaged over the extract calls made since
 * orbhip_extractor_set_profiling(e, 1) (at most the last 256), measured with HIP events on the
 * handle's stream: [0] pyramid (7 launches), [1] FAST+NMS cells, [2] octree, [3] always 0 (the separate blur stage of
 * round 1: the descriptor kernel blurs the patches it samples, nothing is launched or timed there), [4] blur of the
 * patches + orientation + descriptors, [5] whole call. */
int orbhip_extractor_set_profiling(orbhip_extractor *e, int on);
int orbhip_extractor_stage_times(orbhip_extractor *e, float us[6]);

/* ---- ORBmatcher --------------------------------------------------------- */

/* Flat view of the Frame fields the matchers read (include/Frame.h). Host pointers. */
typedef struct orbhip_frame_view {
    int32_t n;                       /* N */
    const orbhip_keypoint *keys;     /* mvKeysUn */
    const uint8_t *desc;             /* mDescriptors, n x 32 */
    const float *u_right;            /* mvuRight or NULL (monocular: all -1) */
    float min_x, min_y, max_x, max_y; /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    float grid_inv_w, grid_inv_h;    /* mfGridElementWidthInv, mfGridElementHeightInv */
    int32_t n_levels;
    const float *scale_factors;      /* mvScaleFactors */
} orbhip_frame_view;

/* One already-projected query of SearchByProjection (the shim does the projection with the
 * reference's own cv::Mat arithmetic, src/ORBmatcher.cc:1360-1390 / src/Frame.cc:269-325). */
typedef struct orbhip_query {
    int32_t valid;        /* 0: skipped (no map point, outlier, bad, not in view, behind camera) */
    float u, v;           /* projection in the searched frame */
    float radius;         /* window half-size in px (th * scale[level], src/ORBmatcher.cc:1381,:69) */
    int32_t min_level, max_level; /* GetFeaturesInArea level window (max_level -1 = open) */
    float ur;             /* projected right-image coordinate (stereo consistency check) */
    int32_t level_aux;    /* informational */
    float angle;          /* angle of the query keypoint (rotation histogram) */
    int32_t observed;     /* pMP->Observations() > 0: once assigned it blocks that slot */
} orbhip_query;

int orbhip_matcher_create(int device, orbhip_matcher **out);
void orbhip_matcher_destroy(orbhip_matcher *m);

/* Batched DescriptorDistance: dist[i*nb + j] = popcount(a_i xor b_j) (host buffers). */
int orbhip_descriptor_distance(orbhip_matcher *m, const uint8_t *a, int na, const uint8_t *b,
                               int nb, int32_t *dist);

/* ORBmatcher::SearchForInitialization(F1,F2,vbPrevMatched,vnMatches12,windowSize) with
 * mfNNratio = nnratio, mbCheckOrientation = check_ori.  prev_matched_xy: n1 x 2 floats, in/out.
 * matches12: n1 int32 out. */
int orbhip_search_for_initialization(orbhip_matcher *m, const orbhip_frame_view *f1,
                                     const orbhip_frame_view *f2, float *prev_matched_xy,
                                     int32_t *matches12, int window_size, float nnratio,
                                     int check_ori, int *nmatches);

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) after projection.
 * q[nq], qdesc[nq*32] = pMP->GetDescriptor(); taken[n] (may be NULL): slot already holds an
 * observed map point.  assign[n] out: query index now held by each current keypoint or -1.
 * Sizes (this and the points / keyframe / sim3 forms below): any n and nq.  Queries with valid == 0 are dropped
 * on the host before anything is staged (a local map or a loop-closing point set is mostly such entries); up to
 * 4096 train keypoints and 4096 VALID queries the resolve state is LDS resident, beyond that it moves to an HBM
 * workspace (slower, same results).  Only orbhip_search_for_initialization keeps a hard limit (4096 keypoints per
 * frame, ORBHIP_E_CAPACITY beyond): its match stealing is replayed by one wavefront over LDS state. */
int orbhip_search_by_projection_frame(orbhip_matcher *m, const orbhip_frame_view *cur,
                                      const orbhip_query *q, const uint8_t *qdesc, int nq,
                                      const uint8_t *taken, int32_t *assign, int check_ori,
                                      int *nmatches);

/* ORBmatcher::SearchByProjection(F, vpMapPoints, th) after Frame::isInFrustum. */
int orbhip_search_by_projection_points(orbhip_matcher *m, const orbhip_frame_view *f,
                                       const orbhip_query *q, const uint8_t *qdesc, int nq,
                                       const uint8_t *taken, int32_t *assign, float nnratio,
                                       int *nmatches);

/* ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) after projection
 * (src/ORBmatcher.cc:1490-1527 stay in the caller: valid = map point exists, !isBad(), not in sAlreadyFound, projects
 * inside the image and inside its scale-invariance range; radius = th*scale[predicted]; levels [pred-1, pred+1]).
 * taken[n]: CurrentFrame.mvpMapPoints[i2] != NULL on entry.  Every accepted match blocks its slot (:1538-1539);
 * accept iff best distance <= orb_dist (:1552); rotation histogram as in the frame-to-frame search. */
int orbhip_search_by_projection_keyframe(orbhip_matcher *m, const orbhip_frame_view *cur, const orbhip_query *q,
                                         const uint8_t *qdesc, int nq, const uint8_t *taken, int32_t *assign,
                                         int orb_dist, int check_ori, int *nmatches);

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) after the Sim3 projection (:315-359 stay in the
 * caller; radius = th*scale[pred], levels [pred-1, pred]).  kf: the KeyFrame's keypoints/descriptors/grid;
 * matched[n]: vpMatched[idx] != NULL on entry; accept iff best distance <= TH_LOW (:393); no orientation check. */
int orbhip_search_by_projection_sim3(orbhip_matcher *m, const orbhip_frame_view *kf, const orbhip_query *q,
                                     const uint8_t *qdesc, int nq, const uint8_t *matched, int32_t *assign,
                                     int *nmatches);

/* Independent best match per query (no slot blocking): the search loop of ORBmatcher::Fuse(pKF, vpMapPoints, th)
 * (src/ORBmatcher.cc:893-950), Fuse(pKF, Scw, ...) (:1045-1075) and of both directions of SearchBySim3 (:1199-1219,
 * :1279-1299).  Candidates = KeyFrame::GetFeaturesInArea(u, v, radius) with octave in [min_level, max_level]
 * (= [pred-1, pred]); chi2_gate != 0 adds Fuse's reprojection gate (e2*mvInvLevelSigma2[level] > 5.99 mono / 7.8
 * when mvuRight[idx] >= 0, using q.ur).  best_idx[nq] (-1 if no candidate), best_dist[nq] (256 if none): the caller
 * applies its threshold (TH_LOW / TH_HIGH) and the map-graph side effects in order. */
int orbhip_search_best_in_window(orbhip_matcher *m, const orbhip_frame_view *kf, const orbhip_query *q,
                                 const uint8_t *qdesc, int nq, int chi2_gate, const float *inv_level_sigma2,
                                 int32_t *best_idx, int32_t *best_dist);

/* Vocabulary-guided matching.  The DBoW2 vocabulary lookup (Frame::ComputeBoW, src/Frame.cc:395-403) stays with
 * the caller; what arrives here is the FeatureVector flattened to one node id per keypoint (node1[n1], node2[n2]:
 * the NodeId at levelsup = 4 that DBoW2 stored the feature under, ORBHIP_NO_NODE if absent).  Node lists are visited
 * in ascending node id and ascending feature index, which is how DBoW2 builds and std::map iterates them.
 *
 * orbhip_search_by_bow: for every f1 keypoint with valid1 != 0 (map point exists and is not bad; null = all), best
 * and second-best Hamming distance among the f2 keypoints of the same node that are neither blocked2 (null = none;
 * key-frame overload: "no good map point in pKF2") nor matched by an earlier f1 keypoint; accepted when
 * best <= max_dist (TH_LOW = 50 for the Frame overload :262, 49 for the key-frame overload's strict "<" :598) and
 * (float)best < nnratio*(float)second; rotation-histogram cull when check_ori.  matches12[n1] = f2 index or -1
 * (the Frame overload's vpMapPointMatches[idx2] = map point of idx1 is the inverse of this 1:1 map).
 * No size limit beyond memory (one wavefront per common node). */
#define ORBHIP_NO_NODE 0xffffffffu
int orbhip_search_by_bow(orbhip_matcher *m, const orbhip_frame_view *f1, const uint32_t *node1, const uint8_t *valid1,
                         const orbhip_frame_view *f2, const uint32_t *node2, const uint8_t *blocked2, int max_dist,
                         float nnratio, int check_ori, int32_t *matches12, int *nmatches);

/* Device-resident, batched orbhip_search_by_bow: pair p matches frame f1_first + p*f1_step of the first set of
 * arrays (the key-frame side) against frame f2_first + p*f2_step of the second set; both sets are in the layout the
 * extractor and orbhip_vocabulary_transform_device write (d_kps [frames][cap] orbhip_keypoint, d_desc [frames][cap][32],
 * d_n [frames] int32, d_node [frames][cap] uint32) and may be the same arrays; d_valid1 / d_blocked2 [frames][cap]
 * uint8 are optional (null).  Outputs d_matches12 [pairs][cap] int32, d_nmatches [pairs] int32.  One launch on the
 * matcher's stream, asynchronous; the (node, index) ordering, grouping, matching and rotation cull all happen on
 * the device.  cap <= 4096. */
int orbhip_search_by_bow_device(orbhip_matcher *m, int pairs, int cap, const void *d_kps1, const void *d_desc1,
                                const void *d_n1, const void *d_node1, const void *d_valid1, int f1_first, int f1_step,
                                const void *d_kps2, const void *d_desc2, const void *d_n2, const void *d_node2,
                                const void *d_blocked2, int f2_first, int f2_step, int max_dist, float nnratio,
                                int check_ori, void *d_matches12, void *d_nmatches);

/* ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823).  valid1 / valid2: keypoint has no map point yet
 * (null = all); stereo flags come from the views' u_right (>= 0, null = monocular); f12: the fundamental matrix of
 * LocalMapping::ComputeF12 (src/LocalMapping.cc:536-553) row-major; (ex, ey): epipole of camera 1 in image 2
 * (:664-670); level_sigma2[f2->n_levels] = pKF2->mvLevelSigma2; f2->scale_factors must be set.  Candidates of the
 * same node with Hamming distance <= TH_LOW that pass the epipole gate (:741-747) and CheckDistEpipolarLine
 * (:140-157); smallest distance wins, the later index on ties (":735 dist>bestDist"); the reference never sets
 * vbMatched2, so queries do not block each other.  matches12[n1] = f2 index or -1 (vMatchedPairs = the non-negative
 * entries in index order).  n1, n2 <= 4096 (ORBHIP_E_CAPACITY otherwise). */
int orbhip_search_for_triangulation(orbhip_matcher *m, const orbhip_frame_view *f1, const uint32_t *node1,
                                    const uint8_t *valid1, const orbhip_frame_view *f2, const uint32_t *node2,
                                    const uint8_t *valid2, const float *f12, float ex, float ey,
                                    const float *level_sigma2, int only_stereo, int check_ori, int32_t *matches12,
                                    int *nmatches);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307), batched: map point p owns the observed
 * descriptors desc[offsets[p] .. offsets[p+1]) (32 bytes each, in the order the reference collects them, i.e.
 * std::map<KeyFrame*,size_t> order without bad key frames).  best_idx[p] = index inside that range of the descriptor
 * with the least median Hamming distance to the others (vDists[0.5*(N-1)], first minimum), -1 for an empty range.
 * At most 2048 observations per map point (ORBHIP_E_CAPACITY otherwise). */
int orbhip_distinctive_descriptors(orbhip_matcher *m, const uint8_t *desc, const int32_t *offsets, int npoints,
                                   int32_t *best_idx);

/* ---- Frame constructor glue either side of the path (rectified / undistorted cameras) -------------------------
 * Frame::AssignFeaturesToGrid (src/Frame.cc:230-245, PosInGrid :382-392): the 64 x 48 grid mGrid as CSR in the order
 * GetFeaturesInArea walks it.  cell c = posX*48 + posY; cell_of[n] = c or -1 (PosInGrid rejects the keypoint);
 * cell_start[64*48 + 1]; cell_items[n] (the first cell_start[3072] entries are used): keypoint indices of every cell
 * in push_back (ascending) order.  f->keys are mvKeysUn.  n <= 4096. */
int orbhip_assign_features_to_grid(orbhip_matcher *m, const orbhip_frame_view *f, int32_t *cell_of, int32_t *cell_start,
                                   int32_t *cell_items);
/* device-resident, batched: d_kps [frames][cap], d_n [frames]; outputs d_cell_of / d_cell_items [frames][cap] int32,
 * d_cell_start [frames][3073] int32.  cap <= 4096.  Asynchronous on the matcher's stream. */
int orbhip_assign_features_to_grid_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap,
                                          float min_x, float min_y, float grid_inv_w, float grid_inv_h, void *d_cell_of,
                                          void *d_cell_start, void *d_cell_items);
/* Frame::UndistortKeyPoints (src/Frame.cc:404-434): keys_un = keys with pt replaced by
 * cv::undistortPoints(pt, mK, mDistCoef, R = I, P = mK); dist5 = {k1, k2, p1, p2, k3} (mDistCoef, src/Tracking.cc:66-81,
 * k3 = 0 when absent); dist5[0] == 0 copies the input (:406-410).  cv::undistortPoints is restated from the published
 * algorithm of OpenCV 2.4 - 3.3 (double arithmetic, 5 fixed-point iterations): parity with a given OpenCV build is
 * unpinned.  The four image corners of Frame::ComputeImageBounds (:436-463) go through the same call. */
int orbhip_undistort_keypoints(orbhip_matcher *m, const orbhip_keypoint *keys, int n, float fx, float fy, float cx, float cy,
                               const float *dist5, orbhip_keypoint *keys_un);
/* device-resident, batched: d_kps / d_kps_un [frames][cap] (may be the same array), d_n [frames] */
int orbhip_undistort_keypoints_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap, float fx,
                                      float fy, float cx, float cy, const float *dist5, void *d_kps_un);
/* Frame::ComputeStereoFromRGBD (src/Frame.cc:643-664): depth = CV_32F image (rows x cols, stride in floats), sampled at
 * the truncated coordinates of keys (mvKeys); u_right[i] = keys_un[i].x - mbf/d, depth_out[i] = d where d > 0, else
 * -1 / -1.  keys_un null = keys.  A keypoint outside the image reads d = 0 (the reference would read out of bounds). */
int orbhip_compute_stereo_from_rgbd(orbhip_matcher *m, const orbhip_keypoint *keys, const orbhip_keypoint *keys_un, int n,
                                    const float *depth, int rows, int cols, int stride_floats, float mbf, float *u_right,
                                    float *depth_out);
/* device-resident, batched: frame f reads d_depth + f * frame_stride_floats; d_kps_un null = d_kps */
int orbhip_compute_stereo_from_rgbd_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_kps_un,
                                           const void *d_n, int cap, const void *d_depth, int rows, int cols,
                                           int stride_floats, size_t frame_stride_floats, float mbf, void *d_u_right,
                                           void *d_depth_out);
/* The same on the depth image as the sensor delivers it (src/Tracking.cc:227-228 in front of src/Frame.cc:643-664):
 * depth_type ORBHIP_DEPTH_U16 (CV_16U, e.g. TUM's PNGs) or ORBHIP_DEPTH_F32; stride_elems in elements.  depth_factor =
 * mDepthMapFactor as the Tracking constructor leaves it (1 / DepthMapFactor, 1 when the setting is below 1e-5;
 * src/Tracking.cc:140-147).  U16: d = (float)raw * depth_factor always; F32: d = raw * depth_factor iff
 * fabs(depth_factor - 1.0f) > 1e-5, else d = raw.  One rounding of the product, as convertTo(CV_32F, factor) does per
 * pixel (stated choice): only the N sampled values are converted, no float image exists. */
#define ORBHIP_DEPTH_U16 0
#define ORBHIP_DEPTH_F32 1
int orbhip_compute_stereo_from_rgbd_raw(orbhip_matcher *m, const orbhip_keypoint *keys, const orbhip_keypoint *keys_un, int n,
                                        const void *depth, int depth_type, int rows, int cols, int stride_elems,
                                        float depth_factor, float mbf, float *u_right, float *depth_out);
int orbhip_compute_stereo_from_rgbd_raw_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_kps_un,
                                               const void *d_n, int cap, const void *d_depth, int depth_type, int rows,
                                               int cols, int stride_elems, size_t frame_stride_elems, float depth_factor,
                                               float mbf, void *d_u_right, void *d_depth_out);

/* ---- DBoW2 vocabulary: ORBVocabulary::loadFromTextFile + transform ---------------------------------------------
 * Replaces, for Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:395-402, src/KeyFrame.cc ComputeBoW), the
 * calls mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4) into
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1199 (+ :1218-1262 per feature, BowVector.cpp:36-88,
 * FeatureVector.cpp:31-46, FORB.cpp:81-101).  scoring / weighting use DBoW2's enum values (BowVector.h:36-53:
 * scoring 0 L1_NORM .. 5 DOT_PRODUCT; weighting 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; ORBvoc.txt is "10 6 0 0"). */
typedef struct orbhip_vocabulary orbhip_vocabulary;

/* Text format of TemplatedVocabulary::loadFromTextFile (:1338-1424): first line "k L scoring weighting", then one
 * line per node "parent isLeaf d0 .. d31 weight" (node ids in file order from 1, root = 0, word ids in order of the
 * leaf lines).  Blank lines are skipped (the reference turns the empty line after the final newline into an extra
 * root child with an uninitialised descriptor). */
int orbhip_vocabulary_load_text(const char *path, int device, orbhip_vocabulary **out);
/* The same tree from arrays: entry i describes node i+1; parent[i] in [0, i]. */
int orbhip_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent,
                             const uint8_t *is_leaf, const uint8_t *desc, const double *weight, int device,
                             orbhip_vocabulary **out);
void orbhip_vocabulary_destroy(orbhip_vocabulary *v);
/* any output pointer may be null; n_nodes counts the root */
int orbhip_vocabulary_info(const orbhip_vocabulary *v, int *k, int *L, int *scoring, int *weighting, int *n_nodes,
                           int *n_words);
int orbhip_vocabulary_set_stream(orbhip_vocabulary *v, void *hip_stream);   /* null = the handle's own stream */
int orbhip_vocabulary_sync(orbhip_vocabulary *v);

/* transform(features, BowVector, FeatureVector, levelsup) for n descriptors (n x 32 bytes, n <= 8192).
 * Per feature (each array n entries, nullable): word_id, word_weight, node_id = the FeatureVector node (ancestor at
 * level L - levelsup, 0 = root when levelsup >= L) or ORBHIP_NO_NODE when the word is stopped (weight <= 0); this is
 * the node1 / node2 input of orbhip_search_by_bow.  BowVector: bow_ids ascending with bow_vals (capacity n each,
 * nullable), *n_bow entries; values are accumulated and normalised in the reference's order, so they are
 * bit-identical doubles. */
int orbhip_vocabulary_transform(orbhip_vocabulary *v, const uint8_t *desc, int n, int levelsup, uint32_t *word_id,
                                double *word_weight, uint32_t *node_id, uint32_t *bow_ids, double *bow_vals, int *n_bow);
/* Device-resident, batched: descriptors in the extractor's output layout d_desc [frames][cap][32] with d_n [frames]
 * int32 counts; outputs d_word_id / d_node_id / d_bow_ids [frames][cap] uint32, d_word_weight / d_bow_vals
 * [frames][cap] double, d_n_bow [frames] int32.  Asynchronous on the handle's stream.  cap <= 8192. */
int orbhip_vocabulary_transform_device(orbhip_vocabulary *v, int frames, const void *d_desc, const void *d_n, int cap,
                                       int levelsup, void *d_word_id, void *d_word_weight, void *d_node_id,
                                       void *d_bow_ids, void *d_bow_vals, void *d_n_bow);

/* Device-resident, batched forms of the two SearchByProjection searches: `pairs` independent frame pairs,
 * asynchronous on the matcher's stream.  Train side in the extractor's output layout: d_kps [pairs][cap]
 * orbhip_keypoint, d_desc [pairs][cap][32], d_n [pairs] int32; optional d_u_right [pairs][cap] float and
 * d_taken [pairs][cap] uint8.  Query side: d_q [pairs][qcap] orbhip_query, d_qdesc [pairs][qcap][32],
 * d_nq [pairs] int32.  The image bounds / grid scale are shared (one camera).  Outputs: d_assign [pairs][cap]
 * int32 (query index held by each keypoint or -1), d_nmatches [pairs] int32.  No size limit: up to 4096 keypoints
 * and queries the resolve state is LDS resident, beyond that it lives in an HBM workspace (slower, same results). */
int orbhip_search_by_projection_frame_device(orbhip_matcher *m, int pairs, const void *d_kps, const void *d_desc,
                                             const void *d_n, int cap, const void *d_u_right, const void *d_taken,
                                             float min_x, float min_y, float grid_inv_w, float grid_inv_h,
                                             const void *d_q, const void *d_qdesc, const void *d_nq, int qcap,
                                             int check_ori, void *d_assign, void *d_nmatches);
int orbhip_search_by_projection_points_device(orbhip_matcher *m, int pairs, const void *d_kps, const void *d_desc,
                                              const void *d_n, int cap, const void *d_u_right, const void *d_taken,
                                              float min_x, float min_y, float grid_inv_w, float grid_inv_h,
                                              const void *d_q, const void *d_qdesc, const void *d_nq, int qcap,
                                              float nnratio, void *d_assign, void *d_nmatches);
/* ORBmatcher::SearchForInitialization, device resident and batched (src/ORBmatcher.cc:405-520): pair p matches
 * F1 = frame f1_first + p*f1_step against F2 = frame f2_first + p*f2_step of the extractor output arrays.
 * d_prev_matched [pairs][cap][2] float = vbPrevMatched (in/out; reset_prev != 0 first sets it to F1's keypoint
 * positions, src/Tracking.cc:578-580); outputs d_matches12 [pairs][cap] int32 (vnMatches12) and d_nmatches [pairs].
 * One wavefront per pair replays the match-stealing loop.  cap <= 4096. */
int orbhip_search_for_initialization_device(orbhip_matcher *m, int pairs, const void *d_kps, const void *d_desc,
                                            const void *d_n, int cap, int f1_first, int f1_step, int f2_first,
                                            int f2_step, float min_x, float min_y, float grid_inv_w, float grid_inv_h,
                                            int reset_prev, void *d_prev_matched, int window_size, float nnratio,
                                            int check_ori, void *d_matches12, void *d_nmatches);

/* ---- projection prologues on the device -------------------------------------------
 * The arithmetic in front of the window search of the two SearchByProjection overloads.  The reference does it with
 * cv::Mat expressions (CV_32F); the operation order used here is stated in DESIGN.md section 3 (per row
 * ((r0*x + r1*y) + r2*z) + t in float without contraction; cv::norm / Mat::dot accumulate in double; logf of
 * MapPoint::PredictScale is a deterministic, correctly rounded log). */
typedef struct orbhip_camera {
    float fx, fy, cx, cy, mbf, mb;           /* Frame::fx, fy, cx, cy, mbf, mb (src/Frame.cc:104-112) */
    float min_x, max_x, min_y, max_y;        /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    int32_t n_levels;                        /* mnScaleLevels */
    float log_scale_factor;                  /* mfLogScaleFactor */
    float scale_factors[ORBHIP_MAX_LEVELS];  /* mvScaleFactors */
} orbhip_camera;
#define ORBHIP_POINT_PRESENT 1   /* the map point exists and takes part (frame search: pMP && !mvbOutlier[i];
                                    frustum: !isBad() and not already matched in this frame) */
#define ORBHIP_POINT_OBSERVED 2  /* pMP->Observations() > 0 */

/* Prologue of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1339-1390:
 * Tcw / Tlw = top three rows of CurrentFrame.mTcw / LastFrame.mTcw, row-major (12 floats); world [n][3] =
 * pMP->GetWorldPos() of LastFrame.mvpMapPoints[i]; flags [n] = ORBHIP_POINT_* bits; last_keys = LastFrame.mvKeysUn
 * (octave: :1379, angle: :1433).  q [n] out, ready for orbhip_search_by_projection_frame with
 * qdesc = the map points' descriptors.  Host buffers, synchronous. */
int orbhip_project_last_frame(orbhip_matcher *m, const orbhip_camera *cam, const float *Tcw, const float *Tlw, int n,
                              const float *world, const uint8_t *flags, const orbhip_keypoint *last_keys, float th,
                              int mono, orbhip_query *q);

/* Frame::isInFrustum(pMP, viewing_cos_limit) (src/Frame.cc:269-325) with MapPoint::PredictScale
 * (src/MapPoint.cc:400-418) for n map points of the local map, followed by the window of
 * SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:52-69, RadiusByViewingCos :131-137).  world / normal [n][3]
 * = GetWorldPos() / GetNormal(); max_dist / min_dist [n] = mfMaxDistance / mfMinDistance (the 1.2 / 0.8 factors of
 * Get{Max,Min}DistanceInvariance are applied here).  q[i].valid = mbTrackInView, u / v / ur / level_aux =
 * mTrackProjX / mTrackProjY / mTrackProjXR / mnTrackScaleLevel; view_cos [n] (nullable) = mTrackViewCos. */
int orbhip_frustum_queries(orbhip_matcher *m, const orbhip_camera *cam, const float *Tcw, int n, const float *world,
                           const float *normal, const float *max_dist, const float *min_dist, const uint8_t *flags,
                           float viewing_cos_limit, float th, orbhip_query *q, float *view_cos);

/* Prologue of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:853-888), Fuse(pKF, Scw, ...) (:1005-1048) and
 * of one direction of SearchBySim3 (:1155-1180 / :1235-1260): projection of n map points into a key frame, written
 * as orbhip_query records for orbhip_search_best_in_window (level window [pred-1, pred], radius th*scale[pred]).
 *   mode 0 (Fuse): T1 = [Rcw | tcw] (for the Sim3 overload the caller passes Rcw = sRcw/scw, tcw = t/scw, :1000-1003);
 *     gates: depth, KeyFrame::IsInImage, scale-invariance range on |X - Ow|, viewing angle PO.dot(Pn) >= 0.5*dist3D;
 *     q.ur = u - bf*invz for the stereo chi-square gate of the search.
 *   mode 1 (SearchBySim3): T1 = [R1w | t1w], T2 = [sR21 | t21] (the caller computes them as :1119-1121); gates: depth,
 *     IsInImage, range on |Pc2|; no normal.
 * double_invz: invz = 1.0/z evaluated in double (:1156, :1017) or 1/z in float (:862).  flags: ORBHIP_POINT_PRESENT =
 * map point exists, !isBad(), not IsInKeyFrame / not already matched.  max_dist / min_dist = mfMaxDistance /
 * mfMinDistance.  Host buffers, synchronous. */
int orbhip_keyframe_queries(orbhip_matcher *m, const orbhip_camera *cam, int mode, int double_invz, const float *T1,
                            const float *T2, int n, const float *world, const float *normal, const float *max_dist,
                            const float *min_dist, const uint8_t *flags, float th, orbhip_query *q);

/* ORBmatcher::Fuse up to the decision (src/ORBmatcher.cc:825-947 / :975-1075): prologue + best key point in the window
 * with the chi-square gate; best_idx[n] / best_dist[n] out (-1 / 256 when nothing passes).  The replace-or-add decision
 * (:949-971, :1077-1095: bestDist <= TH_LOW, pKF->GetMapPoint(bestIdx), Replace / AddObservation) touches the map
 * graph, depends on the order of the points and stays in the caller.  sim3_form != 0: the Scw overload (invz in double,
 * and no chi-square gate: its loop, :1062-1079, tests the level window only; inv_level_sigma2 is not read).
 * point_desc [n][32] = pMP->GetDescriptor(). */
int orbhip_fuse(orbhip_matcher *m, const orbhip_frame_view *kf, const orbhip_camera *cam, const float *Tcw, int sim3_form,
                int n, const float *world, const float *normal, const float *max_dist, const float *min_dist,
                const uint8_t *flags, const uint8_t *point_desc, float th, const float *inv_level_sigma2, int32_t *best_idx,
                int32_t *best_dist);

/* ORBmatcher::Fuse up to the decision for K key frames at once: what LocalMapping::SearchInNeighbors
 * (src/LocalMapping.cc:454-515: matcher.Fuse(pKFi, vpMapPointMatches) for every covisible key frame and second
 * neighbour) and LoopClosing::SearchAndFuse (src/LoopClosing.cc:585-610: one Sim3 per key frame) ask of
 * ORBmatcher::Fuse (src/ORBmatcher.cc:825-950 / :975-1075).  One set of map points, K targets, one launch; row k of the
 * outputs is bit-identical to one orbhip_fuse call with key frame k, Tcw[k] and flags[k].  The decision (:952-971) stays
 * in the caller, which applies the rows in key-frame order: the call sees the map as it is at call time (INTEGRATION.md,
 * "Fusing into many key frames").
 *
 * orbhip_fuse_device: device-resident, asynchronous on the matcher's stream, no host synchronisation, no staging copy.
 *   key frames: d_kf_index [K] int32; target k is frame row d_kf_index[k] (any order, gaps and repeats allowed) of
 *     d_kps [..][cap] (mvKeysUn), d_desc [..][cap][32], d_n [..] int32 and the optional d_u_right [..][cap] (mvuRight; NULL:
 *     monocular), in the extractor's output layout.  d_Tcw [K][12]: [Rcw | tcw] of target k; sim3_form != 0: the Scw
 *     overload, the caller passes Rcw = sRcw/scw, tcw = t/scw as for orbhip_fuse.
 *     d_cell_start [..][3073] / d_cell_items [..][cap]: mGrid of the same frame rows as
 *     orbhip_assign_features_to_grid_device writes it; both NULL: the call builds the grids of the K targets itself.
 *     The grid origin and scale are cam's (min_x, min_y, 64/(max_x-min_x), 48/(max_y-min_y)).
 *   map points (shared by all targets): np points in arrays of pcap entries: d_world / d_normal [pcap][3],
 *     d_max_dist / d_min_dist [pcap], d_point_desc [pcap][32]; d_flags [K][pcap] uint8, ORBHIP_POINT_PRESENT = good map
 *     point and !pMP->IsInKeyFrame(target k) (:849, one row per target).  inv_level_sigma2: host, cam->n_levels floats.
 *   outputs: d_best_idx / d_best_dist [K][pcap] int32 (-1 / 256 where nothing passes; entries >= np untouched);
 *     d_q [K][pcap] orbhip_query or NULL: the prologue's records (those of orbhip_keyframe_queries mode 0).
 *   cap <= 4096 (ORBHIP_E_CAPACITY beyond); K >= 0, 0 <= np <= pcap (ORBHIP_E_ARG otherwise); refused before any device
 *   work.  K == 0 or np == 0: success, nothing written.
 *
 * orbhip_fuse_batch: host buffers, synchronous; what a host-side LocalMapping thread calls.  kfs [K] key frames,
 *   Tcw [K][12], flags [K][n], best_idx / best_dist [K][n]; everything is staged in one copy, fused by one
 *   orbhip_fuse_device call that builds the grids, and read back in one copy.  A key frame with more than 4096 key points,
 *   or whose grid or level count differs from cam's, takes the orbhip_fuse path for its row. */
int orbhip_fuse_device(orbhip_matcher *m, int K, const void *d_kf_index, const orbhip_camera *cam, const void *d_Tcw,
                       int sim3_form, const void *d_kps, const void *d_desc, const void *d_n, int cap, const void *d_u_right,
                       const void *d_cell_start, const void *d_cell_items, int np, int pcap, const void *d_world,
                       const void *d_normal, const void *d_max_dist, const void *d_min_dist, const void *d_point_desc,
                       const void *d_flags, float th, const float *inv_level_sigma2, void *d_best_idx, void *d_best_dist,
                       void *d_q);
int orbhip_fuse_batch(orbhip_matcher *m, int K, const orbhip_frame_view *const *kfs, const orbhip_camera *cam,
                      const float *Tcw, int sim3_form, int n, const float *world, const float *normal,
                      const float *max_dist, const float *min_dist, const uint8_t *flags, const uint8_t *point_desc,
                      float th, const float *inv_level_sigma2, int32_t *best_idx, int32_t *best_dist);

/* ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1102-1326), complete: both projection directions, both searches
 * (accept bestDist <= TH_HIGH) and the mutual-agreement pass.  kf1 / kf2: the key frames' keypoints, descriptors and
 * grid; per key-frame slot i: world*[i], max/min_dist*[i], desc*[i] = the slot's map point (GetWorldPos,
 * mfMax/MinDistance, GetDescriptor), flags*[i] = ORBHIP_POINT_PRESENT iff the slot has a good map point that is not in
 * vpMatches12 already (:1132-1143).  matches12[n1] = matched kf2 slot or -1 (the caller sets vpMatches12[i1] =
 * vpMapPoints2[matches12[i1]]); *nfound = the return value. */
int orbhip_search_by_sim3(orbhip_matcher *m, const orbhip_frame_view *kf1, const orbhip_frame_view *kf2,
                          const orbhip_camera *cam, const float *T1w, const float *T2w, const float *S21, const float *S12,
                          const float *world1, const float *max_dist1, const float *min_dist1, const uint8_t *flags1,
                          const uint8_t *desc1, const float *world2, const float *max_dist2, const float *min_dist2,
                          const uint8_t *flags2, const uint8_t *desc2, float th, int32_t *matches12, int *nfound);

/* Device-resident, batched.  Frames live in the extractor's output layout (d_kps [frames][cap] orbhip_keypoint,
 * d_desc [frames][cap][32], d_n [frames] int32); pair p has CurrentFrame = frame cur_first + p*cur_step and
 * LastFrame = frame last_first + p*last_step.  d_Tcw / d_Tlw [pairs][12] float; d_world [frames][cap][3] float and
 * d_flags [frames][cap] uint8 are indexed by the LAST frame (one map point per last-frame keypoint).
 *
 * orbhip_project_last_frame_device writes d_q [pairs][cap] orbhip_query and d_nq [pairs] int32 (= the last frame's n).
 *
 * orbhip_track_last_frame_device = that prologue + SearchByProjection's search, resolve and rotation cull in one call
 * (Tracking::TrackWithMotionModel's matching step, src/Tracking.cc:880-885): the queries' descriptors are the last
 * frame's (the tracked map points were created from / last seen in it); optional d_u_right [frames][cap] float
 * (indexed by the current frame) and d_taken [pairs][cap] uint8; outputs d_assign [pairs][cap] int32 (last-frame
 * keypoint index now held by each current keypoint or -1), d_nmatches [pairs] int32. */
int orbhip_project_last_frame_device(orbhip_matcher *m, int pairs, const orbhip_camera *cam, const void *d_Tcw,
                                     const void *d_Tlw, const void *d_kps, const void *d_n, int cap, int last_first,
                                     int last_step, const void *d_world, const void *d_flags, float th, int mono,
                                     void *d_q, void *d_nq);
int orbhip_track_last_frame_device(orbhip_matcher *m, int pairs, const orbhip_camera *cam, const void *d_Tcw,
                                   const void *d_Tlw, const void *d_kps, const void *d_desc, const void *d_n, int cap,
                                   int cur_first, int cur_step, int last_first, int last_step, const void *d_world,
                                   const void *d_flags, const void *d_u_right, const void *d_taken, float th, int mono,
                                   int check_ori, void *d_assign, void *d_nmatches);
/* Frame::isInFrustum for `frames` frames at once: d_Tcw [frames][12]; the points of frame f are d_world / d_normal
 * [frames][pcap][3], d_max_dist / d_min_dist [frames][pcap], d_flags [frames][pcap] uint8, d_np [frames] int32.
 * Outputs d_q [frames][pcap] orbhip_query, d_view_cos [frames][pcap] float (nullable). */
int orbhip_frustum_queries_device(orbhip_matcher *m, int frames, const orbhip_camera *cam, const void *d_Tcw, int pcap,
                                  const void *d_np, const void *d_world, const void *d_normal, const void *d_max_dist,
                                  const void *d_min_dist, const void *d_flags, float viewing_cos_limit, float th,
                                  void *d_q, void *d_view_cos);

/* ---- seeding stereo / RGB-D map points -------------------------------------------------------------------------
 * The step between mvDepth (orbhip_compute_stereo_matches*, orbhip_compute_stereo_from_rgbd*) and the world / flags arrays
 * orbhip_track_last_frame_device reads: which keypoints become new map points, and where they are.
 *   ORBHIP_SEED_CLOSEST  Tracking::UpdateLastFrame (src/Tracking.cc:812-864) and Tracking::CreateNewKeyFrame (:1073-1133):
 *     vDepthIdx = the (z, i) of every keypoint with z = depth[i] > 0, sorted ascending (std::sort on pair<float,int>: by z,
 *     then by i); the walk counts every entry it visits and stops after the first entry with z > th_depth once more than
 *     100 have been visited (that entry is still processed).  A visited entry is created iff its slot has no map point or
 *     a map point nobody observes: !(flags[i] & ORBHIP_POINT_PRESENT) || !(flags[i] & ORBHIP_POINT_OBSERVED) (:839-845).
 *   ORBHIP_SEED_ALL      Tracking::StereoInitialization (:523-538): every keypoint with z > 0, in index order, is created.
 * Flag meaning for these entries: ORBHIP_POINT_PRESENT = mvpMapPoints[i] != NULL (outliers included: the loop does not
 * read mvbOutlier), ORBHIP_POINT_OBSERVED = pMP->Observations() > 0.
 * A created entry gets Frame::UnprojectStereo(i) (src/Frame.cc:666-680): x = ((u - cx) * z) * invfx, y = ((v - cy) * z) *
 * invfy with invfx = 1.0f / fx (src/Frame.cc:108-109), (u, v) = keys[i]; X = mRwc * (x, y, z) + mOw with mRwc = Rcw^T and
 * mOw = -Rcw^T * tcw, all in float in the operation order DESIGN.md section 3 states.  keys = mvKeysUn.
 * KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631, called from src/LocalMapping.cc:342,346) has the same arithmetic but
 * reads mvKeys, NOT mvKeysUn (src/KeyFrame.cc:620): a caller restating the KeyFrame form passes mvKeys.
 * Tcw: top three rows of mTcw, row-major.  world [n][3] / flags [n] are updated in place: created entries get their
 * position and flags[i] = created_flags (ORBHIP_POINT_PRESENT for UpdateLastFrame's temporal points, | ORBHIP_POINT_OBSERVED
 * where the caller adds the observation at once, :1115, :530); every other entry keeps the caller's values.
 * order [n] (nullable): order[j] = i for the j-th visited entry, the order in which the caller creates its MapPoints;
 * created [n] (nullable): 1 where entry i was created, else 0; counts [3] = {n_valid (z > 0), n_visited, n_created}.
 * n == 0 or no positive depth: success, zero counts.  n <= 4096 (ORBHIP_E_CAPACITY beyond: the sort is LDS resident).
 * Host buffers, synchronous. */
#define ORBHIP_SEED_ALL     0   /* StereoInitialization, src/Tracking.cc:523-538 */
#define ORBHIP_SEED_CLOSEST 1   /* UpdateLastFrame :812-864, CreateNewKeyFrame :1073-1133 */
int orbhip_seed_stereo_points(orbhip_matcher *m, const orbhip_camera *cam, const float *Tcw, const orbhip_keypoint *keys,
                              const float *depth, int n, float th_depth, int mode, int created_flags, float *world,
                              uint8_t *flags, int32_t *order, uint8_t *created, int32_t *counts);
/* Device-resident, batched, asynchronous on the matcher's stream: output frame f (0 .. frames-1) reads the keypoints and
 * the count of frame kp_first + f*kp_step of d_kps [..][cap] / d_n [..] (the left frames of an interleaved stereo batch:
 * kp_first = 0, kp_step = 2) and d_Tcw [frames][12], d_depth [frames][cap]; d_world [frames][cap][3] and d_flags
 * [frames][cap] in/out, d_order [frames][cap] int32 and d_created [frames][cap] uint8 nullable, d_counts [frames][3] int32.
 * d_depth is what orbhip_compute_stereo_matches_device writes; orbhip_track_last_frame_device addresses d_world / d_flags by
 * the last frame's index in the extractor arrays, so a caller feeding it allocates them [frames of the batch][cap] and
 * output frame f here is row f of them.  cap <= 4096. */
int orbhip_seed_stereo_points_device(orbhip_matcher *m, int frames, const orbhip_camera *cam, const void *d_Tcw, const void *d_kps,
                                     const void *d_n, int cap, int kp_first, int kp_step, const void *d_depth, float th_depth,
                                     int mode, int created_flags, void *d_world, void *d_flags, void *d_order, void *d_created,
                                     void *d_counts);
/* Tracking::NeedNewKeyFrame's close-point counts (src/Tracking.cc:1001-1018): over the keypoints with depth[i] > 0 &&
 * depth[i] < th_depth (strict), *tracked = nTrackedClose counts those with ORBHIP_POINT_PRESENT, *non_tracked =
 * nNonTrackedClose the others.  Flag meaning for THIS entry: ORBHIP_POINT_PRESENT = mvpMapPoints[i] && !mvbOutlier[i]
 * (:1010), not the bare "map point exists" of the seeding entries.  Host buffers, synchronous; any n. */
int orbhip_count_close_points(orbhip_matcher *m, const float *depth, const uint8_t *flags, int n, float th_depth, int *tracked,
                              int *non_tracked);
/* device-resident, batched: d_depth [frames][cap] float, d_flags [frames][cap] uint8, d_n [frames] int32 (indexed by the
 * output frame, like the other arrays); d_counts [frames][2] int32 = {nTrackedClose, nNonTrackedClose}.  Asynchronous. */
int orbhip_count_close_points_device(orbhip_matcher *m, int frames, const void *d_depth, const void *d_flags, const void *d_n,
                                     int cap, float th_depth, void *d_counts);

/* ---- refreshing map points: descriptor, normal and depth range ---------------------------------------------------
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371) for np map
 * points in one call, from an observation table over the key-frame bank the other _device entries read (d_Tcw [rows][12],
 * d_kps [rows][cap] = mvKeysUn, d_desc [rows][cap][32], d_n [rows]).  It writes the four per-point arrays that
 * orbhip_fuse_device, orbhip_frustum_queries_device, orbhip_keyframe_queries and orbhip_search_by_sim3 read, so that the
 * steps the reference follows with both functions (src/LocalMapping.cc:152-153, :442-444, :526-527; src/Tracking.cc:532-533,
 * :668-669, :1117-1118; src/LoopClosing.cc:500, :532; normal and depth only: src/Optimizer.cc:227, :776, :1042) need no host
 * hop.  The map graph (AddObservation, Replace, the choice of mpRefKF, building the table) stays with the caller.
 *   what: ORBHIP_UPDATE_DESCRIPTOR | ORBHIP_UPDATE_NORMAL_DEPTH, at least one of them (anything else: ORBHIP_E_ARG).
 *   Table, CSR in the caller's order: d_obs_start [np+1] int32, non-decreasing; observation j of point p is key point
 *   d_obs_idx[o] of bank row d_obs_kf[o], o = d_obs_start[p] + j.  A row may repeat inside a list.  d_ref_obs [np] int32: the
 *   position j of mpRefKF's observation in the point's own list (what observations[pRefKF] finds).  The reference iterates a
 *   map<KeyFrame*, size_t>, in heap-address order; here the order is the table's: it decides the float sum of the normal
 *   and which of several equal medians wins (the first).
 *   d_kf_bad [rows] uint8, nullable: pKF->isBad().  Such an observation is left out of the descriptor set (:265) but still
 *   counts for the normal and for n (:350-357 has no such test).
 *   d_flags [pcap] uint8: ORBHIP_POINT_PRESENT = !mbBad; d_world [pcap][3] = mWorldPos.
 *   Outputs, written only where the reference writes (every other entry, and everything at np and above, keeps the caller's
 *   bytes): d_point_desc [pcap][32] = mDescriptor, d_normal [pcap][3] = mNormalVector, d_max_dist / d_min_dist [pcap] = raw
 *   mfMaxDistance / mfMinDistance (the consumers apply 1.2 / 0.8 themselves).  Reports, written for every p < np:
 *   d_status [np] uint8 = one ORBHIP_MAPPOINT_* code; d_best_obs [np] int32 (nullable; written when ORBHIP_UPDATE_DESCRIPTOR
 *   is selected) = position in the point's list of the chosen descriptor, -1 where none was chosen.
 *   Arithmetic: DESIGN.md section 3.  A point on a camera centre divides by zero; the inf / NaN propagates as is.
 *   The device form does not range-check rows, key-point indices or d_obs_start (like d_kf_index elsewhere); d_n is not read.
 *   cap <= 4096 (ORBHIP_E_CAPACITY beyond); np == 0: success, nothing written; np < 0, np > pcap, a bad mask or a null
 *   pointer that a selected bit needs (descriptor: d_desc, d_point_desc; normal / depth: cam, d_Tcw, d_kps, d_ref_obs,
 *   d_world, d_normal, d_max_dist, d_min_dist; always: the table, d_flags, d_status): ORBHIP_E_ARG before any device work.
 *   Asynchronous on the matcher's stream, no host synchronisation and no staging copy; the worklist of the points with more
 *   than 16 observations lives in the handle. */
#define ORBHIP_UPDATE_DESCRIPTOR   1   /* ComputeDistinctiveDescriptors */
#define ORBHIP_UPDATE_NORMAL_DEPTH 2   /* UpdateNormalAndDepth */
#define ORBHIP_MAPPOINT_UPDATED        0   /* refreshed as asked */
#define ORBHIP_MAPPOINT_BAD            1   /* not ORBHIP_POINT_PRESENT (:251, :338): nothing written */
#define ORBHIP_MAPPOINT_NO_OBSERVATION 2   /* empty list (:256, :345): nothing written */
#define ORBHIP_MAPPOINT_NO_DESCRIPTOR  3   /* every observing key frame is bad (:269); normal and depth range are written */
#define ORBHIP_MAPPOINT_BAD_REF        4   /* ref_obs outside [0, N): the descriptor is written, normal and depth range are
                                              not; reported in preference to NO_DESCRIPTOR */
#define ORBHIP_MAPPOINT_TOO_MANY       5   /* N > 2048, the limit of orbhip_distinctive_descriptors: nothing written */
int orbhip_update_map_points_device(orbhip_matcher *m, const orbhip_camera *cam, int what, const void *d_Tcw, const void *d_kps,
                                    const void *d_desc, const void *d_n, int cap, const void *d_kf_bad, int np, int pcap,
                                    const void *d_obs_start, const void *d_obs_kf, const void *d_obs_idx, const void *d_ref_obs,
                                    const void *d_world, const void *d_flags, void *d_point_desc, void *d_normal,
                                    void *d_max_dist, void *d_min_dist, void *d_best_obs, void *d_status);
/* Host buffers, synchronous: one staging copy, the device call above, one read-back.  The bank is K frame views (keys,
 * desc, n; at most 4096 key points each), Tcw [K][12] and kf_bad [K] (nullable); obs_kf indexes the views.  The four
 * arrays are in/out with np entries (entries the reference would not write keep the caller's values); best_obs (nullable)
 * and status are outputs.  Rows outside [0, K), key-point indices outside [0, kfs[row]->n) and a decreasing obs_start are
 * ORBHIP_E_ARG.  Arrays that the selected bits do not need may be null. */
int orbhip_update_map_points(orbhip_matcher *m, const orbhip_camera *cam, int what, int K, const orbhip_frame_view *const *kfs,
                             const float *Tcw, const uint8_t *kf_bad, int np, const int32_t *obs_start, const int32_t *obs_kf,
                             const int32_t *obs_idx, const int32_t *ref_obs, const float *world, const uint8_t *flags,
                             uint8_t *point_desc, float *normal, float *max_dist, float *min_dist, int32_t *best_obs,
                             uint8_t *status);

/* ---- local map: votes, local key frames, local points -----------------------------------------------------------------
 * Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1231-1339), UpdateLocalPoints (:1205-1228) and the two loops in front of
 * SearchLocalPoints' search (:1146-1180) for `frames` current frames in one call, over tables.  The covisibility graph
 * (covis, parent, child) is passed as tables like the observation table: orbhip_update_connections_device and
 * orbhip_children_from_parents_device below maintain them on the device.  Where the reference iterates a map<KeyFrame*, int> or a set<KeyFrame*> in heap-address order, the
 * order here is the table's: ascending bank row for the vote map, the caller's order for the children.
 *
 * orbhip_local_map_tables (read only).  The key-frame bank has `rows` rows of `cap` slots, the map np points in arrays of pcap:
 *   slot_point [rows][cap] int32 = mvpMapPoints of each bank row as point indices, -1 = none; n [rows] int32.
 *   kf_bad [rows] uint8, nullable = pKF->isBad().
 *   covis [rows][10] int32 = the head of mvpOrderedConnectedKeyFrames (GetBestCovisibilityKeyFrames(10)), -1 padded.
 *   child_start [rows+1] / child [..] int32 = mspChildrens in CSR form; parent [rows] int32, -1 = none.
 *   obs_start [np+1] / obs_kf [..] int32: the observation table of orbhip_update_map_points_device.
 *   flags [pcap] uint8: ORBHIP_POINT_PRESENT = !isBad(), ORBHIP_POINT_OBSERVED = Observations() > 0.
 *   world / normal [pcap][3], max_dist / min_dist [pcap] float, point_desc [pcap][32] (16-byte aligned): the arrays
 *   orbhip_update_map_points_device maintains.
 * orbhip_local_map_io.  In/out: frame_point [frames][cap] int32 = mCurrentFrame.mvpMapPoints (a bad point is set to -1,
 *   :1248, :1153), frame_n [frames] int32 (read only); local_kf [frames][rows] int32 / n_local_kf [frames] int32 =
 *   mvpLocalKeyFrames (in/out because :1253 returns early when nobody voted: the previous list then stays and the local
 *   points are rebuilt from it).  Outputs:
 *   votes [frames][rows] int32 = keyframeCounter, zeroed by the call (a row repeated in a list counts each time);
 *   local_point [frames][pcap] int32 = mvpLocalMapPoints as point indices, in the reference's push_back order: list order,
 *     then slot order, each good point at its first occurrence.  SearchByProjection gives a key point to the first point
 *     in this order that wins it, so the order is part of the result;
 *   world_l / normal_l [frames][pcap][3], max_dist_l / min_dist_l [frames][pcap], desc_l [frames][pcap][32] (16-byte
 *     aligned), flags_l [frames][pcap] uint8, np_l [frames] int32: the same points gathered in that order, in the layout
 *     orbhip_frustum_queries_device and orbhip_search_by_projection_points_device read.  flags_l is 0 for a point the frame
 *     already holds (mnLastFrameSeen == mnId, :1170) and ORBHIP_POINT_PRESENT | (flags & ORBHIP_POINT_OBSERVED) otherwise;
 *   taken [frames][cap] uint8 = frame_point[i] >= 0 && Observations() > 0 (src/ORBmatcher.cc:84-86), for i < frame_n;
 *   report [frames][8] int32 = {status, n_voted (bad rows included), n_local_kf, ref_row = mpReferenceKF (-1: unchanged),
 *     ref_votes, walk_end, n_local_points, n_to_match (0 here; orbhip_track_local_map_device fills it)}.
 *     status: ORBHIP_LOCALMAP_OK; ORBHIP_LOCALMAP_NO_VOTES (list kept); ORBHIP_LOCALMAP_ALL_BAD (every voted row is bad: the
 *     list is empty, the reference key frame unchanged).  walk_end (the loop :1282-1332): ORBHIP_LOCALMAP_WALK_EXHAUSTED,
 *     ORBHIP_LOCALMAP_WALK_LIMIT (size() > 80 at the start of a visit), ORBHIP_LOCALMAP_WALK_PARENT (the break at :1328, which
 *     leaves the whole walk).  The reference key frame is the first row, ascending, with the strictly largest vote count
 *     among the rows that are not bad.
 *   A row and a point appear at most once, so [rows] and [pcap] cannot overflow; entries past the counts (and taken past
 *   frame_n) keep the caller's bytes.
 * Asynchronous on the matcher's stream, no host synchronisation, no staging copy: two memsets and six kernel launches.  The
 * workspace (first-occurrence keys, frame-held marks, per-row counts) lives in the handle, grows on demand and is reset by
 * every call.  cap <= 4096, rows <= 65536 (ORBHIP_E_CAPACITY beyond); frames, rows or np negative, cap < 1, np > pcap or a
 * null required pointer (everything but kf_bad): ORBHIP_E_ARG; all refused before any device work.  frames == 0: success,
 * nothing written.  The device form does not range-check the tables' contents (rows, point indices, CSR arrays). */
#define ORBHIP_LOCALMAP_OK       0
#define ORBHIP_LOCALMAP_NO_VOTES 1
#define ORBHIP_LOCALMAP_ALL_BAD  2
#define ORBHIP_LOCALMAP_WALK_EXHAUSTED 0
#define ORBHIP_LOCALMAP_WALK_LIMIT     1
#define ORBHIP_LOCALMAP_WALK_PARENT    2
typedef struct orbhip_local_map_tables {
    const void *slot_point, *n, *kf_bad, *covis, *child_start, *child, *parent;
    const void *obs_start, *obs_kf, *flags;
    const void *world, *normal, *max_dist, *min_dist, *point_desc;
} orbhip_local_map_tables;
typedef struct orbhip_local_map_io {
    void *frame_point;
    const void *frame_n;
    void *local_kf, *n_local_kf;
    void *votes, *local_point, *world_l, *normal_l, *max_dist_l, *min_dist_l, *desc_l, *flags_l, *np_l, *taken, *report;
} orbhip_local_map_io;
int orbhip_update_local_map_device(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap,
                                   const orbhip_local_map_tables *tables, const orbhip_local_map_io *io);
/* The above, then Frame::isInFrustum for the gathered points (orbhip_frustum_queries_device's kernel) and
 * SearchByProjection(F, vpMapPoints, th) (orbhip_search_by_projection_points_device's kernels) on the same stream: the
 * matching step of Tracking::TrackLocalMap up to the pose optimisation.  Rows equal calling the three entries in sequence.
 * track: Tcw [frames][12]; kps [frames][cap] orbhip_keypoint, desc [frames][cap][32], u_right [frames][cap] float (nullable)
 * = the current frames in the extractor's layout (their counts are io->frame_n).  Outputs: q [frames][pcap] orbhip_query,
 * assign [frames][cap] int32 (local entry held by each key point, or -1), nmatches [frames] int32; io->frame_point[i] =
 * local_point[assign[i]] where a key point was assigned (src/ORBmatcher.cc:122) and report[f][7] = nToMatch, the valid query
 * records.  Needs pcap >= 1 besides the limits above. */
typedef struct orbhip_local_map_track {
    const void *Tcw, *kps, *desc, *u_right;
    void *q, *assign, *nmatches;
} orbhip_local_map_track;
int orbhip_track_local_map_device(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap,
                                  const orbhip_local_map_tables *tables, const orbhip_local_map_io *io, const orbhip_camera *cam,
                                  const orbhip_local_map_track *track, float viewing_cos_limit, float th, float nnratio);
/* Host buffers, synchronous: one staging copy, orbhip_update_local_map_device, one read-back.  The same two records with
 * host pointers; the in/out and output arrays come back whole (entries past the counts as they were passed in).  It
 * range-checks what the device form does not: rows in [0, rows), point indices in [-1, np), non-decreasing CSR arrays
 * starting at or above 0, frame_n and n in [0, cap], n_local_kf in [0, rows]: ORBHIP_E_ARG. */
int orbhip_update_local_map(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap,
                            const orbhip_local_map_tables *tables, const orbhip_local_map_io *io);

/* ---- covisibility graph -----------------------------------------------------------------------------------------------
 * KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379) for the U bank rows of d_update_rows, with AddConnection (:123-136)
 * and UpdateBestCovisibles (:138-157) on the rows it connects.  The result equals running it for each entry in list order;
 * a row may come more than once.  The bank has `rows` rows of `cap` slots.
 *
 * orbhip_covis_tables (read only): slot_point [rows][cap] / n [rows], obs_start [np+1] / obs_kf, flags [pcap] as in
 *   orbhip_local_map_tables (ORBHIP_POINT_PRESENT = !isBad()).
 * orbhip_covis_state (in/out, owned by the caller, maintained by the call):
 *   conn_w [rows][rows] int32 = mConnectedKeyFrameWeights of every row, dense; 0 = no entry (the reference never stores a
 *     weight below 1).  GetWeight(c) of row r is conn_w[r][c].
 *   ord_kf / ord_w [rows][rows] int32, n_ord [rows] int32 = mvpOrderedConnectedKeyFrames / mvOrderedWeights; a rewrite of a
 *     list stores its n_ord[r] entries and nothing behind them.  GetCovisiblesByWeight(w) is the prefix of ord_kf[r] whose ord_w[r] is above w.
 *   covis [rows][10] int32 = the head of ord_kf, -1 padded: the array orbhip_local_map_tables.covis reads.  Rewritten for
 *     every row whose ordered list is rewritten.
 *   first_conn [rows] uint8 = mbFirstConnection; parent [rows] int32 = mpParent, written on a first connection.
 * id0_row: the row whose mnId is 0 (it never gets a parent, :371), or -1.
 *
 * Per updated row r.  Counter (:302-320): every slot i < n[r] with a present point adds 1 to counter[obs_kf[o]] for each of
 * its observations with obs_kf[o] != r; a row repeated in a list counts each time; bad key frames are not skipped.  An empty
 * counter (:323) writes nothing, first_conn stays, status ORBHIP_CONNECTIONS_EMPTY.  The qualifying rows are those with
 * counter >= 15, or, if there are none, the first row in ascending order with the strictly largest count (:334-352).
 * AddConnection(r, counter[c]) runs on every qualifying c: if conn_w[c][r] already equals the weight row c is left alone
 * (the early return, :131-132), otherwise conn_w[c][r] is written and ALL entries of conn_w[c][:] are re-sorted into
 * ord_kf[c] / ord_w[c] / n_ord[c] / covis[c].  The own row (:367-369): conn_w[r][:] becomes the WHOLE counter, entries below
 * 15 included and old entries dropped, while ord_kf[r] / ord_w[r] hold ONLY the qualifying rows; the reference has this
 * asymmetry, and it shows when a later AddConnection re-sorts row r from the full map.  Order of a list: the reference sorts
 * pair<int, KeyFrame*> ascending and reverses, so equal weights go by heap address; here address order is row order, as for
 * the vote map of the local map: descending weight, then descending row.  First connection (:371-376): if first_conn[r] and
 * r != id0_row, parent[r] = ord_kf[r][0] and first_conn[r] = 0.
 * d_report [U][8] int32 = {status, distinct voted rows, n_ord[r], row of the maximum (-1: none), the maximum, parent set
 * (-1: not set), other rows re-sorted, 1 if the fallback to the maximum was used}.
 *
 * Asynchronous on the matcher's stream, no host synchronisation: one memset, two launches for the counters of all entries
 * and one launch per entry.  rows, cap <= 4096 (ORBHIP_E_CAPACITY beyond: the state is dense, 3 x 64 MB there); rows, np or U
 * negative, cap < 1, np > pcap, id0_row outside [-1, rows) or a null pointer: ORBHIP_E_ARG; all refused before any device
 * work.  U == 0: success, nothing written.  The device form does not range-check the tables' contents. */
#define ORBHIP_CONNECTIONS_OK    0
#define ORBHIP_CONNECTIONS_EMPTY 1
typedef struct orbhip_covis_tables {
    const void *slot_point, *n, *obs_start, *obs_kf, *flags;
} orbhip_covis_tables;
typedef struct orbhip_covis_state {
    void *conn_w, *ord_kf, *ord_w, *n_ord, *covis, *first_conn, *parent;
} orbhip_covis_state;
int orbhip_update_connections_device(orbhip_matcher *m, int rows, int cap, int np, int pcap, const orbhip_covis_tables *tables,
                                     const orbhip_covis_state *state, int id0_row, int U, const void *d_update_rows,
                                     void *d_report);
/* Host buffers, synchronous: one staging copy, orbhip_update_connections_device, one read-back.  The records hold host
 * pointers to the whole arrays, but only the rows the call can reach travel: the updated rows and the rows their points'
 * observations name; every other row keeps its bytes.  It range-checks what the device form does not: update_rows and
 * obs_kf in [0, rows), n and n_ord in [0, cap] / [0, rows], the point indices of the updated rows in [-1, np), obs_start
 * non-decreasing from 0 or above: ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_update_connections(orbhip_matcher *m, int rows, int cap, int np, int pcap, const orbhip_covis_tables *tables,
                              const orbhip_covis_state *state, int id0_row, int U, const int32_t *update_rows, int32_t *report);
/* Readers of the graph, for Q current rows d_cur [Q], one wavefront each.
 *   nn2 == 0: GetBestCovisibilityKeyFrames(nn) verbatim (:174-182), the neighbour list of CreateNewMapPoints
 *     (src/LocalMapping.cc:210-213); bad rows are NOT skipped there.
 *   nn2 > 0: vpTargetKFs of SearchInNeighbors (src/LocalMapping.cc:457-479; nn = 10 or 20, nn2 = 5 there).  A first
 *     neighbour is skipped if bad or stamped (mnFuseTargetForKF), otherwise appended and stamped; then each of its nn2 best
 *     covisibles is appended unless it is bad, stamped or the current row.  Second neighbours are not stamped, so a row can
 *     come again, which orbhip_fuse_device allows.
 * d_ord_kf [rows][rows] / d_n_ord [rows]: the state above; d_kf_bad [rows] uint8, nullable.  Outputs: d_targets
 * [Q][nn * (1 + nn2)] int32, -1 behind the count, and d_counts [Q] int32: the lists are d_kf_index of
 * orbhip_create_new_map_points_device / orbhip_fuse_device, whose K is a host integer, so the caller reads d_counts.
 * rows <= 4096 (ORBHIP_E_CAPACITY); rows or Q negative, nn < 1, nn2 < 0, nn or nn2 above 4096 or a null pointer:
 * ORBHIP_E_ARG.  Q == 0: success, nothing written. */
int orbhip_covisible_targets_device(orbhip_matcher *m, int rows, const void *d_ord_kf, const void *d_n_ord, const void *d_kf_bad,
                                    int Q, const void *d_cur, int nn, int nn2, void *d_targets, void *d_counts);
/* Host buffers, synchronous; only the heads of the lists it walks travel.  Range-checked: cur and the entries it reads in
 * [0, rows), n_ord in [0, rows]: ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_covisible_targets(orbhip_matcher *m, int rows, const int32_t *ord_kf, const int32_t *n_ord, const uint8_t *kf_bad,
                             int Q, const int32_t *cur, int nn, int nn2, int32_t *targets, int32_t *counts);
/* d_child_start [rows+1] / d_child [rows] (the CSR orbhip_local_map_tables reads) from d_parent [rows] and d_kf_bad [rows]
 * (nullable): row c is a child of parent[c] iff 0 <= parent[c] < rows and c is not bad, because SetBadFlag erases itself from
 * its parent (src/KeyFrame.cc:453-545); ascending row inside a list.  A first connection then needs no host edit of the CSR.
 * rows <= 4096 (ORBHIP_E_CAPACITY). */
int orbhip_children_from_parents_device(orbhip_matcher *m, int rows, const void *d_parent, const void *d_kf_bad,
                                        void *d_child_start, void *d_child);

/* ---- culling: MapPointCulling, KeyFrameCulling, SetBadFlag ------------------------------------------------------------
 * The two steps of LocalMapping::Run that shrink the map, over the tables the entries above read and maintain.
 * mObservations of a point is its list in the observation table of orbhip_update_map_points_device; both calls read the
 * table IN and write the table OUT, the same lists in table order without the erased entries, into buffers the caller
 * provides and then swaps in.  Lists are maps here: mObservations holds a key frame once, so these entries need every list
 * to name a bank row at most once (the other entries tolerate repeats).  The host forms check that; the device forms do not,
 * and a repeated row then leaves its second entry in the list.
 *
 * orbhip_cull_tables (read only): kps [rows][cap] orbhip_keypoint (mvKeysUn; only octave is read), u_right [rows][cap] float
 *   (mvuRight; NULL = monocular: every observation counts 1), depth [rows][cap] float (mvDepth; may be NULL only with
 *   mono != 0), n [rows] int32, obs_start [np+1] / obs_kf / obs_idx / ref_obs [np] int32 as orbhip_update_map_points_device
 *   defines them (ref_obs is a position inside the point's own list), not_erase [rows] uint8 (mbNotErase; NULL = none).
 *   orbhip_cull_map_points* reads u_right and the table only.
 * orbhip_cull_io.  In/out: slot_point [rows][cap] int32, flags [pcap] uint8, kf_bad [rows] uint8, to_be_erased [rows] uint8
 *   (mbToBeErased; needed when not_erase is given), child_start [rows+1] / child [rows] int32 (rewritten at the end as
 *   orbhip_children_from_parents_device does).  Out: obs_start_out [np+1], obs_kf_out / obs_idx_out [obs_cap], ref_obs_out
 *   [np] = the new position of the reference observation, -1 for an empty list or a ref_obs outside its list.  The out
 *   buffers must not be the in buffers (ORBHIP_E_ARG).  orbhip_cull_map_points* uses slot_point, flags and the table out.
 * obs_cap: entries of obs_kf / obs_idx and of their out buffers, at least obs_start[np]; it sizes the workspace, because the
 *   device forms never read obs_start on the host.
 *
 * Observations() is not a caller array: a call derives it at its start as the sum over the list of (u_right[kf][idx] >= 0 ?
 * 2 : 1), which is what AddObservation / EraseObservation maintain for a good point (src/MapPoint.cc:98-137).  A point that
 * is not ORBHIP_POINT_PRESENT when the call starts has no observations (SetBadFlag cleared them): its list is dropped from
 * the table out.  Where a call changes a count it rewrites ORBHIP_POINT_OBSERVED as count > 0; a point that turns bad loses
 * ORBHIP_POINT_PRESENT only (SetBadFlag does not reset nObs).  MapPoint::SetBadFlag (:151-168): every observation (kf, idx)
 * of the point is erased and slot_point[kf][idx] = -1, whatever that slot holds (EraseMapPointMatch is by index).
 *
 * orbhip_cull_map_points_device: d_recent [R] int32 = mlpRecentAddedMapPoints as point indices in list order, d_found /
 *   d_visible / d_first_kf_id [pcap] int32 (mnFound, mnVisible, mnFirstKFid), cur_kf_id, th_obs (2 monocular, 3 otherwise).
 *   Per entry, in the order of the reference's if / else if, d_status [R] uint8:
 *     ORBHIP_CULLPOINT_ALREADY_BAD  isBad(): dropped;
 *     ORBHIP_CULLPOINT_BAD_RATIO    (float)found / visible < 0.25f, evaluated as 4 * found < visible (equal for counts below
 *                                   2^24; x / 0 is false both ways): SetBadFlag, dropped;
 *     ORBHIP_CULLPOINT_BAD_OBS      cur_kf_id - first_kf_id >= 2 and Observations() <= th_obs: SetBadFlag, dropped;
 *     ORBHIP_CULLPOINT_DROPPED_OLD  cur_kf_id - first_kf_id >= 3: dropped, not bad;
 *     ORBHIP_CULLPOINT_KEPT.
 *   d_recent_out [R] = the kept entries in order (entries behind the count keep the caller's bytes), d_n_recent_out [1].
 *   A point listed twice belongs to its first entry: if that one culls it the later ones report ALREADY_BAD, as the
 *   sequential loop does.  No entry's decision reads what another entry's SetBadFlag writes, so the loop is parallel.
 *   Seven launches.  R == 0 (four launches and a memset): the table is still copied through, so the caller can swap
 *   unconditionally.
 *
 * orbhip_cull_key_frames_device: d_cand [U] int32 = the reference's copy vpLocalKeyFrames (:638); -1 entries are skipped, so
 *   the output of orbhip_covisible_targets_device(nn, 0) can be passed as it is.  The call copies the list first: it may be
 *   ord_kf[cur], which the call itself re-sorts.  state: orbhip_covis_state; conn_w, ord_kf, ord_w, n_ord, covis and parent
 *   are maintained, first_conn is not touched.  id0_row as in orbhip_update_connections_device; mono, th_depth = mbMonocular,
 *   mThDepth.  The result equals running the loop for each candidate in list order against the state the candidates before
 *   it left.
 *   Decision (:643-694): r == id0_row is skipped.  Over slots i < n[r] holding a present point: unless mono, a slot with
 *   depth > th_depth || depth < 0 is skipped; nMPs++; if Observations() > 3, the observations in rows other than r whose key
 *   point's octave is <= octave(r, i) + 1 are counted, and the point is redundant at 3.  Cull iff nRedundant > 0.9 * nMPs,
 *   evaluated as 10 * nRedundant > 9 * nMPs.
 *   KeyFrame::SetBadFlag of a culled r (src/KeyFrame.cc:453-545): not_erase[r] sets to_be_erased[r] and nothing else.
 *   Connections: for every c with conn_w[r][c] != 0 and conn_w[c][r] != 0, conn_w[c][r] is cleared and ALL of conn_w[c][:]
 *   is re-sorted into ord_kf[c] / ord_w[c] / n_ord[c] / covis[c] with the order and dense-list rules of
 *   orbhip_update_connections_device; a row r names but that does not name r (the own-row asymmetry) is left alone.
 *   conn_w[r][r] must be 0, as UpdateConnections leaves it.  Points: every slot of r with a point index runs
 *   EraseObservation(r) (src/MapPoint.cc:111-137): r's entry leaves the list, the count drops by 2 or 1, a reference
 *   observation that was r's moves to the first entry left in table order, and at a count <= 2 the point turns bad.  r's own
 *   slots keep their point indices.  Own row: conn_w[r][:] = 0, n_ord[r] = 0, covis[r] = -1 (ord_kf[r] / ord_w[r] keep
 *   their bytes).  Spanning tree (:479-535): the children are the rows c with parent[c] == r that are not bad, in ascending
 *   row; the candidates start as {parent[r]}; each round goes over the children in order and over ord_kf[c] in list order,
 *   and the first strictly largest conn_w[c][entry] to a candidate wins: that child gets that parent and becomes a
 *   candidate.  The children left when no pair is found get parent[r].  parent[r] itself stays.  A culled row without a
 *   parent dereferences null in the reference; here the candidates start empty and the children left get -1.  Then
 *   kf_bad[r] = 1.  A candidate that is already bad goes through all of this again, as in the reference.  mTcp,
 *   Map::EraseKeyFrame and KeyFrameDatabase::erase stay with the caller.
 *   d_report [U][8] int32 = {ORBHIP_CULLKF_* status, nMPs, nRedundant, observations erased (EraseObservation calls that
 *   found an entry), points turned bad, other rows re-sorted, children of r, 1 if a child fell back to parent[r] or r had no
 *   parent}; SKIPPED rows report zeros behind the status.
 *   One launch at the start, then in stream order one for the first verdict and two per candidate (connections and points;
 *   the spanning tree together with the next candidate's verdict, which reads nothing the tree writes), three for the
 *   table and k_cv_children: 2 U + 6 (5 for U == 0).  The launches of a candidate that is not culled leave at once.  The
 *   spanning tree is one wavefront and serial in the children of r.
 *
 * Both: asynchronous on the matcher's stream, no host synchronisation, no staging copy; the alive marks and counts live in
 * the handle, grow on demand and are reset by every call.  rows, cap <= 4096 (ORBHIP_E_CAPACITY beyond).  Negative counts,
 * cap < 1, np > pcap, id0_row outside [-1, rows), th_obs < 0, aliasing in/out tables or a null required pointer:
 * ORBHIP_E_ARG, before any device work.  The device forms do not range-check the tables' contents. */
#define ORBHIP_CULLPOINT_KEPT        0
#define ORBHIP_CULLPOINT_ALREADY_BAD 1
#define ORBHIP_CULLPOINT_BAD_RATIO   2
#define ORBHIP_CULLPOINT_BAD_OBS     3
#define ORBHIP_CULLPOINT_DROPPED_OLD 4
#define ORBHIP_CULLKF_NOT_CULLED    0
#define ORBHIP_CULLKF_CULLED        1
#define ORBHIP_CULLKF_SKIPPED_ID0   2
#define ORBHIP_CULLKF_SKIPPED_ENTRY 3
#define ORBHIP_CULLKF_NOT_ERASE     4
typedef struct orbhip_cull_tables {
    const void *kps, *u_right, *depth, *n, *obs_start, *obs_kf, *obs_idx, *ref_obs, *not_erase;
} orbhip_cull_tables;
typedef struct orbhip_cull_io {
    void *slot_point, *flags, *kf_bad, *to_be_erased, *child_start, *child;
    void *obs_start_out, *obs_kf_out, *obs_idx_out, *ref_obs_out;
} orbhip_cull_io;
int orbhip_cull_map_points_device(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap,
                                  const orbhip_cull_tables *tables, const orbhip_cull_io *io, int R, const void *d_recent,
                                  const void *d_found, const void *d_visible, const void *d_first_kf_id, int cur_kf_id, int th_obs,
                                  void *d_recent_out, void *d_n_recent_out, void *d_status);
int orbhip_cull_key_frames_device(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap,
                                  const orbhip_cull_tables *tables, const orbhip_cull_io *io, const orbhip_covis_state *state,
                                  int id0_row, int U, const void *d_cand, int mono, float th_depth, void *d_report);
/* Host buffers, synchronous: one staging copy, the device call, one read-back.  The records hold host pointers; in/out and
 * output arrays come back whole (entries behind the counts as they were passed in).  They range-check what the device forms
 * do not: obs_kf in [0, rows), obs_idx in [0, cap), a row at most once per list, obs_start non-decreasing from 0 with
 * obs_start[np] <= obs_cap, point indices in [-1, np), n in [0, cap], n_ord in [0, rows] and its entries and parent inside
 * the bank, candidates in [-1, rows) with a row at most once, recent in [0, np): ORBHIP_E_ARG, before the handle is looked
 * at. */
int orbhip_cull_map_points(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *tables,
                           const orbhip_cull_io *io, int R, const int32_t *recent, const int32_t *found, const int32_t *visible,
                           const int32_t *first_kf_id, int cur_kf_id, int th_obs, int32_t *recent_out, int32_t *n_recent_out,
                           uint8_t *status);
int orbhip_cull_key_frames(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *tables,
                           const orbhip_cull_io *io, const orbhip_covis_state *state, int id0_row, int U, const int32_t *cand,
                           int mono, float th_depth, int32_t *report);

/* ---- Sim3 RANSAC ----------------------------------------------------------------------------------------------------------
 * Sim3Solver (src/Sim3Solver.cc) for the current key frame and C loop candidates in one call each: the step of
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:238-342) between orbhip_search_by_bow_device and orbhip_search_by_sim3.
 * orbhip_sim3_setup_device is the constructor (:37-112) with SetRansacParameters (:114-138); orbhip_sim3_iterate_device is
 * iterate (:140-207) for every candidate at once.  The arithmetic, operation by operation, is tests/seqref/sim3.py and
 * DESIGN.md section 3 (a two-sided Jacobi method in fp32 stands in for cv::eigen, the rotation comes straight from the
 * normalised quaternion).  The reference draws with rand(); here the draws are caller data.
 *
 * orbhip_sim3_tables (read only).  The key-frame bank has `rows` rows of `cap` slots, the map np points in arrays of pcap:
 *   slot_point [rows][cap] int32 = mvpMapPoints as point indices, -1 = none; n [rows] int32;
 *   obs_start [np+1] / obs_kf / obs_idx int32: the observation table of orbhip_update_map_points_device.
 *     MapPoint::GetIndexInKeyFrame(row) is obs_idx of the first entry of the point's list whose obs_kf is the row, -1 if none;
 *   flags [pcap] uint8 (ORBHIP_POINT_PRESENT = !isBad()), world [pcap][3] float = mWorldPos;
 *   Tcw [rows][12] float = [Rcw | tcw]; kps [rows][cap] orbhip_keypoint = mvKeysUn (only octave is read).
 * orbhip_sim3_solvers (device state the caller owns, one row per candidate; written by setup, read and advanced by iterate):
 *   x1 / x2 [C][cap][3] float = mvX3Dc1 / mvX3Dc2, p1 / p2 [C][cap][2] float = mvP1im1 / mvP2im2,
 *   max_err1 / max_err2 [C][cap] uint32 = mvnMaxError1 / 2: the reference keeps them in a vector<size_t>, so the threshold is
 *     the TRUNCATED integer of 9.210 * (double)sigma2 (9 at level 0, not 9.21; saturated at 2^32 - 1), compared as a float;
 *   slot1 [C][cap] int32 = mvnIndices1; n_corr [C] int32 = N; n1 [C] int32 = mN1 = n[cur] when setup ran;
 *   limit [C] int32 = mRansacMaxIts after SetRansacParameters, 0 where N < min_inliers;
 *   state [C][2] int32 = {mnIterations, mnBestInliers}.
 *   Entries behind n_corr keep the caller's bytes.
 *
 * orbhip_sim3_setup_device: candidate c is bank row d_kf_index[c], the current key frame row `cur`.  d_matched12 [C][cap]
 * int32 = vpMatched12 per slot of `cur`, negative = none: point indices (ORBHIP_SIM3_MATCH_POINTS) or key-point slots of the
 * candidate row as orbhip_search_by_bow_device writes them (ORBHIP_SIM3_MATCH_SLOTS; mapped through slot_point, a slot
 * without a point is no match).  A slot i1 < n[cur] is kept unless it has no match, slot i1 of `cur` has no point, either
 * point is not ORBHIP_POINT_PRESENT, or either point has no observation in its key frame; the kept ones are compacted in
 * slot order.  level_sigma2 [cam->n_levels] = mvLevelSigma2 (host).  The iteration limit depends on N only: 1 for
 * N == min_inliers, otherwise ceil(log(1 - prob) / log(1 - pow((float)min_inliers / N, 3))) clamped to [1, max_its]; the
 * library computes the cap + 1 values on the host, keeps them in the handle and rebuilds them only when (prob,
 * min_inliers, max_its, cap) change (that one call waits for the stream and uploads the table; no other call
 * synchronises).  state is zeroed.  One launch, one workgroup per candidate.
 * min_inliers >= 3 (a sample is three correspondences), max_its >= 1, 0 < prob < 1.
 *
 * orbhip_sim3_iterate_device advances every candidate by at most n_iterations (the reference passes 5; a device caller
 * passes max_its).  d_draws [C][max_its][3] int32: row `it` serves iteration number `it`, so a later call continues in the
 * same array; draw k lies in [0, N-1-k] and stands for DUtils::Random::RandomInt(0, vAvailableIndices.size()-1) (:168).
 * All hypotheses of the call are computed and scored at once, then the state machine of :183-204 runs as a prefix maximum
 * over the iteration numbers, which gives what the sequential loop gives: the first iteration whose inlier count is
 * >= the best so far and > min_inliers returns.
 *   d_report [C][8] int32 = {status, N, limit, mnIterations after, mnBestInliers after, returned iteration or -1, nInliers,
 *     0}.  status: ORBHIP_SIM3_RETURNED; ORBHIP_SIM3_CONTINUE (bNoMore false, nothing returned); ORBHIP_SIM3_NO_MORE
 *     (mnIterations >= limit when the loop ended without a return; a return on the last allowed iteration reports
 *     RETURNED and the NEXT call reports NO_MORE without running anything); ORBHIP_SIM3_TOO_FEW (N < min_inliers, :146).
 *   d_sim3 [C][16] float = mBestRotation (9, row-major), mBestTranslation (3), mBestScale, three zeros: written only on
 *     a return.
 *   d_inliers [C][cap] uint8 = vbInliers over the slots of `cur`: zeroed for i1 < n1 on every call (:143), then set at
 *     slot1 of the returned hypothesis's inliers.
 * min_inliers, max_its and cap must be the values setup was given; cam supplies fx, fy, cx, cy for both key frames.
 * fix_scale = mbFixScale (stereo / RGB-D).  Three launches; the hypotheses, counts and inlier masks of a call live in the
 * handle.  A zero depth or a degenerate sample propagates inf / NaN as is: every comparison is false, 0 inliers.
 *
 * Both: asynchronous on the matcher's stream, no host synchronisation, no staging copy.  cap <= 4096 (ORBHIP_E_CAPACITY
 * beyond); C, rows or np negative, np > pcap, cap < 1, cur outside [0, rows), a bad match_form, parameters outside the
 * ranges above or a null pointer: ORBHIP_E_ARG; all refused before any device work.  C == 0: success, nothing written.
 * The device forms do not range-check the tables' contents, the candidate rows or the draws (a draw outside its range is
 * clamped into the arrays and gives an unspecified sample). */
#define ORBHIP_SIM3_MATCH_POINTS 0
#define ORBHIP_SIM3_MATCH_SLOTS  1
#define ORBHIP_SIM3_RETURNED 0
#define ORBHIP_SIM3_CONTINUE 1
#define ORBHIP_SIM3_NO_MORE  2
#define ORBHIP_SIM3_TOO_FEW  3
typedef struct orbhip_sim3_tables {
    const void *slot_point, *obs_start, *obs_kf, *obs_idx, *flags, *world, *Tcw, *kps, *n;
} orbhip_sim3_tables;
typedef struct orbhip_sim3_solvers {
    void *x1, *x2, *p1, *p2, *max_err1, *max_err2, *slot1, *n_corr, *n1, *limit, *state;
} orbhip_sim3_solvers;
int orbhip_sim3_setup_device(orbhip_matcher *m, int C, int cur, const void *d_kf_index, const orbhip_camera *cam, int rows, int cap,
                             int np, int pcap, const orbhip_sim3_tables *tables, const void *d_matched12, int match_form,
                             const float *level_sigma2, double prob, int min_inliers, int max_its,
                             const orbhip_sim3_solvers *solvers);
int orbhip_sim3_iterate_device(orbhip_matcher *m, int C, int cap, const orbhip_camera *cam, const orbhip_sim3_solvers *solvers,
                               const void *d_draws, int max_its, int n_iterations, int min_inliers, int fix_scale, void *d_sim3,
                               void *d_inliers, void *d_report);
/* Host buffers, synchronous: one staging copy, setup + iterate(n_iterations), one read-back.  The same table record with
 * host pointers; kf_index [C], matched12 [C][cap], draws [C][max_its][3].  state [C][2] int32, nullable, in/out: NULL (or
 * zeros) is a fresh solver; passing back what an earlier call left resumes that solver, which is how the reference's
 * five-iterations-at-a-time loop runs over this form (the setup is recomputed, it is a function of the tables).  sim3
 * [C][16], inliers [C][cap] and report [C][8] as above (entries the call does not write keep the caller's values).  It
 * range-checks what the device forms do not: kf_index in [0, rows), n in [0, cap], slot_point in [-1, np), matches below np
 * (points) or cap (slots), obs_start non-decreasing from 0, obs_kf in [0, rows), obs_idx in [0, cap), octaves in
 * [0, cam->n_levels), state[c][0] in [0, max_its] and every draw the call can reach in [0, N-1-k] (checked against the N
 * of the tables on the host): ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_sim3_ransac(orbhip_matcher *m, int C, int cur, const int32_t *kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                       int pcap, const orbhip_sim3_tables *tables, const int32_t *matched12, int match_form,
                       const float *level_sigma2, double prob, int min_inliers, int max_its, int fix_scale, const int32_t *draws,
                       int n_iterations, int32_t *state, float *sim3, uint8_t *inliers, int32_t *report);

/* ---- PnP RANSAC -----------------------------------------------------------------------------------------------------------
 * PnPsolver (src/PnPsolver.cc) for the current frame and C relocalisation candidates in one call each: the step of
 * Tracking::Relocalization (src/Tracking.cc:1341-1500) between orbhip_search_by_bow_device and
 * orbhip_search_by_projection_keyframe.  orbhip_pnp_setup_device is the constructor (:67-110) with SetRansacParameters
 * (:121-157); orbhip_pnp_iterate_device is iterate (:165-258) for every candidate at once; PnPsolver::find (:159-163) is
 * iterate(mRansacMaxIts) and has no entry of its own.  The arithmetic, operation by operation, is tests/seqref/pnp.py and
 * DESIGN.md section 3 (Jacobi methods in fp64 stand in for cvSVD, cvInvert(CV_SVD) and cvSolve(CV_SVD)).  The reference
 * draws with DUtils::Random; here the draws are caller data.
 *
 * orbhip_pnp_params = the arguments of SetRansacParameters: prob, min_inliers, max_its, min_set, epsilon, th2 (the
 * reference's relocalisation passes 0.99, 10, 300, 4, 0.5, 5.991).  min_set must be 4 (the sample of :191 is what EPnP
 * here is built for), min_inliers >= 1, max_its in [1, 65536], 0 < prob < 1, epsilon and th2 finite and >= 0.
 * orbhip_pnp_map (read only): flags [pcap] uint8 (ORBHIP_POINT_PRESENT = !isBad()), world [pcap][3] float = mWorldPos,
 *   slot_point [rows][cap] int32 = mvpMapPoints of the candidate key frames as point indices, -1 = none (read only with
 *   ORBHIP_PNP_MATCH_SLOTS; may be NULL otherwise).
 * orbhip_pnp_solvers (device state the caller owns, one row per candidate; written by setup, read and advanced by iterate):
 *   p2d [C][cap][2] float = mvP2D, p3d [C][cap][3] float = mvP3Dw,
 *   max_err [C][cap] float = mvMaxError = mvSigma2[i] * th2 as a float product (a vector<float>, :156),
 *   kp_index [C][cap] int32 = mvKeyPointIndices, n_corr [C] int32 = N,
 *   min_inliers [C] int32 = mRansacMinInliers after the adjustment, limit [C] int32 = mRansacMaxIts after it (0 where
 *     N is below the adjusted minimum: iterate never runs then, :173),
 *   state [C][2] int32 = {mnIterations, mnBestInliers},
 *   best_inliers [C][cap] uint8 = mvbBestInliers over the correspondences, best_Tcw [C][12] float = mBestTcw: written by
 *     iterate when an iteration sets a new best (:212-224), meaningful while state[c][1] > 0; setup leaves them alone.
 *   Entries behind n_corr keep the caller's bytes.
 *
 * orbhip_pnp_setup_device: d_kps [n] orbhip_keypoint = mvKeysUn of the current frame (x, y and octave are read), n <= cap
 * slots.  d_matches [C][cap] int32 = vpMapPointMatches per slot, negative = none: point indices (ORBHIP_PNP_MATCH_POINTS)
 * or key-point slots of bank row d_kf_index[c] as orbhip_search_by_bow_device writes them (ORBHIP_PNP_MATCH_SLOTS; mapped
 * through slot_point, whose rows have the same `cap`; a slot without a point is no match; rows may repeat).  A slot i < n is
 * kept iff it has a match and the point is ORBHIP_POINT_PRESENT (:83-85); the kept ones are compacted in slot order.
 * level_sigma2 [cam->n_levels] = mvLevelSigma2 (host).  The adjustment of :134-152 depends on N and the parameters only:
 *   nMinInliers = (int)((float)N * epsilon), raised to min_inliers, then to min_set; epsilon raised to
 *   (float)nMinInliers / N; the limit is 1 when nMinInliers == N, otherwise
 *   ceil(log(1 - prob) / log(1 - pow(epsilon, 3))) -- exponent 3 although the sample is 4 -- clamped to [1, max_its] (the
 *   quotient is clamped while still a double; the text converts to int first).
 * The library computes the cap + 1 pairs on the host, keeps them in the handle and rebuilds them only when the parameters
 * or cap change (that one call waits for the stream and uploads the table; no other call synchronises).  state is zeroed.
 *
 * orbhip_pnp_iterate_device: d_draws [C][draw_rows][4] int32: row `it` serves iteration number `it`, so a later call
 * continues in the same array; draw k lies in [0, N-1-k] and stands for RandomInt(0, vAvailableIndices.size()-1) (:193).
 * The loop condition of :182 is an OR: a call runs the iterations mnIterations ... max(limit, mnIterations +
 * n_iterations) - 1 unless it returns earlier -- a first call with n_iterations = 5 runs to the limit, a call on a solver
 * at its limit runs n_iterations more.  draw_rows >= max(max_its, n_iterations) is required (ORBHIP_E_ARG otherwise: a
 * fresh solver can reach that many); the limit and the state live on the device, so iterations a resumed solver would
 * run at or behind draw_rows are not run (the host form refuses such a call instead).
 * All hypotheses of the call are computed and scored at once.  Refine() (:260-305) refines mvbBestInliers, not the
 * current hypothesis, and is deterministic, so it runs once per best set: for the set the record holds and for every
 * iteration whose count passes the gate (>= the adjusted minimum, :209) and is strictly above the running best (:212).
 * The iteration that returns is the first one that passes the gate while the refinement of the best set so far has more
 * inliers than the adjusted minimum (:292, strict).
 *   d_report [C][8] int32 = {status, N, limit, mnIterations after, mnBestInliers after, returned iteration or -1,
 *     nInliers, adjusted min inliers}.  status, one per way out of the function:
 *     ORBHIP_PNP_REFINED (:235, bNoMore false; mnIterations stops behind the returned iteration),
 *     ORBHIP_PNP_BEST (:253, bNoMore true: the unrefined mBestTcw / mvbBestInliers, possibly left by an earlier call),
 *     ORBHIP_PNP_NO_MORE (:257 with bNoMore true: the loop only ends with mnIterations >= limit),
 *     ORBHIP_PNP_TOO_FEW (:173; the state is left alone).
 *   d_Tcw [C][12] float = [Rcw | tcw]: written only on REFINED and BEST.
 *   d_inliers [C][cap] uint8 = vbInliers over the key-point slots of the frame (vbInliers[mvKeyPointIndices[i]]): on REFINED
 *     and BEST entries i < n are zeroed, then set; otherwise untouched.
 * n, cap and the parameters must be the values setup was given.  Five launches; the hypotheses, counts, masks and
 * refinements of a call live in the handle.  A NaN or inf from a degenerate sample (coplanar or repeated points, zero
 * depth) propagates: every comparison is false, 0 inliers, nothing faults.
 *
 * Both: asynchronous on the matcher's stream, no host synchronisation, no staging copy.  cap <= 4096 (ORBHIP_E_CAPACITY
 * beyond); C, n, rows or np negative, n > cap, np > pcap, cap < 1, a bad match_form, min_set != 4, parameters outside the
 * ranges above or a null pointer: ORBHIP_E_ARG; all refused before any device work.  C == 0: success, nothing written.
 * The device forms do not range-check the matches, the candidate rows, the state or the draws (a draw outside its range
 * is clamped into the list). */
#define ORBHIP_PNP_MATCH_POINTS 0
#define ORBHIP_PNP_MATCH_SLOTS  1
#define ORBHIP_PNP_REFINED 0
#define ORBHIP_PNP_BEST    1
#define ORBHIP_PNP_NO_MORE 2
#define ORBHIP_PNP_TOO_FEW 3
typedef struct orbhip_pnp_params {
    double prob;
    int32_t min_inliers, max_its, min_set;
    float epsilon, th2;
} orbhip_pnp_params;
typedef struct orbhip_pnp_map {
    const void *flags, *world, *slot_point;
} orbhip_pnp_map;
typedef struct orbhip_pnp_solvers {
    void *p2d, *p3d, *max_err, *kp_index, *n_corr, *min_inliers, *limit, *state, *best_inliers, *best_Tcw;
} orbhip_pnp_solvers;
int orbhip_pnp_setup_device(orbhip_matcher *m, int C, const void *d_kps, int n, int cap, const void *d_matches, int match_form,
                            const void *d_kf_index, int rows, int np, int pcap, const orbhip_pnp_map *map,
                            const orbhip_camera *cam, const float *level_sigma2, const orbhip_pnp_params *params,
                            const orbhip_pnp_solvers *solvers);
int orbhip_pnp_iterate_device(orbhip_matcher *m, int C, int n, int cap, const orbhip_camera *cam, const orbhip_pnp_params *params,
                              const orbhip_pnp_solvers *solvers, const void *d_draws, int draw_rows, int n_iterations,
                              void *d_Tcw, void *d_inliers, void *d_report);
/* Host buffers, synchronous: one staging copy, setup + iterate(n_iterations), one read-back.  kps [n], matches [C][cap],
 * kf_index [C] (NULL allowed with ORBHIP_PNP_MATCH_POINTS), the map record with host pointers, draws [C][draw_rows][4].
 * state [C][2], best_inliers [C][cap] and best_Tcw [C][12] are in/out and nullable together: NULL (or a zero state) is a
 * fresh solver; passing back what an earlier call left resumes it, which is how the reference's five-iterations-at-a-time
 * loop runs over this form (the setup is recomputed, it is a function of the inputs).  Tcw [C][12], inliers [C][cap] and
 * report [C][8] as above (what the call does not write keeps the caller's values).  It range-checks what the device forms
 * do not: matches below np (points) or cap (slots), kf_index in [0, rows), slot_point in [-1, np), octaves in
 * [0, cam->n_levels), state[c][0] >= 0, state[c][1] either 0 or in [adjusted minimum, N] and equal to the number of set
 * entries of best_inliers[c], draw_rows large enough for every iteration the call runs, and every such draw in
 * [0, N-1-k]: ORBHIP_E_ARG, before the handle is looked at, nothing written. */
int orbhip_pnp_ransac(orbhip_matcher *m, int C, const orbhip_keypoint *kps, int n, int cap, const int32_t *matches, int match_form,
                      const int32_t *kf_index, int rows, int np, int pcap, const orbhip_pnp_map *map, const orbhip_camera *cam,
                      const float *level_sigma2, const orbhip_pnp_params *params, const int32_t *draws, int draw_rows,
                      int n_iterations, int32_t *state, uint8_t *best_inliers, float *best_Tcw, float *Tcw, uint8_t *inliers,
                      int32_t *report);

/* ---- pose optimisation --------------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization (src/Optimizer.cc:239-451) for `frames` frames in one call, one workgroup each: the step of
 * Tracking between orbhip_track_last_frame_device and orbhip_track_local_map_device (src/Tracking.cc:898, :775), the one
 * after SearchLocalPoints (:940) and the one relocalisation runs on every pose orbhip_pnp_iterate_device returns
 * (:1440-1471).  One 6-DoF vertex, unary monocular and stereo edges, four rounds of g2o's Levenberg-Marquardt with the
 * outlier classification between them.  The arithmetic, operation by operation, is tests/seqref/poseopt.py and DESIGN.md
 * section 3 (the order of the sums over edges, det_sincos64, the pivoted LDLt and Eigen's quaternion formulas are stated
 * there).
 *
 * Read only: d_kps [frames][cap] orbhip_keypoint = mvKeysUn (x, y and octave are read), d_n [frames] int32 = N,
 * d_u_right [frames][cap] float = mvuRight (NULL: every edge is monocular; otherwise u_right[i] < 0 is monocular, :286),
 * d_world [wrows][pcap][3] float = mWorldPos, d_point_flags [wrows][pcap] uint8 (ORBHIP_POINT_OBSERVED is read by the two
 * epilogue modes; NULL allowed with ORBHIP_POSEOPT_PLAIN), d_world_row [frames] int32 = the row of d_world / d_point_flags a
 * frame's point indices refer to (NULL: row 0 for every frame, the shared map arrays of orbhip_local_map_tables; with
 * pcap == cap and world_row[p] = the last frame of pair p it is the per-frame layout of orbhip_track_last_frame_device),
 * inv_level_sigma2 [cam->n_levels] = mvInvLevelSigma2 (host), cam: fx, fy, cx, cy, mbf.
 * In/out: d_Tcw [frames][12] float = [Rcw | tcw]; d_frame_point [frames][cap] int32 = mvpMapPoints as indices into the
 * frame's world row, -1 = none (written only by the two epilogue modes).
 * Out: d_outlier [frames][cap] uint8 = mvbOutlier: only slots i < n with a point are written (:289 and :323 clear them
 * even when the function returns at :365); d_discarded [frames][cap] int32, nullable: for i < n the point an epilogue took
 * out of slot i, else -1 (not written with ORBHIP_POSEOPT_PLAIN); d_report [frames][8] int32 = {status,
 * nInitialCorrespondences, nBad, return value, rounds run, optimize() iterations run in total, count A, count B}.
 * status: ORBHIP_POSEOPT_OK; ORBHIP_POSEOPT_TOO_FEW (:364, fewer than three edges: return value 0, the pose is untouched);
 * ORBHIP_POSEOPT_ONE_ROUND (the break of :440: optimizer.edges() counts all edges, so it happens after round 0 and exactly
 * when 3 <= nInitialCorrespondences < 10).
 * mode: ORBHIP_POSEOPT_PLAIN: the function alone (counts A and B are 0).
 *   ORBHIP_POSEOPT_DISCARD: plus the loop of src/Tracking.cc:900-919 (the same text as :778-795): an outlier slot has its
 *     point moved to d_discarded, frame_point = -1 and the outlier byte cleared; count A = the slots that keep a point
 *     (nmatches left), count B = nmatchesMap, the inlier slots whose point is ORBHIP_POINT_OBSERVED.
 *   ORBHIP_POSEOPT_LOCAL_MAP: plus :941-963: count A = mnMatchesInliers (inlier slots whose point is OBSERVED, or all
 *     inlier slots with the flag ORBHIP_POSEOPT_ONLY_TRACKING), count B = the inlier slots (the IncreaseFound count); with
 *     the flag ORBHIP_POSEOPT_STEREO outlier slots lose their point (:959-960) and their outlier byte stays set, as in
 *     the reference.
 * Every round restarts from the input pose (:377), only the outlier set carries over, and the pose returned is the last
 * round's.  A NaN or inf from a point at zero depth propagates; nothing faults.
 *
 * Asynchronous on the matcher's stream, no host synchronisation, no staging copy, one launch.  cap <= 4096
 * (ORBHIP_E_CAPACITY beyond); frames, wrows or pcap negative, cap < 1, wrows or pcap < 1 with frames > 0, cam->n_levels
 * outside [1, ORBHIP_MAX_LEVELS], a bad mode, flag bits other than the two above or a null required pointer:
 * ORBHIP_E_ARG; all refused before any device work.  frames == 0: success, nothing written.  The device form does not
 * range-check its arrays: n is clamped to [0, cap], an octave into the level table, and a point index outside [0, pcap)
 * or a frame whose world_row is outside [0, wrows) counts as "no point". */
#define ORBHIP_POSEOPT_PLAIN     0
#define ORBHIP_POSEOPT_DISCARD   1
#define ORBHIP_POSEOPT_LOCAL_MAP 2
#define ORBHIP_POSEOPT_ONLY_TRACKING 1
#define ORBHIP_POSEOPT_STEREO        2
#define ORBHIP_POSEOPT_OK        0
#define ORBHIP_POSEOPT_TOO_FEW   1
#define ORBHIP_POSEOPT_ONE_ROUND 2
int orbhip_pose_optimization_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap, const void *d_u_right,
                                    const void *d_world, const void *d_point_flags, int wrows, int pcap, const void *d_world_row,
                                    const orbhip_camera *cam, const float *inv_level_sigma2, int mode, int flags, void *d_Tcw,
                                    void *d_frame_point, void *d_outlier, void *d_discarded, void *d_report);
/* Host buffers, synchronous: one staging copy, the launch, one read-back; what the call does not write keeps the caller's
 * values.  It range-checks what the device form does not: n in [0, cap], world_row in [0, wrows), and for the slots i < n
 * point indices in [-1, pcap) and, where a slot has a point, octaves in [0, cam->n_levels): ORBHIP_E_ARG, before the handle
 * is looked at, nothing written. */
int orbhip_pose_optimization(orbhip_matcher *m, int frames, const orbhip_keypoint *kps, const int32_t *n, int cap, const float *u_right,
                             const float *world, const uint8_t *point_flags, int wrows, int pcap, const int32_t *world_row,
                             const orbhip_camera *cam, const float *inv_level_sigma2, int mode, int flags, float *Tcw,
                             int32_t *frame_point, uint8_t *outlier, int32_t *discarded, int32_t *report);

/* ---- Sim3 optimisation ----------------------------------------------------------------------------------------------------
 * Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) for the current key frame and C loop candidates in one call, one
 * workgroup each: the step of LoopClosing::ComputeSim3 (src/LoopClosing.cc:326) after orbhip_search_by_sim3.  One Sim3
 * vertex, fixed points, the pairs of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ with g2o's numeric Jacobian
 * (delta = 1e-9), Huber in both rounds: optimize(5), the check, optimize(nBad > 0 ? 10 : 5), the check.  The arithmetic,
 * operation by operation, is tests/seqref/sim3opt.py and DESIGN.md section 3 (the order of the sums over pairs, det_exp64,
 * det_sincos64, the pivoted LDLt at 7 and Eigen's quaternion formulas are stated there).
 *
 * C, cur, d_kf_index [C], rows, cap, np, pcap, tables and match_form are those of orbhip_sim3_setup_device; of the tables'
 * kps x, y and octave are read.  inv_level_sigma2 [cam->n_levels] = mvInvLevelSigma2 (host); cam supplies fx, fy, cx, cy for
 * both key frames.  th2 is 10 in the reference (> 0); deltaHuber is sqrtf(th2).  fix_scale = bFixScale: the scale leaves
 * the call with the bits it came with.
 * d_select [C] uint8, nullable: a candidate with 0 is skipped, nothing of its rows is written except report[0] =
 * ORBHIP_SIM3OPT_SKIPPED; a caller passes the batch of orbhip_sim3_iterate_device as it stands and selects the candidates
 * that reported ORBHIP_SIM3_RETURNED.
 * In/out: d_matched12 [C][cap] int32 = vpMatches1 per slot of `cur`, as point indices or as slots of the candidate row
 * (resolved as setup resolves them).  A slot i < n[cur] makes a pair unless it has no match, slot i of `cur` has no point,
 * either point is not ORBHIP_POINT_PRESENT or the candidate's point has no observation in the candidate row (i2 =
 * GetIndexInKeyFrame; the index of the first point in `cur` is not asked for: obs1 is key point i).  An entry becomes -1
 * where the reference nulls vpMatches1[idx] (after either round); every other entry keeps its bytes.
 * In: d_sim3 [C][16] float as orbhip_sim3_iterate_device writes it: R (9), t (3), s; it enters as
 * g2o::Sim3(toMatrix3d(R), toVector3d(t), s).
 * Out: d_S12 [C][8] double = g2oS12 after the call: quaternion x, y, z, w (not normalised, as g2o keeps it), t, s; on the
 * early return (nCorrespondences - nBad < 10) the input Sim3 converted as above.  d_Scw [C][12] float, nullable =
 * Converter::toCvMat(gScm * gSmw) with gSmw = Sim3(R2w, t2w, 1) (src/LoopClosing.cc:333-335): rows of s R | t; written for
 * every candidate that did not return early, the caller uses the rows whose nIn >= 20.  d_report [C][8] int32 = {status,
 * nCorrespondences, nBad (of the first check), nIn (the return value; 0 on the early return), LM iterations of round 1, of
 * round 2, 0, 0}; status: ORBHIP_SIM3OPT_OK, ORBHIP_SIM3OPT_TOO_FEW (the early return; with no pair at all nothing is
 * optimised) or ORBHIP_SIM3OPT_SKIPPED.
 * chi2 is compared as a double against (double)th2, strictly, at the last TRIED estimate of the round; a NaN from a point at
 * zero depth is not greater and its pair stays.
 *
 * Asynchronous on the matcher's stream, no host synchronisation, no staging copy, one launch.  cap <= 4096
 * (ORBHIP_E_CAPACITY beyond); C, rows, np or pcap negative, np > pcap, cap < 1, cur outside [0, rows), a bad match_form,
 * cam->n_levels outside [1, ORBHIP_MAX_LEVELS], th2 not > 0 or a null required pointer: ORBHIP_E_ARG; all refused before any
 * device work.  C == 0: success, nothing written.  The device form does not range-check the tables' contents or the
 * candidate rows. */
#define ORBHIP_SIM3OPT_OK      0
#define ORBHIP_SIM3OPT_TOO_FEW 1
#define ORBHIP_SIM3OPT_SKIPPED 2
int orbhip_optimize_sim3_device(orbhip_matcher *m, int C, int cur, const void *d_kf_index, const orbhip_camera *cam, int rows, int cap,
                                int np, int pcap, const orbhip_sim3_tables *tables, int match_form, const float *inv_level_sigma2,
                                float th2, int fix_scale, const void *d_select, void *d_matched12, const void *d_sim3, void *d_S12,
                                void *d_Scw, void *d_report);
/* Host buffers, synchronous: one staging copy, the launch, one read-back; what the call does not write keeps the caller's
 * values.  The same table record with host pointers; kf_index [C], select [C] or NULL, matched12 [C][cap], sim3 [C][16],
 * S12 [C][8], Scw [C][12] or NULL, report [C][8].  It range-checks what orbhip_sim3_ransac range-checks of the tables, the
 * candidate rows and the matches, and the octaves of the slots of `cur` that hold a point: ORBHIP_E_ARG, before the handle
 * is looked at. */
int orbhip_optimize_sim3(orbhip_matcher *m, int C, int cur, const int32_t *kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                         int pcap, const orbhip_sim3_tables *tables, int match_form, const float *inv_level_sigma2, float th2,
                         int fix_scale, const uint8_t *select, int32_t *matched12, const float *sim3, double *S12, float *Scw,
                         int32_t *report);

/* ---- local bundle adjustment --------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) for one current key frame, device resident: the link of a
 * local-mapping step between orbhip_update_connections_device and orbhip_cull_key_frames_device.  The three lists
 * (:456-504), one SE3 vertex per listed key frame, one point vertex per local point, one EdgeSE3ProjectXYZ /
 * EdgeStereoSE3ProjectXYZ per observation whose key frame is not bad (:589), g2o's Levenberg-Marquardt over
 * BlockSolver_6_3 (the Schur complement over points, a dense system over the free poses), optimize(5) with Huber, the
 * level-1 rule (:672-702), optimize(10) without kernel, the final check (:715-743) and the write-back (:762-776).  The
 * arithmetic, operation by operation, is tests/seqref/lba.py and DESIGN.md section 3: everything is fp64 with one rounding
 * per operation, the orders of all sums, the 3x3 inverse, the order of the poses in the Schur system (list order) and its
 * unpivoted LDLt are stated there.
 *
 * cur: the row of the current key frame; id0_row: the row whose mnId is 0 (setFixed although local), or -1.
 * orbhip_lba_tables: slot_point [rows][cap] int32, n [rows] int32, kf_bad [rows] uint8 (nullable: none is bad) as in the
 * culling entries; obs_start [np+1], obs_kf, obs_idx int32: the observation table; flags [pcap] uint8, ORBHIP_POINT_PRESENT
 * = !isBad(); kps [rows][cap] (x, y and octave are read); u_right [rows][cap] float, nullable (every observation is
 * monocular), monocular iff u_right < 0 (:594); ord_kf [rows][rows], n_ord [rows] int32 of orbhip_covis_state
 * (GetVectorCovisibleKeyFrames); in/out: Tcw [rows][12] float, world [pcap][3] float.  Where the reference iterates a
 * std::map<KeyFrame*, size_t> the order is the table's order.
 * orbhip_lba_out: local_kf [rows], fixed_kf [rows] int32 = lLocalKeyFrames, lFixedCameras in push_back order; local_point
 * [max_points] int32 = lLocalMapPoints likewise, the point list orbhip_update_map_points_device takes (chain it with
 * ORBHIP_UPDATE_NORMAL_DEPTH for :776); erase [max_edges][3] int32 = (key-frame row, key-point index, point) of vToErase in
 * the reference's order, all monocular edges in creation order, then all stereo edges: applying them (:748-757) stays with
 * the caller; report [16] int32 = {status, local key frames, fixed key frames, local points, monocular edges, stereo
 * edges, edges at level 1 after round 1, erase rows, outer iterations and trials of round 1, of round 2, poses in the
 * system of round 1, of round 2, 0, samples of the stop byte}.
 * status: ORBHIP_LBA_OK; ORBHIP_LBA_STOPPED (the stop byte was set at :655-657: only the report is written);
 * ORBHIP_LBA_ONE_ROUND (bDoMore false: the final check and the write-back still happen); ORBHIP_LBA_CAPACITY (more than
 * ORBHIP_LBA_MAX_LOCAL non-fixed local key frames, more than max_points points or max_edges edges: only the report is
 * written, the caller falls back).  Every local key frame and every local point is written back, as toCvMat(SE3Quat) and
 * as float, the fixed id0_row included; fixed cameras are not.
 * d_stop: nullable device byte = *pbStopFlag, sampled where the reference samples it (:655, :664, terminate() at the top of
 * every outer iteration and at the end of a rejected trial).  Only "set before the call" and "null" are deterministic.
 *
 * Asynchronous on the matcher's stream, no host synchronisation: a fixed sequence of small launches (5 and 10 outer
 * iterations of at most 10 trials) is enqueued, every kernel reads the state record first and leaves when its step is not
 * due; no workgroup waits for another.  The workspace belongs to the handle and is sized from rows, pcap, max_points and
 * max_edges; growing it is the only thing that synchronises.  rows, cap <= 4096 (ORBHIP_E_CAPACITY beyond); negative counts,
 * cap < 1, np > pcap, cur outside [0, rows), id0_row outside [-1, rows), max_points or max_edges < 1, cam->n_levels outside
 * [1, ORBHIP_MAX_LEVELS] or a null required pointer: ORBHIP_E_ARG; all refused before any device work.  The device form
 * does not range-check the tables' contents. */
#define ORBHIP_LBA_MAX_LOCAL 128
#define ORBHIP_LBA_OK        0
#define ORBHIP_LBA_STOPPED   1
#define ORBHIP_LBA_ONE_ROUND 2
#define ORBHIP_LBA_CAPACITY  3
typedef struct orbhip_lba_tables {
    const void *slot_point, *n, *kf_bad, *obs_start, *obs_kf, *obs_idx, *flags, *kps, *u_right, *ord_kf, *n_ord;
    void *Tcw, *world;
} orbhip_lba_tables;
typedef struct orbhip_lba_out {
    void *local_kf, *fixed_kf, *local_point, *erase, *report;
} orbhip_lba_out;
int orbhip_local_bundle_adjustment_device(orbhip_matcher *m, int cur, int id0_row, const orbhip_camera *cam, int rows, int cap, int np,
                                          int pcap, const orbhip_lba_tables *tables, const float *inv_level_sigma2, int max_points,
                                          int max_edges, const void *d_stop, const orbhip_lba_out *out);
/* Host buffers, synchronous: one staging copy, the call, one read-back; what the call does not write keeps the caller's
 * values.  The same records with host pointers; stop points to a host byte or is NULL.  It range-checks what the device
 * form does not: n in [0, cap], slot points in [-1, np), obs_start non-decreasing from 0 or above, obs_kf in [0, rows),
 * obs_idx in [0, cap), n_ord in [0, rows], the head of ord_kf[cur] in [0, rows), and the octaves of observed key points in
 * [0, cam->n_levels): ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_local_bundle_adjustment(orbhip_matcher *m, int cur, int id0_row, const orbhip_camera *cam, int rows, int cap, int np,
                                   int pcap, const orbhip_lba_tables *tables, const float *inv_level_sigma2, int max_points,
                                   int max_edges, const uint8_t *stop, const orbhip_lba_out *out);

/* ---- essential-graph optimisation ----------------------------------------------------------------------------------------
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044, called at src/LoopClosing.cc:567), device resident: the
 * step of CorrectLoop that moves the map.  One VertexSim3Expmap per bank row that is not bad, in row order (the row
 * loop_row is fixed); EdgeSim3 with the identity as information in the reference's creation order: the loop connections
 * (weight gate conn_w[i][j] < 100, the pair (cur, loop_row) exempt; they form sInsertedEdges), then per row the
 * spanning-tree edge, the old loop edges to a smaller mnId, and the covisibility edges of weight >= 100 to a smaller mnId
 * that are not the parent, a child, a loop-edge partner, bad or already inserted; g2o's numeric Jacobians through
 * oplusImpl, Levenberg-Marquardt from setUserLambdaInit(1e-16) for 20 outer iterations of at most 10 trials, no robust
 * kernel; the SE3 write-back (:991-1010) and the correction of every present point (:1012-1041).  The arithmetic,
 * operation by operation, is tests/seqref/essgraph.py and DESIGN.md section 3: everything is fp64 with one rounding per
 * operation; det_log64 / det_acos64 stand for std::log / acos, a stated 3x3 LU for W.lu().solve(t), and a dense unpivoted
 * LDLt over 7 unknowns per free vertex in row order for LinearSolverEigen's sparse Cholesky.  Where the reference iterates a
 * std::set or std::map of key frames the order is ascending bank row: loop_kf and lc_kf list each row's entries ascending.
 *
 * orbhip_eg_tables: kf_bad [rows] uint8 (nullable: none is bad; a bad row is not in the map and is skipped everywhere),
 * kf_id [rows] int32 = mnId, parent [rows] int32 (-1: none), conn_w / ord_kf / ord_w [rows][rows], n_ord [rows] int32 of
 * orbhip_covis_state (GetCovisiblesByWeight(100) is the prefix of ord_kf whose ord_w is at least 100 -- and, as
 * src/KeyFrame.cc:191-193 has it, nothing when no entry of the row is below 100; hasChild(n) is parent[n] == r && !kf_bad[n]),
 * loop_start [rows+1] / loop_kf int32 = mspLoopEdges, lc_start [rows+1] / lc_kf int32 = LoopConnections, corrected /
 * non_corrected [rows][8] double = CorrectedSim3 / NonCorrectedSim3 in the S12 layout of orbhip_optimize_sim3 (quaternion x,
 * y, z, w, t, s) with in_corrected / in_non_corrected [rows] uint8 saying which rows they hold, flags [pcap] uint8
 * (ORBHIP_POINT_PRESENT = !isBad()), ref_kf [pcap] int32 = the row of GetReferenceKeyFrame(), corrected_by_kf /
 * corrected_ref [pcap] int32 = mnCorrectedByKF / mnCorrectedReference as rows (-1: none); in/out: Tcw [rows][12] float,
 * world [pcap][3] float.
 * orbhip_eg_out: point_list [pcap] int32 = the present points in index order, the list orbhip_update_map_points_device
 * takes (chain it with ORBHIP_UPDATE_NORMAL_DEPTH for :1042); Scw / Swc [rows][8] double = vScw / vCorrectedSwc of the rows
 * that are not bad; report [16] int32 = {status, vertices, loop-connection edges, spanning-tree edges, old-loop edges,
 * covisibility edges, edges skipped by the sInsertedEdges rule, by the weight gate, outer iterations, trials, unknowns,
 * points listed, edges skipped because an end is a bad row (a null vertex in the reference), 0, 0, 0}.
 * Every row that is not bad has its Tcw written as [R | t/s] in float, loop_row included; every present point whose
 * reference row is in the map has its position written; a point whose reference row is bad or -1 keeps its position (the
 * reference reads default-constructed Sim3s there) and is still listed.
 * status: ORBHIP_EG_OK; ORBHIP_EG_CAPACITY (more than ORBHIP_EG_MAX_KF rows that are not bad, or more than max_edges edges:
 * only the report is written, the caller falls back); ORBHIP_EG_SINGULAR (a pivot was <= 0 on every trial of the first
 * iteration: the estimates are unchanged and the write-back still happens with them, as g2o does).
 *
 * This entry synchronises: the number of trials depends on the data, so the call reads the state record back once after
 * the setup and once per trial (one small pinned copy, one stream synchronisation) and enqueues the next step from it; when
 * it returns, the work is done.  The launches per trial depend on rows only.  The factorisation is blocked over panels of
 * whole poses and runs from global memory; the workspace (about 100 MB at 512 key frames, plus 3 KB per edge) belongs to
 * the handle.  rows <= 4096 (ORBHIP_E_CAPACITY beyond); rows < 1, pcap < 0, cur or loop_row outside [0, rows), max_edges <
 * 1 or a null required pointer: ORBHIP_E_ARG; all refused before any device work.  The device form does not range-check
 * the tables' contents; an edge whose other end is a bad row is skipped and counted. */
#ifndef ORBHIP_EG_MAX_KF
#define ORBHIP_EG_MAX_KF 512
#endif
#define ORBHIP_EG_OK       0
#define ORBHIP_EG_CAPACITY 1
#define ORBHIP_EG_SINGULAR 2
typedef struct orbhip_eg_tables {
    const void *kf_bad, *kf_id, *parent, *conn_w, *ord_kf, *ord_w, *n_ord, *loop_start, *loop_kf, *lc_start, *lc_kf, *corrected,
        *non_corrected, *in_corrected, *in_non_corrected, *flags, *ref_kf, *corrected_by_kf, *corrected_ref;
    void *Tcw, *world;
} orbhip_eg_tables;
typedef struct orbhip_eg_out {
    void *point_list, *Scw, *Swc, *report;
} orbhip_eg_out;
int orbhip_optimize_essential_graph_device(orbhip_matcher *m, int cur, int loop_row, int rows, int pcap,
                                           const orbhip_eg_tables *tables, int fix_scale, int max_edges, const orbhip_eg_out *out);
/* Host buffers, synchronous: one staging copy, the call, one read-back; what the call does not write keeps the caller's
 * values.  The same records with host pointers.  It range-checks what the device form does not: parent in [-1, rows), n_ord
 * in [0, rows], the entries of ord_kf behind n_ord in [0, rows), loop_start / lc_start non-decreasing from 0, loop_kf /
 * lc_kf in [0, rows) and ascending within a row, ref_kf / corrected_ref in [-1, rows); and it refuses the tables the
 * reference would dereference a null vertex on: a row that is not bad whose parent, loop_kf entry or lc_kf entry is a bad
 * row, and a bad row with lc_kf entries: ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_optimize_essential_graph(orbhip_matcher *m, int cur, int loop_row, int rows, int pcap, const orbhip_eg_tables *tables,
                                    int fix_scale, int max_edges, const orbhip_eg_out *out);
/* counters [2] = {stream synchronisations, kernel launches} of this handle's last essential-graph call. */
int orbhip_optimize_essential_graph_counters(orbhip_matcher *m, int32_t counters[2]);

/* ---- global bundle adjustment ---------------------------------------------------------------------------------------------
 * Optimizer::BundleAdjustment (src/Optimizer.cc:49-237; GlobalBundleAdjustemnt :41-46 is the call with null lists), device
 * resident: the end of a loop closure (LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:645-749) and of monocular
 * initialisation (Tracking::CreateInitialMapMonocular).  One SE3 vertex per listed key frame that is not bad (:71-83; the rows
 * whose kf_id is 0 are fixed, maxKFid is the largest kf_id among the vertices), one point vertex per listed point that is
 * PRESENT, one EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ per observation in table order whose row is not bad and has kf_id
 * <= maxKFid (:109), monocular iff u_right < 0, information mvInvLevelSigma2[octave]; a point without an edge is removed
 * (:175-179) and neither written nor marked; one optimize(iterations) of g2o's Levenberg-Marquardt over BlockSolver_6_3, at most
 * 10 trials per iteration, with Huber kernels of (float)sqrt(5.99) and (float)sqrt(7.815) when robust, none otherwise; no
 * level-1 rule, no chi2 check, no erase list; the write-back (:193-235).  The arithmetic, operation by operation, is
 * tests/seqref/gba.py and DESIGN.md section 3: the edges, the blocks, the Schur complement, the state machine and every sum
 * order are those of the local bundle adjustment; the free poses of the reduced system are the vertices in list order with
 * the fixed rows left out; its unpivoted LDLt is blocked (the kernels the essential-graph optimisation uses) and equals the
 * sequential one bit for bit.
 *
 * orbhip_gba_tables: kf_bad [rows] uint8 (nullable: none is bad), kf_id [rows] int32 = mnId, obs_start [np+1], obs_kf, obs_idx
 * int32, flags [pcap] uint8, kps [rows][cap], u_right [rows][cap] float (nullable: every observation is monocular) as in
 * orbhip_lba_tables; in/out: Tcw [rows][12] float, world [pcap][3] float.
 * d_kf_list [nkf] / d_pt_list [npt] int32 = vpKFs / vpMP, each nullable: every row / every point index below np in ascending
 * order (nkf / npt are ignored then).  A list entry outside the tables is skipped.  iterations >= 1.
 * mode ORBHIP_GBA_IN_PLACE (nLoopKF == 0): Tcw and world are written, and out->point_list [max_points] int32 receives the
 * written points in list order: the list orbhip_update_map_points_device takes (chain it with ORBHIP_UPDATE_NORMAL_DEPTH for
 * :227).  mode ORBHIP_GBA_STAGED (nLoopKF != 0): out->TcwGBA [rows][12] and out->posGBA [pcap][3] float are written and
 * out->kf_mark [rows] / out->pt_mark [pcap] uint8 are set to 1 for exactly the entries written (mnBAGlobalForKF == nLoopKF; the
 * caller clears the marks beforehand); Tcw and world are untouched.  The arrays of the other mode may be null.
 * Every vertex is written back as toCvMat(SE3Quat), the fixed rows too, and every included point as float -- also when the stop
 * byte was set on entry: ORBHIP_GBA_STOPPED, zero iterations, the poses are the inputs after the quaternion round trip.  When
 * no listed row has kf_id 0 nothing is fixed and the system stands on the damping alone, as in g2o.
 * An observation whose row is in the map and old enough but is not listed is a null vertex in the reference: the device form
 * skips it (it is no edge of its point) and counts it; the host form refuses such tables.
 * out->report [16] int32 = {status, key-frame vertices, free poses, included points, points removed for lack of edges, monocular
 * edges, stereo edges, observations skipped by the bad / maxKFid rule, null-vertex skips, outer iterations, trials, unknowns of
 * the reduced system, points listed for UpdateNormalAndDepth, 0, 0, samples of the stop byte}.
 * status: ORBHIP_GBA_OK; ORBHIP_GBA_STOPPED; ORBHIP_GBA_CAPACITY (more than ORBHIP_GBA_MAX_KF vertices, more than max_points
 * included points or max_edges edges: only the report is written, the caller falls back).
 * d_stop: nullable device byte = *pbStopFlag, sampled where g2o samples terminate(): at the top of every outer iteration and
 * in the condition of the trial loop after a rejected trial.  Only "set before the call" and "null" are deterministic.
 *
 * This entry synchronises: the call reads the state record back once after the setup and once per trial (one small pinned
 * copy, one stream synchronisation) and enqueues the next step from it; when it returns, the work is done.  One stream, no
 * cooperative launch.  The workspace belongs to the handle and is sized from rows, pcap, max_points and max_edges (the reduced
 * system takes 75 MB at 512 key frames).  rows, cap <= 4096 (ORBHIP_E_CAPACITY beyond); negative counts, cap < 1, np > pcap, a
 * list longer than its table, iterations < 1, a bad mode, max_points or max_edges < 1, cam->n_levels outside [1,
 * ORBHIP_MAX_LEVELS] or a null required pointer: ORBHIP_E_ARG; all refused before any device work.  The device form does not
 * range-check the tables' contents.  The entries read no environment variable. */
#define ORBHIP_GBA_MAX_KF   512
#define ORBHIP_GBA_IN_PLACE 0
#define ORBHIP_GBA_STAGED   1
#define ORBHIP_GBA_OK       0
#define ORBHIP_GBA_STOPPED  1
#define ORBHIP_GBA_CAPACITY 2
typedef struct orbhip_gba_tables {
    const void *kf_bad, *kf_id, *obs_start, *obs_kf, *obs_idx, *flags, *kps, *u_right;
    void *Tcw, *world;
} orbhip_gba_tables;
typedef struct orbhip_gba_out {
    void *TcwGBA, *posGBA, *kf_mark, *pt_mark, *point_list, *report;
} orbhip_gba_out;
int orbhip_global_bundle_adjustment_device(orbhip_matcher *m, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                                           const orbhip_gba_tables *tables, const float *inv_level_sigma2, const void *d_kf_list,
                                           int nkf, const void *d_pt_list, int npt, int iterations, int robust, int mode,
                                           int max_points, int max_edges, const void *d_stop, const orbhip_gba_out *out);
/* Host buffers, synchronous: one staging copy, the call, one read-back; what the call does not write keeps the caller's
 * values.  The same records with host pointers; stop points to a host byte or is NULL.  It range-checks what the device form
 * does not: list entries in [0, rows) / [0, np) and no row listed twice, obs_start non-decreasing from 0 or above, obs_kf in
 * [0, rows), obs_idx in [0, cap), the octaves of observed key points in [0, cam->n_levels), and it refuses a null vertex:
 * ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_global_bundle_adjustment(orbhip_matcher *m, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                                    const orbhip_gba_tables *tables, const float *inv_level_sigma2, const int32_t *kf_list, int nkf,
                                    const int32_t *pt_list, int npt, int iterations, int robust, int mode, int max_points,
                                    int max_edges, const uint8_t *stop, const orbhip_gba_out *out);
/* counters [2] = {stream synchronisations, kernel launches} of this handle's last global-bundle-adjustment call. */
int orbhip_global_bundle_adjustment_counters(orbhip_matcher *m, int32_t counters[2]);

/* The map update after a staged global bundle adjustment (src/LoopClosing.cc:676-737).  d_origins [n_origins] int32 =
 * mvpKeyFrameOrigins as rows; parent [rows] int32 and kf_bad [rows] uint8 (nullable): the children of a row are the rows that
 * are not bad whose parent it is, in ascending row where the reference iterates a std::set<KeyFrame*>; kf_mark, TcwGBA, Tcw
 * in/out; pt_mark, posGBA, flags, ref_kf [pcap] in; world in/out; TcwBefGBA [rows][12] float out.
 * The walk is breadth first from the origins in lpKFtoCheck order: a child whose mark is clear gets TcwGBA = (Tcw_child *
 * Twc_parent) * TcwGBA_parent and its mark; every child is queued; the popped row then gets TcwBefGBA = Tcw and Tcw = TcwGBA.
 * Twc_parent is formed from the parent's Tcw before that assignment (Rwc = Rcw^T, Ow = -Rwc tcw, KeyFrame::SetPose), a child's
 * Tcw is still its old pose.  At most `rows` rows are popped; an origin that is bad, outside the table or unmarked (it has no
 * TcwGBA) is not queued by the device form and refused by the host form.  Then every present point: marked, world = posGBA;
 * otherwise, if its reference row is marked and was popped, Xc = Rcw_bef Xw + tcw_bef and world = Rwc Xc + twc with the
 * inverse of the row's new pose; otherwise it is left (reference row unmarked, never reached, or -1).  Float arithmetic is
 * fp32, per row, left to right, the 4x4 products element by element over k = 0..3.
 * report [8] int32 = {rows popped, rows whose TcwGBA was propagated, points set from posGBA, points moved through their
 * reference row, points left, present points, 0, 0}.
 * Asynchronous on the matcher's stream, no host synchronisation, two launches.  rows <= 4096 (ORBHIP_E_CAPACITY beyond);
 * rows < 1, pcap < 0, n_origins < 0 or a null required pointer: ORBHIP_E_ARG, before any device work. */
typedef struct orbhip_gba_apply {
    const void *origins, *parent, *kf_bad, *pt_mark, *posGBA, *flags, *ref_kf;
    void *kf_mark, *TcwGBA, *Tcw, *world, *TcwBefGBA, *report;
} orbhip_gba_apply;
int orbhip_apply_global_ba_device(orbhip_matcher *m, int n_origins, int rows, int pcap, const orbhip_gba_apply *a);
/* Host buffers, synchronous; additionally range-checks origins (in [0, rows), not bad, marked), parent in [-1, rows) and
 * ref_kf in [-1, rows): ORBHIP_E_ARG, before the handle is looked at. */
int orbhip_apply_global_ba(orbhip_matcher *m, int n_origins, int rows, int pcap, const orbhip_gba_apply *a);

/* ---- creating new map points -------------------------------------------------------------------------------------
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452) for the current key frame and K neighbours in one call, up
 * to the point where the map graph is touched: `new MapPoint`, AddObservation and everything after :434 stay with the
 * caller, as does ComputeSceneMedianDepth (:256).  Replaces, per neighbour, the baseline gate (:244-261), ComputeF12
 * (:536-553), the epipole (src/ORBmatcher.cc:664-670), ORBmatcher::SearchForTriangulation (:657-823) and the loop body
 * :286-431 (parallax test, linear triangulation or UnprojectStereo, two positive-depth tests, two reprojection tests,
 * scale consistency).  The operation order of the float arithmetic, and the two stated choices (cos(2 atan2) as a rational
 * expression, one-sided Jacobi SVD of the 4x4 system), are in DESIGN.md section 3.
 *
 * Frames are rows of arrays in the extractor's output layout: d_kps [..][cap] orbhip_keypoint (mvKeysUn), d_desc
 * [..][cap][32], d_n [..] int32, d_u_right / d_depth [..][cap] float (mvuRight / mvDepth; both NULL = monocular), d_node
 * [..][cap] uint32 as orbhip_vocabulary_transform_device writes it, d_has_point [..][cap] uint8 (the slot already holds a
 * map point; NULL = none does), d_Tcw [..][12] = [Rcw | tcw] per frame row.  `cur` is the row of mpCurrentKeyFrame,
 * d_kf_index [K] int32 the neighbour rows: any order, gaps, repeats and `cur` itself are allowed.  One camera for all
 * frames (the reference itself uses mpCurrentKeyFrame->mbf for key frame 2, :406); mfScaleFactor of ratioFactor (:232) is
 * cam->scale_factors[1] (scale_factors[0] with one level).  level_sigma2 [cam->n_levels] = mvLevelSigma2 (host).
 * UnprojectStereo (:342, :346) is evaluated on d_kps; KeyFrame::UnprojectStereo reads mvKeys (src/KeyFrame.cc:620), which
 * equals mvKeysUn for the rectified stereo / RGB-D input this branch exists for.
 * Baseline gate: stereo / RGB-D (d_u_right given, d_median_depth NULL) skips a neighbour when baseline < cam->mb;
 * monocular (d_u_right NULL) needs d_median_depth [K] float = pKF2->ComputeSceneMedianDepth(2) per neighbour and skips
 * when (float)(baseline / median) < 0.01.
 * Outputs, row k = neighbour k, entry i = key point i of the current key frame: d_matches12 [K][cap] int32 (what
 * orbhip_search_for_triangulation returns for that pair), d_nmatches [K] int32, d_x3d [K][cap][3] float (the point where
 * one was computed, i.e. status 0 or >= ORBHIP_NEWPOINT_BEHIND_1, else zeros), d_status [K][cap] uint8 (ORBHIP_NEWPOINT_*,
 * one per way out of the loop body), d_skipped [K] uint8 (the baseline gate fired: nmatches 0, every entry NO_MATCH);
 * optional d_f12 [K][9] / d_epipole [K][2] float (zeros for a skipped row).  Entries >= n[cur] stay untouched.
 * has_point is read as it is at call time: INTEGRATION.md section 3 says how the caller applies the rows in order.
 * Asynchronous on the matcher's stream, no host synchronisation, no staging copy: three launches, four with check_ori.
 * cap <= 4096 (ORBHIP_E_CAPACITY beyond); bad arguments are refused before any device work; K == 0 or n[cur] == 0:
 * success, nothing written. */
#define ORBHIP_NEWPOINT_CREATED      0  /* passed every gate: the caller creates the MapPoint (:434) */
#define ORBHIP_NEWPOINT_NO_MATCH     1  /* SearchForTriangulation gave this key point no partner */
#define ORBHIP_NEWPOINT_LOW_PARALLAX 2  /* no stereo and very low parallax (:349) */
#define ORBHIP_NEWPOINT_W_ZERO       3  /* homogeneous coordinate 0 (:333) */
#define ORBHIP_NEWPOINT_BEHIND_1     4  /* z1 <= 0 (:355) */
#define ORBHIP_NEWPOINT_BEHIND_2     5  /* z2 <= 0 (:359) */
#define ORBHIP_NEWPOINT_REPROJ_1     6  /* reprojection error in the current key frame (:374, :385) */
#define ORBHIP_NEWPOINT_REPROJ_2     7  /* reprojection error in the neighbour (:400, :411) */
#define ORBHIP_NEWPOINT_ZERO_DIST    8  /* dist1 == 0 || dist2 == 0 (:422) */
#define ORBHIP_NEWPOINT_SCALE        9  /* scale consistency (:430) */
int orbhip_create_new_map_points_device(orbhip_matcher *m, int cur, int K, const void *d_kf_index, const orbhip_camera *cam,
                                        const void *d_Tcw, const void *d_kps, const void *d_desc, const void *d_n, int cap,
                                        const void *d_u_right, const void *d_depth, const void *d_node, const void *d_has_point,
                                        const void *d_median_depth, int only_stereo, int check_ori, const float *level_sigma2,
                                        void *d_matches12, void *d_nmatches, void *d_x3d, void *d_status, void *d_skipped,
                                        void *d_f12, void *d_epipole);
/* Host buffers, synchronous: one staging copy, one device call, one read-back.  cur / kfs[K]: views of the current key
 * frame and the neighbours (u_right set on all non-empty ones or on none); node_cur / node[k], has_point_cur / has_point[k]
 * (nullable, also per entry), depth_cur / depth[k] (stereo only): one entry per key point; Tcw_cur [12], Tcw [K][12];
 * median_depth [K] (monocular only).  Outputs are packed by the current key frame's count n = cur->n: matches12 [K][n],
 * nmatches [K], x3d [K][n][3], status [K][n], skipped [K], optional f12 [K][9] / epipole [K][2].  A key frame with more
 * than 4096 key points: ORBHIP_E_CAPACITY, as orbhip_search_for_triangulation. */
int orbhip_create_new_map_points(orbhip_matcher *m, const orbhip_frame_view *cur, const uint32_t *node_cur,
                                 const uint8_t *has_point_cur, const float *depth_cur, const float *Tcw_cur, int K,
                                 const orbhip_frame_view *const *kfs, const uint32_t *const *node, const uint8_t *const *has_point,
                                 const float *const *depth, const float *Tcw, const float *median_depth,
                                 const orbhip_camera *cam, int only_stereo, int check_ori, const float *level_sigma2,
                                 int32_t *matches12, int32_t *nmatches, float *x3d, uint8_t *status, uint8_t *skipped,
                                 float *f12, float *epipole);

/* Launch on a caller-owned hipStream_t (NULL: the handle's own stream); wait for the handle's stream. */
int orbhip_matcher_set_stream(orbhip_matcher *m, void *stream);
int orbhip_matcher_sync(orbhip_matcher *m);
/* Test hook: overwrite the handle's workspaces with `byte` (0 .. 255).  Every allocated device scratch slot is filled on the
 * handle's stream, ordered after earlier calls and before later ones; then, after a stream synchronise, the pinned staging
 * and read-back buffers and the pinned state records of the essential-graph and global-bundle-adjustment calls.  The two
 * slots that cache a host-built table (the RANSAC iteration tables of the Sim3 and PnP setup calls) are invalidated, so the
 * next setup call uploads its table again.  No slot carries state from one public call to the next, so none is excluded.
 * bytes_filled (nullable): the number of bytes written.  Every call of this header must give the same results after it. */
int orbhip_matcher_fill_scratch(orbhip_matcher *m, int byte, unsigned long long *bytes_filled);

/* Frame::ComputeStereoMatches.  The image pyramids are the ones left in the two extractor
 * handles by their last extract call (frame indices frame_l / frame_r of those batches), i.e.
 * mpORBextractorLeft/Right->mvImagePyramid.  keys/desc: host buffers (mvKeys, mDescriptors,
 * mvKeysRight, mDescriptorsRight).  mb is passed explicitly (the reference reads it before
 * assignment, src/Frame.cc:496 vs :114).  u_right[nl], depth[nl] out (mvuRight, mvDepth).
 * At most 2^20 right keypoints (ORBHIP_E_CAPACITY beyond: the match key holds distance << 20 | index). */
int orbhip_compute_stereo_matches(orbhip_matcher *m, orbhip_extractor *left, int frame_l,
                                  orbhip_extractor *right, int frame_r,
                                  const orbhip_keypoint *keys_l, const uint8_t *desc_l, int nl,
                                  const orbhip_keypoint *keys_r, const uint8_t *desc_r, int nr,
                                  float mbf, float mb, float *u_right, float *depth, int *nmatches);

/* Device-resident, batched Frame::ComputeStereoMatches over `pairs` stereo pairs: pair p uses frame l0 + p*ls of
 * the left extractor's last batch (pyramid and rows of d_kps_l / d_desc_l / d_n_l) and frame r0 + p*rs of the right
 * one (left and right may be the same handle holding an interleaved batch: l0=0, ls=2, r0=1, rs=2).  Arrays are in
 * the extractor's output layout with stride `cap`.  Outputs: d_u_right / d_depth [pairs][cap] float (entries beyond
 * the left frame's count are untouched), d_nmatches [pairs] int32.  Asynchronous on the matcher's stream; the caller
 * orders it after the extractions (same stream, or orbhip_extractor_sync).  cap <= 2^20 (ORBHIP_E_CAPACITY beyond). */
int orbhip_compute_stereo_matches_device(orbhip_matcher *m, orbhip_extractor *left, int l0, int ls,
                                         orbhip_extractor *right, int r0, int rs, int pairs, const void *d_kps_l,
                                         const void *d_desc_l, const void *d_n_l, const void *d_kps_r,
                                         const void *d_desc_r, const void *d_n_r, int cap, float mbf, float mb,
                                         void *d_u_right, void *d_depth, void *d_nmatches);

#ifdef __cplusplus
}
#endif
#endif /* ORBHIP_H */
