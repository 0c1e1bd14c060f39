// Internal (non-ABI) definitions shared by the extractor and matcher translation units.
#pragma once
#include "orbhip_common.h"
#include "pyr_span.h"

#include <vector>

struct orbhip_extractor;
namespace orbhip {
struct BlurW { int w[7]; };
struct TileDesc { short level, tx, ty, pad; };
constexpr int kBlurTW = 64, kBlurTH = 58;
// LDS geometry of k_fast_cells, derived on the host from the largest cell of the image size
struct FastLds {
    int strideW;      // row stride in dwords (odd) = the kernel's template argument: staged dwords + one real dword on the left
    int scoreW;       // score-map row stride in dwords (= strideW - 2)
    int img_words, score_words, list_words;
    int list_cap;     // survivor-list entries (uint16); a round with more survivors is repeated in row bands
};
// How k_fast_cells brings a cell's sub-image to LDS.  The product library has one way (kFastStage); development builds
// instantiate the others beside it for tools/fast_ab.py (orbhip_dev_set_fast_variant).
constexpr int kFastStageBatch = 0;       // lane = (row mod RPI, dword column) through registers, whole batches of row groups
constexpr int kFastStageDense = 1;       // lane = row * SW + dword column through registers, exactly the cell's rows
constexpr int kFastStageDma = 2;         // the same lanes and rows by global_load_lds_dword: no data register, no LDS store
constexpr int kFastStage = kFastStageDma;
// What a cell-wave pays once, around its loops ("what a cell-wave pays once").  The product library has the set
// that was kept (kFastFix); development builds instantiate the steps towards it for tools/fast_ab.py.
constexpr int kFastFixDiv = 1;           // no run-time division: band size and banded-NMS index split from the cell record
constexpr int kFastFixDma = 2;           // the staging's row groups in one statement: M0 saved once, running scalar adds
constexpr int kFastFixMask = 4;          // the live-lane mask of the dense loop and the compaction seed on the scalar unit:
                                         // measured slower (three scalar instructions per trip for two vector ones), not kept
constexpr int kFastFix = kFastFixDiv | kFastFixDma;
// One FAST cell as k_fast_cells2 wants it: every derived quantity precomputed, one 32-byte scalar load per wavefront
struct alignas(32) FastCell {
    uint32_t src_off;        // byte offset inside a frame's pyramid block of LDS (row 0, col 0): row y0, column gxb - 4
    uint32_t magic;          // ceil(2^18 / ngrp), ngrp = four-pixel groups per detection row
    unsigned short pitch;    // row pitch of the level's padded plane
    short kpx, kpy;          // keypoint = (LDS col + kpx, detection row + kpy) relative to (minBorderX, minBorderY)
    unsigned char sw, sh, a; // sub-image size; a = x0 & 3
    unsigned char img;       // 1: src_off / pitch address the caller's image (level 0 without a materialised plane)
    unsigned short band_items;   // (list_cap / (4 * ngrp)) * ngrp: work items of a row band that cannot overflow the survivor list
    uint32_t nms_magic;      // ceil(2^20 / dw), dw = detection columns: floor(i / dw) = (i * nms_magic) >> 20 for i < dw * dh
    unsigned char pad[8];
};
static_assert(sizeof(FastCell) == 32, "FastCell is one s_load_dwordx8");
struct FastParams {
    uint32_t frame_bytes, rcp_cells;
    int ncells_total, slot_cap, ini_th, min_th, img_words, score_words, list_cap;
    int dev;   // development builds only: timing floors / stamped kernel
};
// Tables of the pyramid kernels (k_pyr_base / k_pyr_rows): a wavefront owns kPyrRows padded destination rows (its row
// records come through scalar loads) and one destination dword (resize) or 16-byte group (level-0 copy) per lane.
struct PyrRow { int s0, s1; uint32_t B0, B1; };        // source rows of a destination row; Q11 row coefficients << 12
struct PyrCol { uint32_t sel[4]; uint32_t alv[4]; };   // per destination dword: v_perm selectors of the 4 tap pairs inside the
                                                       // 8-byte source window; Q11 column coefficients a0 | a1 << 16
struct PyrCopyCol { uint32_t selA[4], selB[4]; };      // level 0: 16 destination bytes gathered from a 16-byte source window
struct PyrLevelTab {
    const PyrRow *row;       // [prows]                      (resize only)
    const void *col;         // [words] PyrCol / PyrCopyCol
    const uint32_t *lo;      // [words] first source byte of the lane's window
    int words;               // lanes per destination row: dwords (resize) or 16-byte groups (copy)
    int nchunks, chunk_w;    // a row is split into nchunks runs of chunk_w <= 64 lanes
    uint32_t rcp_chunks;     // ceil(2^32 / nchunks)
    int units;               // wavefront work items = row groups x nchunks
    int prows, pitch;        // destination rows the tables cover, row pitch of the plane
    unsigned plane_off;      // destination byte of table row 0, lane 0, inside a frame's pyramid block: the padded plane for
                             // level 0; for a level >= 1 the first dword of its eager span (pyr_span.h: row0, col0)
    int src_h, src_pitch;    // source: rows (level-0 copy: REFLECT_101 of the row index), pitch for levels >= 2
    unsigned src_off;        // source ROI inside the frame's pyramid block (levels >= 2)
};
int ensure_level0(orbhip_extractor *e, hipStream_t consumer);   // orbhip_extractor.hip
int ensure_frames(orbhip_extractor *e, hipStream_t consumer);   // orbhip_extractor.hip

// orbhip_localmap.hip: the tables, in/out lists and outputs of orbhip_update_local_map_device, and its workspace
struct LocalMapArgs {
    const int *slot_point, *n;          // [rows][cap], [rows]
    const uint8_t *kf_bad;              // [rows] or null
    const int *covis;                   // [rows][10]
    const int *child_start, *child, *parent;
    const int *obs_start, *obs_kf;
    const uint8_t *flags;               // [pcap]
    const float *world, *normal, *max_dist, *min_dist;
    const uint8_t *point_desc;          // [pcap][32]
    int *frame_point;                   // [frames][cap], in/out
    const int *frame_n;
    int *local_kf, *n_local_kf;         // [frames][rows], [frames], in/out
    int *votes, *local_point;
    float *world_l, *normal_l, *max_dist_l, *min_dist_l;
    uint8_t *desc_l, *flags_l;
    int *np_l;
    uint8_t *taken;
    int *report;                        // [frames][8]
    // workspace: first [frames][pcap] (reset by the call), free_pt [frames][pcap] (0 = the frame holds the point, reset
    // by the call), base [frames][rows] (winner counts, then their exclusive scan)
    uint32_t *first;
    uint8_t *free_pt;
    int *base;
    int frames, rows, cap, pcap;
};
size_t local_map_workspace_bytes(int frames, int rows, int pcap);
int launch_local_map(hipStream_t stream, LocalMapArgs A, void *workspace);
// n_to_match and F.mvpMapPoints[bestIdx] = pMP after the points search of orbhip_track_local_map_device
int launch_local_map_apply(hipStream_t stream, int frames, int cap, int pcap, const void *q, const int *np_l, const int *frame_n,
                           const int *assign, const int *local_point, int *frame_point, int *report);

// orbhip_covisibility.hip: the tables, the graph state and the workspace of orbhip_update_connections_device
struct CovisArgs {
    const int *slot_point, *n;          // [rows][cap], [rows]
    const int *obs_start, *obs_kf;
    const uint8_t *flags;               // [pcap]
    int *conn_w, *ord_kf, *ord_w;       // [rows][rows] each, in/out
    int *n_ord, *covis;                 // [rows], [rows][10]
    uint8_t *first_conn;
    int *parent;
    // null: bank row c is row c of every array above.  The host entry keeps only the rows a call can reach on the device,
    // row_slot[c] = where row c is (-1: not resident); the columns of conn_w / ord_* stay bank rows.
    const int *row_slot;
    const int *update_rows;             // [U]
    int *report;                        // [U][8]
    // workspace: counter [U][rows] (reset by the call), summary [U][4] = {voted rows, maximum, its row, rows >= 15}
    int *counter, *summary;
    int rows, cap, np, id0_row, U;
};
struct CovisTargetArgs {
    const int *ord_kf, *n_ord;          // [rows][stride] (the head of each list), [rows]
    const int *row_slot;                // as in CovisArgs
    const uint8_t *kf_bad;              // [rows] or null
    const int *cur;                     // [Q]
    int *targets, *counts;              // [Q][nn * (1 + nn2)], [Q]
    int rows, stride, nn, nn2;
};
size_t covis_workspace_bytes(int U, int rows);
int launch_update_connections(hipStream_t stream, CovisArgs A, void *workspace);
int launch_covisible_targets(hipStream_t stream, CovisTargetArgs A, int Q);
int launch_children_from_parents(hipStream_t stream, int rows, const int *parent, const uint8_t *kf_bad, int *child_start, int *child);

// UpdateBestCovisibles (src/KeyFrame.cc:138-157) of one bank row by one workgroup of 256 threads, shared by k_cv_apply and
// k_cull_apply.  The caller has filled s_key[0 .. N) (N the power of two at or above rows, at least 2) with
// weight << 32 | row for the entries of the list and 0 elsewhere, and counted its own entries in `mine`.  A bitonic sort
// in LDS, descending: larger weight first, the higher row first among equal weights.  It stores the n_out entries to
// okf / ow and nothing behind them, the head to covis10, and n_out to *n_ord.  Returns n_out in every thread; s_key then
// holds the sorted keys.
__device__ __forceinline__ int cv_resort_row(unsigned long long *s_key, int *s_cnt, int mine, int N, int *okf, int *ow, int *covis10,
                                             int *n_ord)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    mine = wave_sum(mine);
    if (lane == 0) s_cnt[wv] = mine;
    __syncthreads();
    const int n_out = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += 256) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = s_key[i], b = s_key[x];
                    if ((i & k) == 0 ? a < b : a > b) { s_key[i] = b; s_key[x] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n_out; i += 256) {
        const unsigned long long key = s_key[i];
        okf[i] = (int)(unsigned)key;
        ow[i] = (int)(key >> 32);
    }
    if (tid < 10) covis10[tid] = tid < n_out ? (int)(unsigned)s_key[tid] : -1;
    if (tid == 0) *n_ord = n_out;
    return n_out;
}

// orbhip_culling.hip: the tables, the graph state and the workspace of orbhip_cull_map_points_device /
// orbhip_cull_key_frames_device
struct CullArgs {
    const orbhip_keypoint *kps;         // [rows][cap]
    const float *u_right, *depth;       // [rows][cap], nullable
    const int *n;                       // [rows]
    const int *obs_start, *obs_kf, *obs_idx, *ref_obs;
    const uint8_t *not_erase;           // [rows] or null
    int *slot_point;                    // [rows][cap], in/out
    uint8_t *flags, *kf_bad, *to_be_erased;
    int *conn_w, *ord_kf, *ord_w, *n_ord, *covis, *parent;
    int *child_start, *child;
    int *obs_start_out, *obs_kf_out, *obs_idx_out, *ref_obs_out;
    // map points
    const int *recent, *found, *visible, *first_kf_id;
    int *recent_out, *n_recent_out;
    uint8_t *status;
    // key frames
    const int *cand_in;                 // [U]
    int *report;                        // [U][8]
    // workspace, reset by every call: nobs [np] = Observations(), alive [obs_cap] (1 = the entry is in mObservations),
    // ref_cur [np] = position of mpRefKF's entry in the list as passed in (-1: none), owner [np] = first list position of a
    // recent point, cand [U] = the call's copy of the list, verdict [U]
    int *nobs, *alive, *ref_cur, *owner, *cand, *verdict;
    int rows, cap, np, obs_cap, id0_row, U, R, cur_kf_id, th_obs, mono;
    float th_depth;
};
size_t cull_workspace_bytes(int np, int obs_cap, int U);
int launch_cull_map_points(hipStream_t stream, CullArgs A, void *workspace);
int launch_cull_key_frames(hipStream_t stream, CullArgs A, void *workspace);

// orbhip_sim3.hip: the tables, the solver state and the workspace of orbhip_sim3_setup_device / orbhip_sim3_iterate_device
constexpr int kSim3HypFloats = 40;      // T12 [12], T21 [12], R12 [9], t12 [3], s12, padding
struct Sim3Args {
    const int *slot_point, *n;          // [rows][cap], [rows]
    const int *obs_start, *obs_kf, *obs_idx;
    const uint8_t *flags;               // [pcap]
    const float *world, *Tcw;           // [pcap][3], [rows][12]
    const orbhip_keypoint *kps;         // [rows][cap]
    const int *kf_index, *matched12;    // [C], [C][cap]
    const int *limit_tab;               // [cap + 1], built on the host
    float *x1, *x2, *p1, *p2;           // [C][cap][3], [C][cap][2]
    uint32_t *max_err1, *max_err2;      // [C][cap]
    int *slot1, *n_corr, *n1, *limit, *state;
    const int *draws;                   // [C][max_its][3]
    float *sim3;                        // [C][16]
    uint8_t *inliers;                   // [C][cap]
    int *report;                        // [C][8]
    // workspace of one iterate call, j = iteration number - mnIterations at the start of the call:
    // hyp [C][n_iter][kSim3HypFloats], count [C][n_iter], mask [C][n_iter][cap16] (bit i & 15 of unit i >> 4 = correspondence i)
    float *hyp;
    int *count;
    uint16_t *mask;
    uint32_t thr[ORBHIP_MAX_LEVELS];    // the truncated thresholds per pyramid level
    float fx, fy, cx, cy;
    int C, cur, rows, cap, np, match_form, n_levels, max_its, n_iter, min_inliers, fix_scale, cap16;
};
size_t sim3_workspace_bytes(int C, int n_iter, int cap);
int launch_sim3_setup(hipStream_t stream, Sim3Args A);
int launch_sim3_iterate(hipStream_t stream, Sim3Args A, void *workspace);

// orbhip_pnp.hip: the inputs, the solver record and the workspace of orbhip_pnp_setup_device / orbhip_pnp_iterate_device
struct PnpArgs {
    const orbhip_keypoint *kps;         // [n]
    const int *matches, *kf_index;      // [C][cap], [C]
    const int *slot_point;              // [rows][cap]
    const uint8_t *flags;               // [pcap]
    const float *world;                 // [pcap][3]
    const int *tab;                     // [cap + 1][2]: adjusted (min inliers, limit) per correspondence count
    float max_err_lv[ORBHIP_MAX_LEVELS];   // mvLevelSigma2[l] * th2, a float product
    float *p2d, *p3d, *max_err;         // [C][cap][2], [C][cap][3], [C][cap]
    int *kp_index, *n_corr, *min_inliers, *limit, *state;
    uint8_t *best_inliers;              // [C][cap]
    float *best_Tcw;                    // [C][12]
    const int *draws;                   // [C][draw_rows][4]
    float *Tcw;                         // [C][12]
    uint8_t *inliers;                   // [C][cap]
    int *report;                        // [C][8]
    // workspace of one iterate call, j = iteration number - mnIterations at the start of the call, e = refinement entry:
    // hyp [C][W][12] (R, t in double), count / is_rec [C][W], mask [C][W][cap], ref_T [C][W+1][12], ref_cnt [C][W+1],
    // ref_mask [C][W+1][cap]
    double *hyp;
    int *count, *is_rec, *ref_cnt;
    uint8_t *mask, *ref_mask;
    float *ref_T;
    double fu, fv, uc, vc;
    int C, n, cap, rows, np, match_form, n_levels, n_iter, draw_rows, W;
};
size_t pnp_workspace_bytes(int C, int W, int cap);
int launch_pnp_setup(hipStream_t stream, PnpArgs A);
int launch_pnp_iterate(hipStream_t stream, PnpArgs A, void *workspace);
}  // namespace orbhip

#include "orbhip_poseopt_core.h"

namespace orbhip {
// orbhip_poseopt.hip: the arguments of orbhip_pose_optimization_device
constexpr int kPoCapMax = 4096;
struct PoArgs {
    const orbhip_keypoint *kps;         // [frames][cap]
    const int *n;                       // [frames]
    const float *u_right;               // [frames][cap] or nullptr
    const float *world;                 // [wrows][pcap][3]
    const uint8_t *point_flags;         // [wrows][pcap] or nullptr
    const int *world_row;               // [frames] or nullptr
    float *Tcw;                         // [frames][12]
    int *frame_point;                   // [frames][cap]
    uint8_t *outlier;                   // [frames][cap]
    int *discarded;                     // [frames][cap] or nullptr
    int *report;                        // [frames][8]
    float inv[ORBHIP_MAX_LEVELS];       // mvInvLevelSigma2
    PoCam cam;
    int frames, cap, wrows, pcap, n_levels, mode, flags;
};
int launch_pose_optimization(hipStream_t stream, PoArgs A);
}  // namespace orbhip

#include "orbhip_sim3opt_core.h"

namespace orbhip {
// orbhip_sim3opt.hip: the arguments of orbhip_optimize_sim3_device
struct S3oArgs {
    S3oTables T;                        // slot_point, n, the observation table, flags
    const orbhip_keypoint *kps;         // [rows][cap]
    const float *world, *Tcw;           // [pcap][3], [rows][12]
    const int *kf_index;                // [C]
    const uint8_t *select;              // [C] or nullptr
    const float *sim3;                  // [C][16]
    int *matched12;                     // [C][cap]
    double *S12;                        // [C][8]
    float *Scw;                         // [C][12] or nullptr
    int *report;                        // [C][8]
    float inv[ORBHIP_MAX_LEVELS];       // mvInvLevelSigma2
    S3oCam cam;
    double delta, th2;                  // (float)sqrt(th2) and th2, widened
    int C, n_levels, fix_scale;
};
int launch_optimize_sim3(hipStream_t stream, S3oArgs A);
}  // namespace orbhip

#include "orbhip_lba_core.h"

namespace orbhip {
// orbhip_lba.hip: the tables, the outputs and the scalars travel in LbaWs; the workspace pointers are carved by the launch
size_t lba_workspace_bytes(LbaWs W);
int launch_local_bundle_adjustment(hipStream_t stream, LbaWs W, void *workspace);
}  // namespace orbhip

#include "orbhip_essgraph_core.h"

namespace orbhip {
// orbhip_essgraph.hip: the tables, the outputs and the scalars travel in EgWs; the workspace pointers are carved by the launch.
// h_state is pinned host memory the call reads the state record into once per trial; counters [2] (nullable) receives the
// synchronisations and the launches of the call.
size_t eg_workspace_bytes(EgWs W);
int launch_optimize_essential_graph(hipStream_t stream, EgWs W, void *workspace, EgState *h_state, int *counters);
}  // namespace orbhip

#include "orbhip_gba_core.h"

namespace orbhip {
// orbhip_gba.hip: as above; h_state is a pinned LbaState, read once after the setup and once per trial
size_t gba_workspace_bytes(GbaWs G);
int launch_global_bundle_adjustment(hipStream_t stream, GbaWs G, void *workspace, LbaState *h_state, int *counters);
size_t gba_apply_workspace_bytes(GbaApply A);
int launch_apply_global_ba(hipStream_t stream, GbaApply A, void *workspace);
}  // namespace orbhip

struct orbhip_extractor {
    int nfeatures = 0;
    double scaleFactor = 1.2;
    int nlevels = 8, iniTh = 20, minTh = 7, device = 0;
    float sf[ORBHIP_MAX_LEVELS], isf[ORBHIP_MAX_LEVELS], sig2[ORBHIP_MAX_LEVELS], isig2[ORBHIP_MAX_LEVELS];
    int nfeat[ORBHIP_MAX_LEVELS];
    int umax[orbhip::kHalfPatch + 1];
    orbhip::BlurW blurw;
    hipStream_t stream = nullptr;       // stream every launch of this handle goes to
    hipStream_t own_stream = nullptr;   // created with the handle; `stream` may be re-pointed
    // profiling: ring of event sets (kProfEv events per extract call), averaged on read-out
    static constexpr int kProfEv = 5;   // before the pyramid, after pyramid / FAST / octree / descriptors
    static constexpr int kProfRing = 256;
    std::vector<hipEvent_t> ev;         // kProfRing * kProfEv, created lazily
    bool profiling = false;
    long prof_calls = 0;

    // geometry (bound to an image size)
    bool bound = false;
    orbhip::PyrGeom G;
    std::vector<orbhip::CellDesc> cells;
    std::vector<orbhip::TileDesc> tiles;
    int octree_maxn = 512;
    int octree_threads = 256;   // workgroup size of k_octree (256 / 512 / 1024)
    orbhip::FastLds fast_lds;   // k_fast_cells dynamic LDS carve-up
    int fast_lds_bytes = 0;
#ifdef ORBHIP_DEVTOOLS
    int stage_mask = 31;        // development build (tools/coexec.py): stages launch_pipeline runs
    int fast_variant = 0;       // development build (tools/fast_ab.py): ones 2 stamped build, 3 / 4 timing floors; tens the staging;
                                // hundreds the fixed-cost parts
    int fast_stage = orbhip::kFastStage;   // staging of k_fast_cells selected by the tens of fast_variant (orbhip_dev_set_fast_variant)
    int fast_fix = orbhip::kFastFix;       // kFastFix* parts selected by its hundreds
    int octree_variant = 0;     // development build (tools/octree_ab.py): bit 0 workspace path for all, bit 1 stamped build
#endif
    orbhip::CellDesc *d_cells = nullptr;
    std::vector<orbhip::FastCell> cells2;
    orbhip::FastCell *d_cells2 = nullptr;
    orbhip::FastParams fast_params;
    int num_cus = 256;              // compute units of the device (launch shaping)
    orbhip::TileDesc *d_tiles = nullptr;
    int *d_desc_tab = nullptr;      // descriptor kernel tables: disc chunks {dword index, u weights, v weights}[4][64], row-pass items[64]
    bool blur_valid = false;        // d_blur holds the blurred planes of the last batch
    // mvImagePyramid[0] on demand (orbhip_extractor_set_lazy_level0)
    bool lazy_l0 = false;           // the caller's choice
    bool l0_in_image = false;       // the last extraction read level 0 from the image and did not write the padded plane
    bool l0_valid = true;           // d_pyr holds the padded level-0 planes of the last batch
    int cells_stride = 0;           // image row stride the level-0 entries of d_cells2 are built for (0: the padded plane)
    const uint8_t *src_images = nullptr; int src_stride = 0; size_t src_frame_stride = 0;   // image buffer of the last extraction
    hipEvent_t ev_l0 = nullptr;
    // the REFLECT_101 frames of levels >= 1 on demand (ensure_frames): an extraction writes each level's eager span only
    bool frames_valid = true;       // d_pyr holds the full frames of levels >= 1 of the last batch
    // stage gates (orbhip_extractor_set_stage_gate): events other pipelines' handles record / wait for
    hipEvent_t gate_wait[4] = {nullptr, nullptr, nullptr, nullptr}, gate_rec[4] = {nullptr, nullptr, nullptr, nullptr};
    float4 *d_patternf = nullptr;   // rBRIEF pattern as floats: (x0, y0, x1, y1) per test
    uint8_t *d_pyrtab = nullptr;    // row / column tables of the pyramid kernels
    orbhip::PyrLevelTab ptab[ORBHIP_MAX_LEVELS];
    bool ptab_rows[ORBHIP_MAX_LEVELS];   // level goes through the table-driven resize (all its tap windows fit 8 bytes)

    // per-batch-capacity buffers
    int batch_cap = 0;
    int last_batch = 0;
    uint8_t *d_pyr = nullptr, *d_blur = nullptr;
    int *d_cell_cnt = nullptr;
    uint32_t *d_cell_kp = nullptr;
    uint32_t *d_keys = nullptr;
    unsigned short *d_knode = nullptr;
    uint32_t *d_sel = nullptr;
    int *d_sel_cnt = nullptr;
    int *d_status = nullptr;
    // colour input (orbhip_extract_color*): the grey frames k_cvt_gray writes, which the pipeline then reads as "the image".
    // Allocated by the first colour extraction of a (geometry, batch) and freed with the per-batch buffers.
    uint8_t *d_gray = nullptr;
    int gray_cap = 0;               // frames d_gray holds
    int gray_w[3] = {4899, 9617, 1868}, gray_shift = 14;   // wR, wG, wB (orbhip_extractor_set_gray_weights)
    uint8_t *d_cimg = nullptr; size_t d_cimg_bytes = 0;    // host colour entries: packed colour frames on the device ...
    uint8_t *h_cin = nullptr; size_t h_cin_bytes = 0;      // ... and their page-locked staging
    // stereo rectification (orbhip_extract_remap*): per-destination-pixel records of the installed map, the weight table,
    // and the sizes the map was built for.  The rectified frames go to d_gray; the host entries stage through d_cimg / h_cin.
    uint2 *d_rmap = nullptr;
    int rmap_drows = 0, rmap_dcols = 0, rmap_srows = 0, rmap_scols = 0;
    uint16_t *d_rtab = nullptr;
    bool rtab_dirty = true;
    std::vector<uint16_t> rtab;     // 1024 x 4 (orbhip_extractor_set_remap_table); empty = the default
    // staging for the host-pointer API
    uint8_t *d_img = nullptr; size_t d_img_bytes = 0;
    orbhip_keypoint *d_okp = nullptr; uint8_t *d_odesc = nullptr; int *d_on = nullptr;
    size_t out_slots = 0;   // keypoint slots allocated in d_okp / d_odesc
    int out_batch = 0;      // entries allocated in d_on
    // host-pointer API: H2D copy + 13 launches + 4 D2H copies captured once per (batch, cap) and replayed with one
    // hipGraphLaunch -- a single frame is launch-bound, not GPU-bound
    hipGraphExec_t graph_exec = nullptr;
    int graph_batch = 0, graph_cap = 0;
    // chunked host path: copy-in / copy-out streams and per-chunk events (created on first use)
    hipStream_t s_in = nullptr, s_out = nullptr;
    std::vector<hipEvent_t> ev_chunk;
    // pinned host staging (pageable 2-D copies are an order of magnitude slower than one pinned DMA)
    uint8_t *h_in = nullptr; size_t h_in_bytes = 0;
    uint8_t *h_out = nullptr; size_t h_out_bytes = 0;
};

