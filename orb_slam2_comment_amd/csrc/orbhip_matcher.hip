// MI355X (gfx950) descriptor matching behind the C ABI of include/orbhip.h.
// Replaces ORBmatcher::SearchByProjection (x2), SearchForInitialization,
// DescriptorDistance (src/ORBmatcher.cc) and Frame::ComputeStereoMatches
// (src/Frame.cc:466-640).
//
// Structure: a fully parallel "window search" kernel (16 or 64 lanes per query:
// Frame::GetFeaturesInArea membership test + 256-bit XOR/popcount Hamming
// distance, candidates compacted with wave ballots and sorted by
// (distance, reference visiting order)), followed by a one-workgroup-per-pair
// "resolve" kernel that reaches the outcome of the reference's order-dependent
// bookkeeping (slots taken by earlier queries, match stealing, rotation
// histogram) by parallel rounds over state held in LDS.  Integer/bitwise path:
// no MFMA.
#include "orbhip_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <vector>

namespace orbhip {

constexpr int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;
constexpr int GRID_ROWS = 48, GRID_COLS = 64;   // include/Frame.h:37-38
constexpr int kResolveMax = 4096;               // LDS-resident state of the resolve kernels
constexpr uint32_t kNoCell = 0xffffffffu;

struct DevFrame {
    int n;
    const orbhip_keypoint *keys;
    const uint8_t *desc;
    const float *u_right;  // nullable
    float min_x, min_y, inv_w, inv_h;
};

// Pair p of a call (blockIdx.y, or blockIdx.x for one workgroup per pair) uses element strides cap / qcap.  A host-pointer
// call is a one-pair batch: cap = n, qcap = nq and null count pointers.
struct Batch {
    const int *n_dev;    // per-frame train keypoint counts, or null (count = cap = F.n)
    const int *nq_dev;   // per-pair query counts, or null (count = qcap)
    int cap, qcap;
    int t0 = 0, ts = 1;    // train side of pair p = frame t0 + p*ts of the extractor-layout arrays
    int qd0 = 0, qds = 1;  // query descriptors of pair p = frame qd0 + p*qds of their array
};
__device__ __forceinline__ void batch_frame(DevFrame &F, const Batch &B, int pair)
{
    const size_t f = (size_t)(B.t0 + pair * B.ts);
    F.keys += f * B.cap;
    F.desc += f * B.cap * 32;
    if (F.u_right) F.u_right += f * B.cap;
    if (B.n_dev) F.n = min(B.n_dev[f], B.cap);
}

__device__ __forceinline__ int hamming256(const uint32_t *a, const uint32_t *b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += __popc(a[i] ^ b[i]);
    return d;
}
// the same against a descriptor that arrived as two 16-byte loads
__device__ __forceinline__ int hamming256(const uint32_t (&q)[8], uint4 d0, uint4 d1)
{
    return __popc(q[0] ^ d0.x) + __popc(q[1] ^ d0.y) + __popc(q[2] ^ d0.z) + __popc(q[3] ^ d0.w) +
           __popc(q[4] ^ d1.x) + __popc(q[5] ^ d1.y) + __popc(q[6] ^ d1.z) + __popc(q[7] ^ d1.w);
}

// ---- the frame grid (Frame::PosInGrid, Frame::GetFeaturesInArea), the one home of its rules ------------------------
// Bit-exactness against the reference hangs on these: `round` in PosInGrid, floor / ceil and the float operation order
// ((x - min_x) - r) * inv_w in the cell window, the strict |dx| < r, Fuse's chi-square gate compared in double.
//
// Frame::PosInGrid (src/Frame.cc:382-392): the cell posX * 48 + posY of a key point, -1 when it is rejected.
__device__ __forceinline__ int grid_cell(float x, float y, float min_x, float min_y, float inv_w, float inv_h)
{
    const int px = (int)roundf(__fmul_rn(__fsub_rn(x, min_x), inv_w));
    const int py = (int)roundf(__fmul_rn(__fsub_rn(y, min_y), inv_h));
    return (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) ? -1 : px * GRID_ROWS + py;
}
// The cells a window of radius r around (x, y) covers (src/Frame.cc:332-346), clamped to the grid.  empty() = either of the
// reference's early exits (nMinCell >= 64 / 48, nMaxCell < 0) or a reversed range, over which its loops do not run.
struct CellWindow {
    int x0, x1, y0, y1;
    __device__ __forceinline__ bool empty() const
    {
        // `|`, not `||`: one straight-line test, no branch around the y terms
        return (x0 >= GRID_COLS) | (x1 < 0) | (y0 >= GRID_ROWS) | (y1 < 0) | (x1 < x0) | (y1 < y0);
    }
};
__device__ __forceinline__ CellWindow cell_window(float x, float y, float r, float min_x, float min_y, float inv_w,
                                                  float inv_h)
{
    CellWindow W;
    W.x0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, min_x), r), inv_w)));
    W.x1 = min(GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, min_x), r), inv_w)));
    W.y0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, min_y), r), inv_h)));
    W.y1 = min(GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, min_y), r), inv_h)));
    return W;
}
constexpr int kGridCells = GRID_COLS * GRID_ROWS;
struct GridRec { float x, y; int octave; uint32_t key; };   // a key point in the CSR grid of k_grid_build; key = cell << 20 | index
struct SigmaTab { float inv_sigma2[ORBHIP_MAX_LEVELS]; };
// The candidate test of the window search (the loop bodies of SearchByProjection / SearchForInitialization over
// GetFeaturesInArea) for the record at CSR position p: level window, |dx|,|dy| < r, the stereo gate (rur[p] is loaded only
// when it applies) and the acceptance cut.  key = dist << 32 | R.key whatever ok says.
struct WindowHit { bool ok; unsigned long long key; };
__device__ __forceinline__ WindowHit window_candidate(const GridRec *__restrict__ rec, const uint4 *__restrict__ rdesc,
                                                      const float *__restrict__ rur, int p, const orbhip_query &Q,
                                                      const uint32_t (&qd)[8], bool stereo_gate, int max_dist)
{
    const GridRec R = rec[p];
    const uint4 d0 = rdesc[2 * p], d1 = rdesc[2 * p + 1];
    bool ok = true;
    if ((Q.min_level > 0) || (Q.max_level >= 0)) {   // bCheckLevels
        if (R.octave < Q.min_level) ok = false;
        if (Q.max_level >= 0 && R.octave > Q.max_level) ok = false;
    }
    ok = ok && fabsf(__fsub_rn(R.x, Q.u)) < Q.radius && fabsf(__fsub_rn(R.y, Q.v)) < Q.radius;
    if (ok && stereo_gate) {
        const float ur = rur[p];
        if (ur > 0 && fabsf(__fsub_rn(Q.ur, ur)) > Q.radius) ok = false;
    }
    const int dist = hamming256(qd, d0, d1);
    // searches that take the best candidate alone (no second best, no ratio test) never look past the first free entry,
    // and an entry beyond their acceptance threshold can only mean "no match": it need not be listed
    return {ok && dist <= max_dist, ((unsigned long long)dist << 32) | R.key};
}
// The candidate test of Fuse and SearchBySim3 (src/ORBmatcher.cc:893-950, :1045-1075, :1199-1219) for train key point j:
// |dx|,|dy| < r, kpLevel in [min_level, max_level], with chi2_gate the reprojection error against 5.99 (mono) / 7.8
// (stereo) scaled by mvInvLevelSigma2[level] and compared in double.  False = not a candidate; else *dist = Hamming distance.
__device__ __forceinline__ bool fuse_candidate(const orbhip_keypoint *__restrict__ keys, const uint8_t *__restrict__ desc,
                                               const float *__restrict__ u_right, int j, float x, float y, float r,
                                               float qur, int min_level, int max_level, bool chi2_gate,
                                               const SigmaTab &sig, const uint32_t (&qd)[8], int *dist)
{
    const orbhip_keypoint kp = keys[j];
    if (!(fabsf(__fsub_rn(kp.x, x)) < r && fabsf(__fsub_rn(kp.y, y)) < r)) return false;
    if (kp.octave < min_level || kp.octave > max_level) return false;   // kpLevel<pred-1 || kpLevel>pred
    if (chi2_gate) {
        const float ex = __fsub_rn(x, kp.x), ey = __fsub_rn(y, kp.y);
        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        const float kpr = u_right ? u_right[j] : -1.0f;
        const float is2 = sig.inv_sigma2[kp.octave & (ORBHIP_MAX_LEVELS - 1)];
        if (kpr >= 0) {
            const float er = __fsub_rn(qur, kpr);
            e2 = __fadd_rn(e2, __fmul_rn(er, er));
            if ((double)__fmul_rn(e2, is2) > 7.8) return false;
        } else if ((double)__fmul_rn(e2, is2) > 5.99) return false;
    }
    const uint4 *tp = reinterpret_cast<const uint4 *>(desc + (size_t)j * 32);
    *dist = hamming256(qd, tp[0], tp[1]);
    return true;
}

// 64-bit minimum over the wavefront (wave-uniform result): the same DPP butterfly + row broadcasts as wave_sum, both
// halves of the key travelling together
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#define ORBHIP_MIN64_STEP(ctrl, rmask)                                                                        \
    {                                                                                                         \
        const uint32_t lo_ = (uint32_t)v, hi_ = (uint32_t)(v >> 32);                                          \
        const uint32_t ol_ = (uint32_t)__builtin_amdgcn_update_dpp((int)lo_, (int)lo_, ctrl, rmask, 0xf, false); \
        const uint32_t oh_ = (uint32_t)__builtin_amdgcn_update_dpp((int)hi_, (int)hi_, ctrl, rmask, 0xf, false); \
        const unsigned long long o_ = ((unsigned long long)oh_ << 32) | ol_;                                  \
        v = o_ < v ? o_ : v;                                                                                  \
    }
    ORBHIP_MIN64_STEP(0xB1, 0xf)
    ORBHIP_MIN64_STEP(0x4E, 0xf)
    ORBHIP_MIN64_STEP(0x141, 0xf)
    ORBHIP_MIN64_STEP(0x140, 0xf)
    ORBHIP_MIN64_STEP(0x142, 0xa)
    ORBHIP_MIN64_STEP(0x143, 0xc)
#undef ORBHIP_MIN64_STEP
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), 63) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}

// 64-bit minimum over LPQ consecutive lanes (8, 16 = one DPP row, 64 = the wavefront), in all of them: quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, and row_mirror for the row
template <int LPQ> __device__ __forceinline__ unsigned long long group_min_u64(unsigned long long v)
{
    static_assert(LPQ == 8 || LPQ == 16 || LPQ == 64, "group sizes of k_fuse_batch and k_window_search");
    if constexpr (LPQ == 64) {
        return wave_min_u64(v);
    } else {
#define ORBHIP_GMIN_STEP(ctrl)                                                                                \
    {                                                                                                         \
        const uint32_t lo_ = (uint32_t)v, hi_ = (uint32_t)(v >> 32);                                          \
        const uint32_t ol_ = (uint32_t)__builtin_amdgcn_update_dpp((int)lo_, (int)lo_, ctrl, 0xf, 0xf, false); \
        const uint32_t oh_ = (uint32_t)__builtin_amdgcn_update_dpp((int)hi_, (int)hi_, ctrl, 0xf, 0xf, false); \
        const unsigned long long o_ = ((unsigned long long)oh_ << 32) | ol_;                                  \
        v = o_ < v ? o_ : v;                                                                                  \
    }
        ORBHIP_GMIN_STEP(0xB1)
        ORBHIP_GMIN_STEP(0x4E)
        ORBHIP_GMIN_STEP(0x141)
        if constexpr (LPQ == 16) ORBHIP_GMIN_STEP(0x140)
#undef ORBHIP_GMIN_STEP
        return v;
    }
}

// The smallest keys of a list whose entries are spread over the lanes, in ascending order, EXACTLY: every lane hands in
// its two smallest keys (a1 < a2, ~0 = none) and whether it holds more than those two.  Minimum after minimum is
// extracted; once a lane has given both of its keys and still holds others, a later minimum could be one of those, so
// the extraction stops there.  Keys are unique.  Returns the number of keys written to head[] (wave-uniform, <= kHeadMax);
// *complete = the list has no further key (the extraction ran dry, not into the stop condition or the limit).
constexpr int kHeadMax = 8;
__device__ __forceinline__ int wave_sorted_head(unsigned long long a1, unsigned long long a2, bool more,
                                                unsigned long long (&head)[kHeadMax], bool *complete)
{
    int given = 0, hl = 0;
    bool stop = false, dry = false;
#pragma unroll
    for (int k = 0; k < kHeadMax; ++k) {
        head[k] = ~0ull;
        if (stop || dry) continue;          // wave-uniform
        const unsigned long long c = given == 0 ? a1 : (given == 1 ? a2 : ~0ull);
        const unsigned long long g = wave_min_u64(c);
        if (g == ~0ull) { dry = true; continue; }
        head[k] = g;
        hl = k + 1;
        const bool mine = c == g;
        if (mine) ++given;
        stop = __any(mine && given == 2 && more) != 0;
    }
    // a lane that still holds an unextracted tracked key, or more keys than it tracks, means the list goes on
    const bool rest = (given == 0 && a1 != ~0ull) || (given <= 1 && a2 != ~0ull) || more;
    *complete = !__any(rest);
    return hl;
}

// ---- rotation consistency (ORBmatcher.cc rotHist + ComputeThreeMaxima), the one home of the rule -------------------
// The accepted matches are histogrammed by rot_bin(query angle, train angle), three_maxima picks the winning bins and
// every match outside them is dropped.  A match without a bin (rot_bin < 0, kept as 0xff where bins are bytes) takes no
// part: it is neither histogrammed nor dropped.  Used by the fused epilogues of k_resolve_par, k_resolve_init and
// k_bow_pairs and by rot_cull_body, the stand-alone cull behind k_rot_cull and k_cnmp_cull.
__device__ __forceinline__ int rot_bin(float a1, float a2)
{
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = __fsub_rn(a1, a2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    const float r = roundf(__fmul_rn(rot, factor));
    // keypoint angles are caller data: outside [0, 360) (or NaN) the reference trips its assert(bin>=0 && bin<HISTO_LENGTH);
    // here such a match simply takes no part in the rotation histogram (-1) instead of writing outside it.  Tested on the
    // float: the conversion of a NaN to int is not defined (the hardware's gives 0, which would be a bin)
    if (!(r >= 0.0f && r <= (float)HISTO_LENGTH)) return -1;
    return r == (float)HISTO_LENGTH ? 0 : (int)r;
}

__device__ __forceinline__ void three_maxima(const int *h, int &ind1, int &ind2, int &ind3)
{
    // ComputeThreeMaxima (src/ORBmatcher.cc:1601-1645) as selects on values: with the three indices passed by reference
    // through a chain of branches the compiler kept them in scratch memory (150 scratch accesses per call)
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    int hv[HISTO_LENGTH];   // all bins first (independent loads, one wait), then the scan on registers
#pragma unroll
    for (int i = 0; i < HISTO_LENGTH; ++i) hv[i] = h[i];
#pragma unroll
    for (int i = 0; i < HISTO_LENGTH; ++i) {
        const int s = hv[i];
        const bool g1 = s > max1, g2 = s > max2, g3 = s > max3;
        max3 = g2 ? max2 : (g3 ? s : max3);  i3 = g2 ? i2 : (g3 ? i : i3);
        max2 = g1 ? max1 : (g2 ? s : max2);  i2 = g1 ? i1 : (g2 ? i : i2);
        max1 = g1 ? s : max1;                i1 = g1 ? i : i1;
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) { i3 = -1; }
    ind1 = i1; ind2 = i2; ind3 = i3;
}

// hist[bin] += 1 for every lane of the wavefront with bin >= 0; all 64 lanes call it.  One atomic per distinct bin of the
// wavefront (most matches of a frame pair share a rotation bin).
__device__ __forceinline__ void wave_hist_add(int *hist, int bin)
{
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int lead = __builtin_amdgcn_readlane(bin, first);
        const unsigned long long same = __ballot(bin == lead);
        if ((threadIdx.x & 63) == first) atomicAdd(&hist[lead], __popcll(same));
        todo &= ~same;
    }
}

// Wavefront 0 ranks the finished histogram (a workgroup's wavefronts share one CU's issue slots) and publishes the three
// winning bins to ind[0..2] for everybody: the barrier is inside, the one that completes the histogram is the caller's.
__device__ __forceinline__ void rank_bins_once(const int *hist, int *ind)
{
    if (threadIdx.x < 64) {
        int i1, i2, i3;
        three_maxima(hist, i1, i2, i3);
        if (threadIdx.x == 0) { ind[0] = i1; ind[1] = i2; ind[2] = i3; }
    }
    __syncthreads();
}

// the cull predicate: bin b takes part (a bin, not -1 / 0xff) and is none of the three winners
__device__ __forceinline__ bool rot_culled(int b, int ind1, int ind2, int ind3)
{
    return (unsigned)b < (unsigned)HISTO_LENGTH && b != ind1 && b != ind2 && b != ind3;
}

// The stand-alone cull: one workgroup, one row of matches.  match[i] = train index of query i or -1; query i's angle is the
// float at qangle + i * qstride bytes (key arrays, query arrays and packed floats alike).  Culls in place; writes the
// number of surviving matches to *out_n when given.  check_ori == 0 only counts.
__device__ __forceinline__ void rot_cull_body(int *__restrict__ match, const int n, const void *__restrict__ qangle,
                                              const size_t qstride, const orbhip_keypoint *__restrict__ tkeys,
                                              const int check_ori, int *__restrict__ out_n)
{
    __shared__ int hist[HISTO_LENGTH], ind[3], kept;
    const int tid = threadIdx.x, T = blockDim.x;
    const auto bin_of = [&](int i, int j) {
        return rot_bin(*reinterpret_cast<const float *>(static_cast<const unsigned char *>(qangle) + i * qstride), tkeys[j].angle);
    };
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) kept = 0;
    __syncthreads();
    if (check_ori) {
        for (int i0 = 0; i0 < n; i0 += T) {
            const int i = i0 + tid, j = i < n ? match[i] : -1;
            wave_hist_add(hist, j >= 0 ? bin_of(i, j) : -1);
        }
        __syncthreads();
        rank_bins_once(hist, ind);
    }
    int cnt = 0;
    for (int i = tid; i < n; i += T) {
        const int j = match[i];
        if (j < 0) continue;
        if (check_ori && rot_culled(bin_of(i, j), ind[0], ind[1], ind[2])) match[i] = -1;
        else ++cnt;
    }
    if (!out_n) return;
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(&kept, cnt);
    __syncthreads();
    if (tid == 0) *out_n = kept;
}

// the body on a row given by host-known pointers (host SearchByBoW, host SearchForTriangulation)
__global__ __launch_bounds__(1024) void k_rot_cull(int *__restrict__ match, int n, const void *__restrict__ qangle, int qstride,
                                                   const orbhip_keypoint *__restrict__ tkeys, int check_ori,
                                                   int *__restrict__ out_n)
{
    rot_cull_body(match, n, qangle, (size_t)qstride, tkeys, check_ori, out_n);
}

// Visiting-order key of every train keypoint, (posX*48+posY) << 20 | index, or kNoCell when PosInGrid rejects it
// (k_best_in_window scans the frame with it).
__global__ void k_grid_order(DevFrame F, uint32_t *__restrict__ ord, Batch B)
{
    batch_frame(F, B, blockIdx.y);
    ord += (size_t)blockIdx.y * B.cap;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= F.n) return;
    const orbhip_keypoint kp = F.keys[j];
    const int cell = grid_cell(kp.x, kp.y, F.min_x, F.min_y, F.inv_w, F.inv_h);
    ord[j] = cell >= 0 ? (((uint32_t)cell << 20) | (uint32_t)j) : kNoCell;
}

// mGrid of the train frame (Frame::AssignFeaturesToGrid, Frame.cc:230-245) as CSR, one workgroup per frame: cell
// c = posX * 48 + posY owns the records rec[start[c] .. start[c+1]).  A record carries everything the window search
// needs of a keypoint -- (x, y, octave, index) and, in a parallel array, its descriptor -- so a query reads its
// candidates with addresses that depend on the cell table only (one memory round trip, not index -> keypoint ->
// descriptor).  Counting sort with LDS atomics; the order INSIDE a cell is arbitrary: every consumer orders candidates
// by the key (cell << 20 | index) = the visiting order of Frame::GetFeaturesInArea (cell-major ix outer / iy inner,
// insertion order inside a cell; Frame.cc:350-358).  Keypoints that PosInGrid rejects (Frame.cc:382-392) are in no
// cell and never candidates.
__device__ __forceinline__ void grid_build_body(DevFrame F, int *__restrict__ cell_start, GridRec *__restrict__ rec,
                                                uint4 *__restrict__ rdesc, float *__restrict__ rur, const Batch &B, const int pair)
{
    __shared__ int s_cnt[kGridCells];
    __shared__ int s_scan[8];
    const int tid = threadIdx.x;
    batch_frame(F, B, pair);
    const size_t rbase = (size_t)pair * B.cap;
    cell_start += (size_t)pair * (kGridCells + 1);
    rec += rbase; rdesc += rbase * 2; rur += rbase;
    for (int c = tid; c < kGridCells; c += 256) s_cnt[c] = 0;
    __syncthreads();
    const auto cell_of = [&](float x, float y) { return grid_cell(x, y, F.min_x, F.min_y, F.inv_w, F.inv_h); };
    const auto emit = [&](int j, float x, float y, int octave, int cell) {
        const int pos = atomicAdd(&s_cnt[cell], 1);
        GridRec r; r.x = x; r.y = y; r.octave = octave; r.key = ((uint32_t)cell << 20) | (uint32_t)j;
        rec[pos] = r;
        const uint4 *d = reinterpret_cast<const uint4 *>(F.desc + (size_t)j * 32);
        rdesc[2 * pos] = d[0]; rdesc[2 * pos + 1] = d[1];
        rur[pos] = F.u_right ? F.u_right[j] : -1.0f;
    };
    // up to kGridKeep keypoints per thread stay in registers between the count pass and the scatter pass (one load of the
    // 28-byte key, one PosInGrid); a larger frame reads its keys twice.  F.n is uniform: one scalar branch, no barrier inside
    constexpr int kGridKeep = 4;
    const bool keep = F.n <= 256 * kGridKeep;
    float kx[kGridKeep], ky[kGridKeep];
    int ko[kGridKeep], kc[kGridKeep];
    if (keep) {
#pragma unroll
        for (int k = 0; k < kGridKeep; ++k) {
            const int j = tid + 256 * k;
            kx[k] = ky[k] = 0.0f; ko[k] = 0; kc[k] = -1;
            if (j < F.n) {
                const orbhip_keypoint kp = F.keys[j];
                kx[k] = kp.x; ky[k] = kp.y; ko[k] = kp.octave; kc[k] = cell_of(kp.x, kp.y);
                if (kc[k] >= 0) atomicAdd(&s_cnt[kc[k]], 1);
            }
        }
    } else {
        for (int j = tid; j < F.n; j += 256) {
            const orbhip_keypoint kp = F.keys[j];
            const int cell = cell_of(kp.x, kp.y);
            if (cell >= 0) atomicAdd(&s_cnt[cell], 1);
        }
    }
    __syncthreads();
    // exclusive scan over the 3072 cells: 12 consecutive cells per thread
    constexpr int PER = kGridCells / 256;
    int local[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { local[k] = s_cnt[tid * PER + k]; sum += local[k]; }
    int incl = sum;
    const int lane = tid & 63, wave = tid >> 6;
    incl = wave_incl_scan_add(incl);
    if (lane == 63) s_scan[wave] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < wave; ++w) base += s_scan[w];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) { s_cnt[tid * PER + k] = base; cell_start[tid * PER + k] = base; base += local[k]; }
    if (tid == 255) cell_start[kGridCells] = base;
    __syncthreads();
    if (keep) {
#pragma unroll
        for (int k = 0; k < kGridKeep; ++k)
            if (kc[k] >= 0) emit(tid + 256 * k, kx[k], ky[k], ko[k], kc[k]);
    } else {
        for (int j = tid; j < F.n; j += 256) {
            const orbhip_keypoint kp = F.keys[j];
            const int cell = cell_of(kp.x, kp.y);
            if (cell >= 0) emit(j, kp.x, kp.y, kp.octave, cell);
        }
    }
}
__global__ __launch_bounds__(256) void k_grid_build(DevFrame F, int *__restrict__ cell_start, GridRec *__restrict__ rec,
                                                    uint4 *__restrict__ rdesc, float *__restrict__ rur, Batch B)
{
    grid_build_body(F, cell_start, rec, rdesc, rur, B, (int)blockIdx.x);
}

// L lanes per query (L = 16: one DPP row, four queries per wavefront; L = 64: the whole wavefront).  The columns of the
// query's window (Frame.cc:332-346) are dealt to the lanes of its group; the records of those columns are then flattened
// over the lanes (group prefix sum of the column populations + an LDS scatter of the record positions), so one pass tests
// L candidates per query: level window, |dx|,|dy| < r, stereo gate, Hamming distance.  Every primitive is scoped to the
// group -- scan, total, ballot prefix, minimum -- and the groups of a wavefront run in lockstep: loops go to the largest
// trip count of the wavefront under per-group predicates, a group without a query or with an empty window idles.
// Nothing is shared between wavefronts (stage / spos rows belong to one group), so there is no workgroup barrier.
// Output: dist << 32 | (cell << 20 | index) keys; with <= 64 candidates the list is rank-sorted (= (distance, reference
// visiting order)) into ccand[q*64 ..] and cnt[q] > 0 -- such a list lives in LDS only and never touches `cand` --
// otherwise it stays unsorted in cand[q*stride ..] with cnt[q] = -count.
constexpr int kCompact = 64;
template <int L> __device__ __forceinline__ int group_incl_scan_add(int v)
{
    static_assert(L == 16, "a group is one DPP row");
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    return v;
}
// total of the values v of a group, in every lane of the group
template <int L> __device__ __forceinline__ int group_total(int v)
{
    static_assert(L == 16, "a group is one DPP row");
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);   // row_mirror
    return v;
}
// the group's bits of a wavefront ballot, shifted down to bit 0
template <int L> __device__ __forceinline__ unsigned long long group_bits(unsigned long long bal)
{
    return (bal >> (threadIdx.x & 63 & ~(L - 1))) & ((1ull << L) - 1ull);
}
// wave_sorted_head per group.  Called by the whole wavefront (the groups step together; one that has stopped, run dry or
// has no long list hands in ~0 and ignores the minimum); every result is group-uniform.
template <int L>
__device__ __forceinline__ int group_sorted_head(unsigned long long a1, unsigned long long a2, bool more,
                                                 unsigned long long (&head)[kHeadMax], bool *complete)
{
    int given = 0, hl = 0;
    bool done = false;   // stopped or dry
#pragma unroll
    for (int k = 0; k < kHeadMax; ++k) {
        head[k] = ~0ull;
        if (!__any(!done)) continue;        // wave-uniform: every group has stopped or run dry
        const unsigned long long c = done ? ~0ull : (given == 0 ? a1 : (given == 1 ? a2 : ~0ull));
        const unsigned long long g = group_min_u64<L>(c);
        const bool got = !done && g != ~0ull;
        if (got) { head[k] = g; hl = k + 1; }
        const bool mine = got && c == g;
        if (mine) ++given;
        const bool stop = group_bits<L>(__ballot(mine && given == 2 && more)) != 0;
        done = done || !got || stop;
    }
    // a lane that still holds an unextracted tracked key, or more keys than it tracks, means the list goes on
    const bool rest = (given == 0 && a1 != ~0ull) || (given <= 1 && a2 != ~0ull) || more;
    *complete = group_bits<L>(__ballot(rest)) == 0;
    return hl;
}
// Rank sort of a group's staged keys (total <= 64, distinct): a lane owns the M keys gl, gl + L, ... and counts for each
// the keys below it -- key j comes to the group as a same-address LDS read -- then stores it at its rank.  Cheaper than a
// bitonic network (12 instructions per stage, 10 .. 21 stages) at every length.  `total` is group-uniform; 0 = no list.
template <int L, int M>
__device__ __forceinline__ void group_rank_store(const unsigned long long *__restrict__ st, const int total, const int gl,
                                                 unsigned long long *__restrict__ row)
{
    unsigned long long v[M];
    int rank[M];
#pragma unroll
    for (int m = 0; m < M; ++m) { v[m] = gl + m * L < total ? st[gl + m * L] : ~0ull; rank[m] = 0; }
#pragma unroll 4
    for (int j = 0; j < total; ++j) {
        const unsigned long long kj = st[j];
#pragma unroll
        for (int m = 0; m < M; ++m) rank[m] += kj < v[m] ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < M; ++m) if (gl + m * L < total) row[rank[m]] = v[m];
}
template <int L>
__global__ __launch_bounds__(256) void k_window_search(DevFrame F, const int *__restrict__ cell_start,
                                                       const GridRec *__restrict__ rec, const uint4 *__restrict__ rdesc,
                                                       const float *__restrict__ rur,
                                                       const orbhip_query *__restrict__ q,
                                                       const uint8_t *__restrict__ qdesc,
                                                       unsigned long long *__restrict__ cand,
                                                       unsigned long long *__restrict__ ccand,
                                                       int *__restrict__ cnt, int stride, int use_ur, Batch B,
                                                       const uint8_t *__restrict__ taken, int max_dist)
{
    static_assert(L == 16, "a group is one DPP row; the wavefront form is the specialisation below");
    constexpr int QW = 256 / L;                    // queries per workgroup
    __shared__ unsigned long long stage[QW][kCompact];
    __shared__ int spos[QW][L];
    const int gl = threadIdx.x & (L - 1), qw = threadIdx.x / L;   // lane in the group, query in the workgroup
    const int pair = blockIdx.y;
    const bool has_ur = F.u_right != nullptr;
    batch_frame(F, B, pair);
    const size_t rbase = (size_t)pair * B.cap;
    cell_start += (size_t)pair * (kGridCells + 1);
    rec += rbase; rdesc += rbase * 2; rur += rbase;
    q += (size_t)pair * B.qcap;
    qdesc += (size_t)(B.qd0 + pair * B.qds) * B.qcap * 32;
    cand += (size_t)pair * B.qcap * stride;
    ccand += (size_t)pair * B.qcap * kCompact;
    cnt += (size_t)pair * B.qcap;
    if (taken) taken += (size_t)pair * B.cap;
    const int nq = B.nq_dev ? min(B.nq_dev[pair], B.qcap) : B.qcap;
    const int qi = blockIdx.x * QW + qw;
    const bool inq = qi < nq;
    orbhip_query Q = {};
    if (inq) Q = q[qi];
    const CellWindow W = cell_window(Q.u, Q.v, Q.radius, F.min_x, F.min_y, F.inv_w, F.inv_h);
    // a group without a valid query or with an empty window idles: no column, no record, no list
    const bool live = inq && Q.valid && !W.empty();
    if (!__any(live)) {   // nothing to search in this wavefront
        if (inq && gl == 0) cnt[qi] = 0;
        return;
    }
    uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const uint32_t *qp = reinterpret_cast<const uint32_t *>(qdesc + (size_t)qi * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) qd[i] = qp[i];
    }
    unsigned long long *out = cand + (size_t)(inq ? qi : 0) * stride;
    const int ncy = W.y1 - W.y0 + 1;
    int total = 0;
    unsigned long long b1 = ~0ull, b2 = ~0ull;   // this lane's two smallest keys among candidates not taken on entry
    int nb = 0;                                  // ... out of how many
    // a column of the window is a contiguous run of cells (cell = ix * 48 + iy), so its records are one contiguous CSR
    // range: lane = window column, range = [start[ix*48 + y0], start[ix*48 + y1 + 1]).  A window wider than L columns
    // takes several trips; total, b1, b2 and nb carry over.
    const int ncol = live ? W.x1 - W.x0 + 1 : 0;
    for (int c0 = 0; __any(c0 < ncol); c0 += L) {
        const int c = c0 + gl;
        int start = 0, ncand = 0;
        if (c < ncol) {
            const int cell0 = (W.x0 + c) * GRID_ROWS + W.y0;
            start = cell_start[cell0];
            ncand = cell_start[cell0 + ncy] - start;
        }
        // exclusive prefix of the column populations over the group
        const int incl = group_incl_scan_add<L>(ncand);
        const int excl = incl - ncand, nrec = group_total<L>(ncand);
        for (int r0 = 0; __any(r0 < nrec); r0 += L) {
            // scatter: flat record t of this chunk comes from CSR position spos[t - r0]
            wave_lds_handoff();   // the previous chunk's reads of spos are done; its staged keys may be copied out below
            for (int k = max(0, r0 - excl); k < ncand && excl + k < r0 + L; ++k) spos[qw][excl + k - r0] = start + k;
            wave_lds_handoff();
            WindowHit H = {false, 0};
            if (r0 + gl < nrec) H = window_candidate(rec, rdesc, rur, spos[qw][gl], Q, qd, use_ur && has_ur, max_dist);
            const bool ok = H.ok;
            const unsigned long long key = H.key;
            const unsigned long long bal = group_bits<L>(__ballot(ok));
            const int ntot = total + __popcll(bal);
            // a list stays in LDS while it fits the compact row; the chunk that takes it past 64 entries moves the staged
            // keys to `cand`, and from then on keys go there directly
            if (ntot > kCompact && total <= kCompact)
                for (int i = gl; i < total; i += L) out[i] = stage[qw][i];
            if (ok) {
                const int pos = total + __popcll(bal & ((1ull << gl) - 1ull));
                if (ntot <= kCompact) stage[qw][pos] = key; else out[pos] = key;
                if (!(taken && taken[key & 0xfffffu])) {
                    if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
                    ++nb;
                }
            }
            total = ntot;
        }
    }
    wave_lds_handoff();                                   // the staged keys are read across the group
    // short lists: sorted into the compact row
    const int ns = total <= kCompact ? total : 0;
    unsigned long long *row = ccand + (size_t)(inq ? qi : 0) * kCompact;
    if (__any(ns > L)) group_rank_store<L, kCompact / L>(stage[qw], ns, gl, row);
    else group_rank_store<L, 1>(stage[qw], ns, gl, row);
    // more than 64 candidates: the list stays unsorted in `cand`; the first (up to kHeadMax) keys of its sorted order
    // among the candidates not taken on entry go to the head of the compact row -- {keys[8], count | complete << 8} --
    // so the resolve walks a sorted head like it does for short lists and only scans the list when the head runs out
    const bool lng = total > kCompact;
    if (__any(lng)) {
        unsigned long long head[kHeadMax];
        bool complete;
        const int hl = group_sorted_head<L>(lng ? b1 : ~0ull, lng ? b2 : ~0ull, lng && nb > 2, head, &complete);
        if (lng && gl < kHeadMax) {
            unsigned long long v = head[0];
#pragma unroll
            for (int k = 1; k < kHeadMax; ++k) if (gl == k) v = head[k];
            row[gl] = v;
        }
        if (lng && gl == 0) row[kHeadMax] = (unsigned long long)hl | (complete ? 0x100ull : 0ull);
    }
    if (inq && gl == 0) cnt[qi] = lng ? -total : total;
}

// L = 64, one wavefront per query: the form SearchForInitialization and wide tracking searches run.  The cells of the
// query's window are dealt to the lanes, one pass tests 64 candidates; every candidate goes to `cand`, the first 64 also to
// the LDS stage that is rank-sorted through v_readlane when the list ends there.
template <>
__global__ __launch_bounds__(256) void k_window_search<64>(DevFrame F, const int *__restrict__ cell_start,
                                                       const GridRec *__restrict__ rec, const uint4 *__restrict__ rdesc,
                                                       const float *__restrict__ rur,
                                                       const orbhip_query *__restrict__ q,
                                                       const uint8_t *__restrict__ qdesc,
                                                       unsigned long long *__restrict__ cand,
                                                       unsigned long long *__restrict__ ccand,
                                                       int *__restrict__ cnt, int stride, int use_ur, Batch B,
                                                       const uint8_t *__restrict__ taken, int max_dist)
{
    __shared__ unsigned long long stage[4][64];
    __shared__ int spos[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int pair = blockIdx.y;
    const bool has_ur = F.u_right != nullptr;
    batch_frame(F, B, pair);
    const size_t rbase = (size_t)pair * B.cap;
    cell_start += (size_t)pair * (kGridCells + 1);
    rec += rbase; rdesc += rbase * 2; rur += rbase;
    q += (size_t)pair * B.qcap;
    qdesc += (size_t)(B.qd0 + pair * B.qds) * B.qcap * 32;
    cand += (size_t)pair * B.qcap * stride;
    ccand += (size_t)pair * B.qcap * kCompact;
    cnt += (size_t)pair * B.qcap;
    if (taken) taken += (size_t)pair * B.cap;
    const int nq = B.nq_dev ? min(B.nq_dev[pair], B.qcap) : B.qcap;
    const int qi = blockIdx.x * 4 + wv;
    if (qi >= nq) return;
    const orbhip_query Q = q[qi];
    if (!Q.valid) { if (lane == 0) cnt[qi] = 0; return; }
    const CellWindow W = cell_window(Q.u, Q.v, Q.radius, F.min_x, F.min_y, F.inv_w, F.inv_h);
    if (W.empty()) {
        if (lane == 0) cnt[qi] = 0;
        return;
    }
    uint32_t qd[8];
    const uint32_t *qp = reinterpret_cast<const uint32_t *>(qdesc + (size_t)qi * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) qd[i] = qp[i];
    unsigned long long *out = cand + (size_t)qi * stride;
    const int ncy = W.y1 - W.y0 + 1;
    int total = 0;
    unsigned long long b1 = ~0ull, b2 = ~0ull;   // this lane's two smallest keys among candidates not taken on entry
    int nb = 0;                                  // ... out of how many
    // a column of the window is a contiguous run of cells (cell = ix * 48 + iy), so its records are one contiguous CSR
    // range: lane = window column, range = [start[ix*48 + y0], start[ix*48 + y1 + 1])
    const int ncol = W.x1 - W.x0 + 1;
    for (int c0 = 0; c0 < ncol; c0 += 64) {
        const int c = c0 + lane;
        int start = 0, ncand = 0;
        if (c < ncol) {
            const int cell0 = (W.x0 + c) * GRID_ROWS + W.y0;
            start = cell_start[cell0];
            ncand = cell_start[cell0 + ncy] - start;
        }
        // exclusive prefix of the column populations over the wave
        int incl = ncand;
        incl = wave_incl_scan_add(incl);
        const int nrec = __builtin_amdgcn_readlane(incl, 63);
        const int excl = incl - ncand;
        for (int r0 = 0; r0 < nrec; r0 += 64) {
            // scatter: flat record t of this chunk comes from CSR position spos[t - r0]
            wave_lds_handoff();                           // the previous chunk's reads of spos are done
            for (int k = max(0, r0 - excl); k < ncand && excl + k < r0 + 64; ++k) spos[wv][excl + k - r0] = start + k;
            wave_lds_handoff();
            WindowHit H = {false, 0};
            if (r0 + lane < nrec) H = window_candidate(rec, rdesc, rur, spos[wv][lane], Q, qd, use_ur && has_ur, max_dist);
            const bool ok = H.ok;
            const unsigned long long key = H.key;
            const unsigned long long bal = __ballot(ok);
            if (ok) {
                const int pos = total + __popcll(bal & ((1ull << lane) - 1ull));
                out[pos] = key;
                if (pos < 64) stage[wv][pos] = key;
                if (!(taken && taken[key & 0xfffffu])) {
                    if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
                    ++nb;
                }
            }
            total += __popcll(bal);
        }
    }
    if (total > 0 && total <= 64) {
        // rank sort of up to 64 distinct keys: lane i counts the keys below its own -- key j comes to all lanes through
        // v_readlane (j is wave-uniform), so a key costs two readlanes, one 64-bit compare and one add -- and stores its
        // key at its rank; cheaper than a bitonic network (12 instructions per stage, 10 .. 21 stages) at every length
        wave_lds_handoff();                               // the staged keys were written by other lanes
        const unsigned long long v = lane < total ? stage[wv][lane] : ~0ull;
        const uint32_t vlo = (uint32_t)v, vhi = (uint32_t)(v >> 32);
        const int tu = __builtin_amdgcn_readfirstlane(total);
        int rank = 0;
        for (int j = 0; j < tu; ++j) {
            const unsigned long long kj = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)vhi, j) << 32) |
                                          (uint32_t)__builtin_amdgcn_readlane((int)vlo, j);
            rank += kj < v ? 1 : 0;
        }
        if (lane < total) ccand[(size_t)qi * kCompact + rank] = v;
        if (lane == 0) cnt[qi] = total;
    } else {
        // more than 64 candidates: the list stays unsorted in `cand`; the first (up to kHeadMax) keys of its sorted order
        // among the candidates not taken on entry go to the head of the compact row -- {keys[8], count | complete << 8} --
        // so the resolve walks a sorted head like it does for short lists and only scans the list when the head runs out
        if (total > 64) {
            unsigned long long head[kHeadMax];
            bool complete;
            const int hl = wave_sorted_head(b1, b2, nb > 2, head, &complete);
            if (lane < kHeadMax) {
                unsigned long long v = head[0];
#pragma unroll
                for (int k = 1; k < kHeadMax; ++k) if (lane == k) v = head[k];
                ccand[(size_t)qi * kCompact + lane] = v;
            }
            if (lane == 0) ccand[(size_t)qi * kCompact + kHeadMax] = (unsigned long long)hl | (complete ? 0x100ull : 0ull);
        }
        if (lane == 0) cnt[qi] = -total;
    }
}

// ---- vocabulary-node guided searches (SearchByBoW :159-288 / :522-655, SearchForTriangulation :657-823) -------
// Both visit the key frame's features in FeatureVector order (node id, then feature index) and only compare
// features filed under the same vocabulary node, in ascending index.
//
// SearchByBoW: matches of one node never interact with another node (a feature sits in exactly one node), so one
// wavefront owns one common node and replays its queries in order; lanes hold the node's candidates (the first 64
// in registers), the "already matched" flags live in slot space and each slot is only ever touched by the lane
// that owns it.  Best / second-best = two wave minima of (distance << 32 | slot).
struct NodeGroup { int q_begin, q_end, t_begin, t_end; };
__global__ __launch_bounds__(256) void k_bow_groups(const NodeGroup *__restrict__ groups, int ngroups,
                                                    const uint8_t *__restrict__ qdesc, const uint32_t *__restrict__ t_order,
                                                    const uint8_t *__restrict__ tdesc, uint8_t *__restrict__ matched,
                                                    int max_dist, float nnratio, int *__restrict__ match_out)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const NodeGroup G = groups[g];
    const int tc = G.t_end - G.t_begin;
    // first chunk of candidates in registers
    uint32_t td0[8];
    const bool have0 = lane < tc;
    {
        const uint32_t *tp = reinterpret_cast<const uint32_t *>(tdesc + (size_t)(have0 ? t_order[G.t_begin + lane] : 0) * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) td0[i] = have0 ? tp[i] : 0u;
    }
    bool used0 = have0 ? matched[G.t_begin + lane] != 0 : true;
    uint32_t qnext[8];
    {
        const uint32_t *qp = reinterpret_cast<const uint32_t *>(qdesc + (size_t)G.q_begin * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) qnext[i] = qp[i];
    }
    for (int qi = G.q_begin; qi < G.q_end; ++qi) {
        uint32_t qd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) qd[i] = qnext[i];
        if (qi + 1 < G.q_end) {   // the next query's descriptor travels while this one is resolved
            const uint32_t *qp = reinterpret_cast<const uint32_t *>(qdesc + (size_t)(qi + 1) * 32);
#pragma unroll
            for (int i = 0; i < 8; ++i) qnext[i] = qp[i];
        }
        unsigned long long k1 = ~0ull, k2 = ~0ull;
        if (!used0) k1 = ((unsigned long long)hamming256(qd, td0) << 32) | (unsigned)(G.t_begin + lane);
        for (int c = G.t_begin + 64 + lane; c < G.t_end; c += 64) {
            if (matched[c]) continue;
            const uint32_t *tp = reinterpret_cast<const uint32_t *>(tdesc + (size_t)t_order[c] * 32);
            uint32_t td[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) td[i] = tp[i];
            const unsigned long long k = ((unsigned long long)hamming256(qd, td) << 32) | (unsigned)c;
            if (k < k1) { k2 = k1; k1 = k; } else if (k < k2) k2 = k;
        }
        const unsigned long long m1 = wave_min_u64(k1);
        int res = -1;
        if (m1 != ~0ull) {
            const unsigned long long m2 = wave_min_u64(k1 == m1 ? k2 : k1);
            const int bestDist1 = (int)(m1 >> 32), bestDist2 = m2 == ~0ull ? 256 : (int)(m2 >> 32);
            if (bestDist1 <= max_dist && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {   // :262-264 / :598-600
                const int slot = (int)(uint32_t)m1;
                if (((slot - G.t_begin) & 63) == lane) {
                    matched[slot] = 1;
                    if (slot - G.t_begin < 64) used0 = true;
                }
                res = (int)t_order[slot];
            }
        }
        if (lane == 0) match_out[qi] = res;
    }
}

// Device-resident, batched SearchByBoW: one 1024-thread workgroup per (key frame, frame) pair does everything the
// host path splits between std::sort, k_bow_groups and k_rot_cull: both sides' (node << 32 | index) keys are sorted
// in LDS (= FeatureVector order), group heads are found on the sorted query keys, the node's candidate range by
// binary search in the sorted train keys, then the 16 wavefronts take the common nodes round-robin and replay each
// node's queries in order exactly like k_bow_groups; rotation histogram, cull and count finish in the same launch.
constexpr int kBowPairMax = 4096;
constexpr int kBowStage = 64;       // queries of a node whose descriptors a wavefront fetches in one go
struct BowPairShared {
    unsigned long long qkey[kBowPairMax], tkey[kBowPairMax];
    int mout[kBowPairMax];
    unsigned short ghead[kBowPairMax];
    unsigned char matched[kBowPairMax], bin[kBowPairMax];
    int hist[HISTO_LENGTH];
    int nq, nt, ngroups, nmatch, next_group;
    uint32_t qstage[16][kBowStage * 8];   // per wavefront: the descriptors of up to kBowStage queries of the node it replays
    unsigned short gt0[kBowPairMax], gt1[kBowPairMax], gq1[kBowPairMax];   // per group: train range, end of the query range
};
struct BowSide {   // one side of the pairs, in the extractor / vocabulary output layout
    const orbhip_keypoint *kps;
    const uint8_t *desc;
    const int *n;
    const uint32_t *node;
    const uint8_t *flag;   // query side: valid1 (null = all); train side: blocked2 (null = none)
    int f0, fs;            // frame index of pair p = f0 + p * fs
};

__device__ __forceinline__ int lower_bound_u64(const unsigned long long *a, int n, unsigned long long v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(1024) void k_bow_pairs(BowSide Q, BowSide T, int cap, int max_dist, float nnratio,
                                                    int check_ori, int *__restrict__ matches12, int *__restrict__ nmatches)
{
    extern __shared__ unsigned char bow_pair_lds[];
    BowPairShared &S = *reinterpret_cast<BowPairShared *>(bow_pair_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = 1024;
    const int pair = blockIdx.x, fq = Q.f0 + pair * Q.fs, ft = T.f0 + pair * T.fs;
    const int n1 = min(Q.n[fq], cap), n2 = min(T.n[ft], cap);
    const orbhip_keypoint *qk = Q.kps + (size_t)fq * cap, *tk = T.kps + (size_t)ft * cap;
    const uint8_t *qd = Q.desc + (size_t)fq * cap * 32, *td = T.desc + (size_t)ft * cap * 32;
    const uint32_t *qn = Q.node + (size_t)fq * cap, *tn = T.node + (size_t)ft * cap;
    const uint8_t *valid1 = Q.flag ? Q.flag + (size_t)fq * cap : nullptr;
    const uint8_t *blocked2 = T.flag ? T.flag + (size_t)ft * cap : nullptr;
    matches12 += (size_t)pair * cap;
    int P = 1024;
    while (P < max(n1, n2)) P <<= 1;
    for (int i = tid; i < P; i += NT) {
        const bool okq = i < n1 && qn[i] != 0xffffffffu && (!valid1 || valid1[i]);
        S.qkey[i] = okq ? (((unsigned long long)qn[i] << 32) | (unsigned)i) : ~0ull;
        const bool okt = i < n2 && tn[i] != 0xffffffffu;
        S.tkey[i] = okt ? (((unsigned long long)tn[i] << 32) | (unsigned)i) : ~0ull;
        S.mout[i] = -1;
        S.bin[i] = 0xff;
    }
    for (int i = tid; i < cap; i += NT) matches12[i] = -1;
    if (tid < HISTO_LENGTH) S.hist[tid] = 0;
    if (tid == 0) { S.nq = 0; S.nt = 0; S.ngroups = 0; S.nmatch = 0; S.next_group = 0; }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const unsigned long long a = S.qkey[i], b = S.qkey[l];
                    if ((a > b) == up) { S.qkey[i] = b; S.qkey[l] = a; }
                    const unsigned long long c = S.tkey[i], d = S.tkey[l];
                    if ((c > d) == up) { S.tkey[i] = d; S.tkey[l] = c; }
                }
            }
            // A thread's elements are tid, tid + 1024, ...: a wavefront owns aligned blocks of 64 elements.  While the
            // partner distance of this step and of the next one is below 64, every element a wavefront touches belongs to
            // it: a wave-local hand-off (wave_lds_handoff) replaces the workgroup barrier (41 of the 55 steps of P = 1024).
            const int jn = j > 1 ? (j >> 1) : k;            // partner distance of the next step
            if (j >= 64 || jn >= 64) __syncthreads();
            else wave_lds_handoff();
        }
    for (int i = tid; i < P; i += NT) {   // sizes of the valid prefixes; group heads of the query side
        if (S.qkey[i] != ~0ull) {
            if (i + 1 == P || S.qkey[i + 1] == ~0ull) S.nq = i + 1;
            if (i == 0 || (uint32_t)(S.qkey[i - 1] >> 32) != (uint32_t)(S.qkey[i] >> 32))
                S.ghead[atomicAdd(&S.ngroups, 1)] = (unsigned short)i;
        }
        if (S.tkey[i] != ~0ull) {
            if (i + 1 == P || S.tkey[i + 1] == ~0ull) S.nt = i + 1;
            S.matched[i] = (unsigned char)(blocked2 ? blocked2[(uint32_t)S.tkey[i]] != 0 : 0);
        }
    }
    __syncthreads();
    const int nq = S.nq, nt = S.nt, ng = S.ngroups;
    // ranges of every group by one thread each (three binary searches that the wavefront replaying the group would
    // otherwise run one after the other, 30 dependent LDS reads per group on the serial path)
    for (int g = tid; g < ng; g += NT) {
        const unsigned long long nodekey = S.qkey[S.ghead[g]] & 0xffffffff00000000ull;
        S.gt0[g] = (unsigned short)lower_bound_u64(S.tkey, nt, nodekey);
        S.gt1[g] = (unsigned short)lower_bound_u64(S.tkey, nt, nodekey + (1ull << 32));
        S.gq1[g] = (unsigned short)lower_bound_u64(S.qkey, nq, nodekey + (1ull << 32));
    }
    __syncthreads();
    // the wavefronts take the groups from a counter, not round-robin: groups differ in length
    for (;;) {
        int g = 0;
        if (lane == 0) g = atomicAdd(&S.next_group, 1);
        g = __builtin_amdgcn_readfirstlane(g);
        if (g >= ng) break;
        const int q_begin = S.ghead[g];
        const int t_begin = S.gt0[g], t_end = S.gt1[g];
        if (t_end <= t_begin) continue;   // node absent from the frame
        const int q_end = S.gq1[g];
        const int tc = t_end - t_begin;
        uint32_t td0[8];
        const bool have0 = lane < tc;
        {
            const uint32_t *tp = reinterpret_cast<const uint32_t *>(td + (size_t)(have0 ? (uint32_t)S.tkey[t_begin + lane] : 0) * 32);
#pragma unroll
            for (int i = 0; i < 8; ++i) td0[i] = have0 ? tp[i] : 0u;
        }
        bool used0 = have0 ? S.matched[t_begin + lane] != 0 : true;
        uint32_t *qs = S.qstage[wave];
        for (int qi = q_begin; qi < q_end; ++qi) {
            // The queries of a node are replayed one after the other (each may take a slot from the next), but their
            // descriptors do not depend on that: the wavefront fetches them kBowStage at a time -- lanes = dwords, a few
            // load instructions, ONE memory round trip -- into its LDS stage instead of waiting for a 32-byte load per query.
            const int qo = (qi - q_begin) & (kBowStage - 1);
            if (qo == 0) {
                const int nst = min(kBowStage, q_end - qi);
                wave_lds_handoff();                       // the previous chunk's reads come before the refill
                for (int e = lane; e < nst * 8; e += 64)
                    qs[e] = reinterpret_cast<const uint32_t *>(qd + (size_t)(uint32_t)S.qkey[qi + (e >> 3)] * 32)[e & 7];
                wave_lds_handoff();
            }
            uint32_t qdw[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) qdw[i] = qs[qo * 8 + i];
            // key = distance << 12 | slot (distances <= 256, slots < kBowPairMax = 4096): a wave minimum is six v_min on the
            // DPP path instead of six 64-bit compare-select steps, twice per query
            constexpr int kNone = 0x7fffffff;
            int k1 = kNone, k2 = kNone;
            if (!used0) k1 = (hamming256(qdw, td0) << 12) | (t_begin + lane);
            for (int c = t_begin + 64 + lane; c < t_end; c += 64) {
                if (S.matched[c]) continue;
                const uint32_t *tp = reinterpret_cast<const uint32_t *>(td + (size_t)(uint32_t)S.tkey[c] * 32);
                uint32_t t8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) t8[i] = tp[i];
                const int k = (hamming256(qdw, t8) << 12) | c;
                if (k < k1) { k2 = k1; k1 = k; } else if (k < k2) k2 = k;
            }
            const int m1 = wave_min(k1);
            if (m1 == kNone) continue;
            const int m2 = wave_min(k1 == m1 ? k2 : k1);
            const int bestDist1 = m1 >> 12, bestDist2 = m2 == kNone ? 256 : m2 >> 12;
            if (bestDist1 <= max_dist && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {
                const int slot = m1 & 4095;
                if (((slot - t_begin) & 63) == lane) {
                    S.matched[slot] = 1;
                    if (slot - t_begin < 64) used0 = true;
                }
                if (lane == 0) S.mout[qi] = (int)(uint32_t)S.tkey[slot];
            }
        }
    }
    __syncthreads();
    // rotation bins of the accepted matches, all at once: the two angle loads per match used to sit in the replay loop, one
    // dependent memory round trip per accepted query on a single lane
    // per-thread atomics and a ranking by every thread: wave_hist_add / rank_bins_once are not measured on the bow leg yet
    if (check_ori) {
        for (int p = tid; p < nq; p += NT) {
            const int idx2 = S.mout[p];
            if (idx2 < 0) continue;
            const int b = rot_bin(qk[(uint32_t)S.qkey[p]].angle, tk[idx2].angle);
            if (b >= 0) { atomicAdd(&S.hist[b], 1); S.bin[p] = (unsigned char)b; }   // stays 0xff otherwise: takes no part
        }
        __syncthreads();
    }
    int ind1 = -1, ind2 = -1, ind3 = -1;
    if (check_ori) three_maxima(S.hist, ind1, ind2, ind3);
    int cnt = 0;
    for (int p = tid; p < nq; p += NT) {
        const int mval = S.mout[p];
        if (mval < 0) continue;
        if (check_ori && rot_culled(S.bin[p], ind1, ind2, ind3)) continue;
        matches12[(uint32_t)S.qkey[p]] = mval;
        ++cnt;
    }
    if (cnt) atomicAdd(&S.nmatch, cnt);
    __syncthreads();
    if (tid == 0) nmatches[pair] = S.nmatch;
}

// SearchForTriangulation: one wavefront per query; the epipole and epipolar-line gates are applied here and only the
// winner (smallest distance, LAST index on ties, ":735 dist>bestDist") is kept.  The reference never sets
// vbMatched2, so queries are independent: the winner is the match, and only the rotation cull (k_rot_cull) follows.
struct TriParams {
    float f12[9];
    float ex, ey;
    float sigma2[ORBHIP_MAX_LEVELS], sf[ORBHIP_MAX_LEVELS];
};

// The candidate scan of one query by one wavefront, shared by k_tri_search and k_cnmp_search: lanes over the train
// keypoints of the query's node; a candidate is left out when tmask[j] != 0 equals mask_skip (tmask nullable) or, with
// only_stereo, when it has no right coordinate (:725-729).  Returns the wave-uniform train index of the winner, -1 = none.
__device__ __forceinline__ int tri_scan(const int lane, const int n, const orbhip_keypoint *__restrict__ keys,
                                        const uint8_t *__restrict__ desc, const float *__restrict__ u_right,
                                        const uint32_t *__restrict__ tnode, const uint8_t *__restrict__ tmask,
                                        const bool mask_skip, const bool only_stereo, const uint32_t qnode,
                                        const uint32_t (&qd)[8], const float qu, const float qv, const bool stereo1,
                                        const float (&f12)[9], const float ex, const float ey,
                                        const float *__restrict__ sigma2, const float *__restrict__ sf)
{
    // epipolar line of the query in image 2, ORBmatcher.cc:143-145
    const float la = __fadd_rn(__fadd_rn(__fmul_rn(qu, f12[0]), __fmul_rn(qv, f12[3])), f12[6]);
    const float lb = __fadd_rn(__fadd_rn(__fmul_rn(qu, f12[1]), __fmul_rn(qv, f12[4])), f12[7]);
    const float lc = __fadd_rn(__fadd_rn(__fmul_rn(qu, f12[2]), __fmul_rn(qv, f12[5])), f12[8]);
    const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
    unsigned long long best = ~0ull;
    for (int j = lane; j < n; j += 64) {
        if (tnode[j] != qnode || (tmask && (tmask[j] != 0) == mask_skip)) continue;
        // the right coordinate is read before the descriptor only where it filters (:725-729); k_tri_search, which never
        // filters on it, reads it after the distance test as it always did
        bool stereo2 = false;
        if (only_stereo) {
            stereo2 = u_right && u_right[j] >= 0;
            if (!stereo2) continue;
        }
        const uint32_t *tp = reinterpret_cast<const uint32_t *>(desc + (size_t)j * 32);
        uint32_t td[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) td[i] = tp[i];
        const int dist = hamming256(qd, td);
        if (dist > TH_LOW) continue;
        if (!only_stereo) stereo2 = u_right && u_right[j] >= 0;
        const orbhip_keypoint kp = keys[j];
        if (!stereo1 && !stereo2) {   // :741-747
            const float dx = __fsub_rn(ex, kp.x), dy = __fsub_rn(ey, kp.y);
            if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.f, sf[kp.octave])) continue;
        }
        // CheckDistEpipolarLine :147-156
        const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, kp.x), __fmul_rn(lb, kp.y)), lc);
        if (den == 0) continue;
        const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
        if (!((double)dsqr < 3.84 * (double)sigma2[kp.octave])) continue;
        const unsigned long long k = ((unsigned long long)dist << 32) | (uint32_t)(0xfffff - j);   // last index wins a tie
        best = k < best ? k : best;
    }
    best = wave_min_u64(best);
    return best == ~0ull ? -1 : 0xfffff - (int)(best & 0xfffffu);
}

__global__ __launch_bounds__(256) void k_tri_search(DevFrame F, const uint32_t *__restrict__ tnode,
                                                    const uint8_t *__restrict__ tvalid,
                                                    const orbhip_query *__restrict__ q,
                                                    const uint8_t *__restrict__ qdesc, int nq, int *__restrict__ out,
                                                    TriParams P)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int qi = blockIdx.x * 4 + wv;
    if (qi >= nq) return;
    const orbhip_query Q = q[qi];
    uint32_t qd[8];
    const uint32_t *qp = reinterpret_cast<const uint32_t *>(qdesc + (size_t)qi * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) qd[i] = qp[i];
    const int best = tri_scan(lane, F.n, F.keys, F.desc, F.u_right, tnode, tvalid, false, false, (uint32_t)Q.level_aux, qd,
                              Q.u, Q.v, Q.ur >= 0, P.f12, P.ex, P.ey, P.sigma2, P.sf);
    if (lane == 0) out[qi] = best;
}

// ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452) up to the map graph --------------------------------
// For the current key frame (row `cur` of the extractor-layout arrays) and K neighbour rows kf_index[k]:
//   k_cnmp_rows         one thread per neighbour: camera centres, the baseline gate (:244-261), ComputeF12 (:536-553) and
//                       the epipole (src/ORBmatcher.cc:664-670) into a [K] table; zeroes nmatches[k]
//   k_cnmp_search       one wavefront per (current keypoint, neighbour): SearchForTriangulation straight from the frame
//                       rows (node equality, has_point / only_stereo filters), gates as k_tri_search (shared tri_scan)
//   k_cnmp_cull         check_ori only, one workgroup per neighbour: rot_cull_body on the neighbour's row of matches, as
//                       k_rot_cull runs it for the host SearchForTriangulation
//   k_cnmp_triangulate  one lane per (neighbour, current keypoint): :286-431, the 4x4 problem in registers
// Arithmetic: DESIGN.md section 3 ("Creating new map points").
struct CnmpRow { float f12[9]; float ex, ey; int skip; };
struct CnmpLevels { float sigma2[ORBHIP_MAX_LEVELS], sf[ORBHIP_MAX_LEVELS]; };
struct CnmpArgs {
    const int *kf_index;               // [K]
    const float *Tcw;                  // [..][12]
    const orbhip_keypoint *keys;       // [..][cap]
    const uint8_t *desc;               // [..][cap][32]
    const int *n_dev;                  // [..]
    const float *u_right, *depth;      // [..][cap] or both null (monocular)
    const uint32_t *node;              // [..][cap]
    const uint8_t *has_point;          // [..][cap] or null
    const float *median_depth;         // [K], monocular only
    int *matches12, *nmatches;         // [K][cap], [K]
    float *x3d;                        // [K][cap][3]
    uint8_t *status, *skipped;         // [K][cap], [K]
    float *f12_out, *ep_out;           // [K][9], [K][2] or null
    CnmpRow *table;                    // [K]
    int cur, K, cap, only_stereo;
};

__device__ __forceinline__ float dot3f(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}
// C = A * B, 3x3 row-major, every element ((a0*b0 + a1*b1) + a2*b2) in float
__device__ __forceinline__ void mat3_mul(const float *A, const float *B, float *C)
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = dot3f(A[r * 3], A[r * 3 + 1], A[r * 3 + 2], B[c], B[3 + c], B[6 + c]);
}
// cv::invert of a 3x3 CV_32F matrix (small-matrix path): cofactors and determinant in double, elements rounded to float
__device__ __forceinline__ void mat3_inv(const float *M, float *out)
{
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    double d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
    if (d == 0.0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = 0.f;
        return;
    }
    d = 1.0 / d;
    out[0] = (float)((m11 * m22 - m12 * m21) * d);
    out[1] = (float)((m02 * m21 - m01 * m22) * d);
    out[2] = (float)((m01 * m12 - m02 * m11) * d);
    out[3] = (float)((m12 * m20 - m10 * m22) * d);
    out[4] = (float)((m00 * m22 - m02 * m20) * d);
    out[5] = (float)((m02 * m10 - m00 * m12) * d);
    out[6] = (float)((m10 * m21 - m11 * m20) * d);
    out[7] = (float)((m01 * m20 - m00 * m21) * d);
    out[8] = (float)((m00 * m11 - m01 * m10) * d);
}
// Ow = -Rcw^T * tcw of a [R | t] row (src/KeyFrame.cc:66-67)
__device__ __forceinline__ void camera_centre(const float *T, float *Ow)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) Ow[c] = -dot3f(T[c], T[4 + c], T[8 + c], T[3], T[7], T[11]);
}
// cv::norm of a 3-vector: squares accumulated in double
__device__ __forceinline__ double norm3d(float x, float y, float z)
{
    return __dsqrt_rn(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
}
// Frame / KeyFrame::UnprojectStereo (src/Frame.cc:666-680): X = Rcw^T * (x, y, z) + Ow
__device__ __forceinline__ void unproject_stereo(const float *T, const float *Ow, float u, float v, float z, float cx, float cy,
                                                 float invfx, float invfy, float *X)
{
    const float x = __fmul_rn(__fmul_rn(__fsub_rn(u, cx), z), invfx);
    const float y = __fmul_rn(__fmul_rn(__fsub_rn(v, cy), z), invfy);
#pragma unroll
    for (int r = 0; r < 3; ++r)
        X[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[r], x), __fmul_rn(T[4 + r], y)), __fmul_rn(T[8 + r], z)), Ow[r]);
}

__global__ __launch_bounds__(64) void k_cnmp_rows(CnmpArgs A, orbhip_camera cam)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= A.K) return;
    const float *T1 = A.Tcw + (size_t)A.cur * 12, *T2 = A.Tcw + (size_t)A.kf_index[k] * 12;
    float Ow1[3], Ow2[3];
    camera_centre(T1, Ow1);
    camera_centre(T2, Ow2);
    // :246-261
    const float baseline = (float)norm3d(__fsub_rn(Ow2[0], Ow1[0]), __fsub_rn(Ow2[1], Ow1[1]), __fsub_rn(Ow2[2], Ow1[2]));
    bool skip;
    if (A.median_depth) skip = (double)__fdiv_rn(baseline, A.median_depth[k]) < 0.01;
    else skip = baseline < cam.mb;
    CnmpRow row;
#pragma unroll
    for (int i = 0; i < 9; ++i) row.f12[i] = 0.f;
    row.ex = 0.f; row.ey = 0.f; row.skip = skip ? 1 : 0;
    if (!skip) {
        float R1[9], R2t[9], R12[9], nR12[9], t12[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) { R1[r * 3 + c] = T1[r * 4 + c]; R2t[r * 3 + c] = T2[c * 4 + r]; }
        mat3_mul(R1, R2t, R12);                         // :543
#pragma unroll
        for (int i = 0; i < 9; ++i) nR12[i] = -R12[i];  // (-R1w) * R2w.t(): negation commutes with the rounding
#pragma unroll
        for (int r = 0; r < 3; ++r)                     // :544
            t12[r] = __fadd_rn(dot3f(nR12[r * 3], nR12[r * 3 + 1], nR12[r * 3 + 2], T2[3], T2[7], T2[11]), T1[r * 4 + 3]);
        const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
        const float Kt[9] = {cam.fx, 0.f, 0.f, 0.f, cam.fy, 0.f, cam.cx, cam.cy, 1.f};
        const float Km[9] = {cam.fx, 0.f, cam.cx, 0.f, cam.fy, cam.cy, 0.f, 0.f, 1.f};
        float Kti[9], Ki[9], M1[9], M2[9];
        mat3_inv(Kt, Kti);
        mat3_inv(Km, Ki);
        mat3_mul(Kti, tx, M1);                          // :552, left to right
        mat3_mul(M1, R12, M2);
        mat3_mul(M2, Ki, row.f12);
        // epipole of camera 1 in image 2, src/ORBmatcher.cc:664-670
        float C2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            C2[r] = __fadd_rn(dot3f(T2[r * 4], T2[r * 4 + 1], T2[r * 4 + 2], Ow1[0], Ow1[1], Ow1[2]), T2[r * 4 + 3]);
        const float invz = __fdiv_rn(1.0f, C2[2]);
        row.ex = __fadd_rn(__fmul_rn(__fmul_rn(cam.fx, C2[0]), invz), cam.cx);
        row.ey = __fadd_rn(__fmul_rn(__fmul_rn(cam.fy, C2[1]), invz), cam.cy);
    }
    A.table[k] = row;
    if (A.n_dev[A.cur] <= 0) return;   // empty current key frame: the call writes nothing
    A.nmatches[k] = 0;
    A.skipped[k] = (uint8_t)row.skip;
    if (A.f12_out)
#pragma unroll
        for (int i = 0; i < 9; ++i) A.f12_out[(size_t)k * 9 + i] = row.f12[i];
    if (A.ep_out) { A.ep_out[(size_t)k * 2] = row.ex; A.ep_out[(size_t)k * 2 + 1] = row.ey; }
}

__global__ __launch_bounds__(256) void k_cnmp_search(CnmpArgs A, CnmpLevels L)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.y, qi = blockIdx.x * 4 + wv;
    const size_t c = (size_t)A.cur, f = (size_t)A.kf_index[k];
    const int n1 = max(min(A.n_dev[c], A.cap), 0);
    if (qi >= n1) return;
    int *out = A.matches12 + (size_t)k * A.cap;
    const CnmpRow row = A.table[k];
    const int n2 = max(min(A.n_dev[f], A.cap), 0);
    const size_t q = c * A.cap + qi;
    const uint32_t qnode = A.node[q];
    const float ur1 = A.u_right ? A.u_right[q] : -1.0f;
    const bool stereo1 = ur1 >= 0;
    // queries of the reference: in the FeatureVector, no map point yet (:697-703), stereo when bOnlyStereo (:706-708)
    if (row.skip || n2 == 0 || qnode == ORBHIP_NO_NODE || (A.has_point && A.has_point[q]) || (A.only_stereo && !stereo1)) {
        if (lane == 0) out[qi] = -1;
        return;
    }
    uint32_t qd[8];
    const uint32_t *qp = reinterpret_cast<const uint32_t *>(A.desc + q * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) qd[i] = qp[i];
    const orbhip_keypoint kq = A.keys[q];
    const int best =
        tri_scan(lane, n2, A.keys + f * A.cap, A.desc + f * A.cap * 32, A.u_right ? A.u_right + f * A.cap : nullptr,
                 A.node + f * A.cap, A.has_point ? A.has_point + f * A.cap : nullptr, true, A.only_stereo != 0, qnode, qd,
                 kq.x, kq.y, stereo1, row.f12, row.ex, row.ey, L.sigma2, L.sf);
    if (lane == 0) out[qi] = best;
}

__global__ __launch_bounds__(1024) void k_cnmp_cull(CnmpArgs A)
{
    const size_t k = blockIdx.x, c = (size_t)A.cur, f = (size_t)A.kf_index[k];
    const orbhip_keypoint *k1 = A.keys + c * A.cap;
    rot_cull_body(A.matches12 + k * A.cap, max(min(A.n_dev[c], A.cap), 0), &k1->angle, sizeof(orbhip_keypoint),
                  A.keys + f * A.cap, 1, nullptr);
}

__device__ __forceinline__ float dot4f(const float (&a)[4], const float (&b)[4])
{
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2])),
                     __fmul_rn(a[3], b[3]));
}
// Right singular vector of the smallest singular value of the 4x4 matrix whose COLUMNS are a[0..3]: one-sided (Hestenes)
// Jacobi in fp32.  Pairs in the fixed order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair is rotated unless
// |a_p . a_q| <= 2 eps sqrt(|a_p|^2 |a_q|^2); the sweeps stop after one without a rotation, or after kJacobiSweeps.
// Smallest = the column with the smallest squared norm, the first one on ties.  All indices are compile-time: registers.
// The cap: on the triangulation matrices of the test scenes most systems stop by the rule after 4 or 5 sweeps; about one
// in twelve never does (its null column is rounding noise, which no relative threshold calls orthogonal), but x3D has
// stopped changing, bit for bit, after sweep 3 in every one of them.  8 leaves that a factor of two.
constexpr int kJacobiSweeps = 8;
__device__ __forceinline__ void jacobi_null4(float (&a)[4][4], float (&x)[4])
{
    float v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.f : 0.f;
    const float eps = 2.384185791015625e-07f;   // 2 * FLT_EPSILON
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        bool changed = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const float alpha = dot4f(a[p], a[p]), beta = dot4f(a[q], a[q]), gamma = dot4f(a[p], a[q]);
                if (fabsf(gamma) <= __fmul_rn(eps, sqrt_rn(__fmul_rn(alpha, beta)))) continue;
                changed = true;
                const float p2 = __fmul_rn(gamma, 2.f), bt = __fsub_rn(alpha, beta);
                const float g = sqrt_rn(__fadd_rn(__fmul_rn(p2, p2), __fmul_rn(bt, bt)));
                float cs, sn;
                if (bt < 0.f) {
                    const float delta = __fmul_rn(__fsub_rn(g, bt), 0.5f);
                    sn = sqrt_rn(__fdiv_rn(delta, g));
                    cs = __fdiv_rn(p2, __fmul_rn(__fmul_rn(g, sn), 2.f));
                } else {
                    cs = sqrt_rn(__fdiv_rn(__fadd_rn(g, bt), __fmul_rn(g, 2.f)));
                    sn = __fdiv_rn(p2, __fmul_rn(__fmul_rn(g, cs), 2.f));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float ap = a[p][r], aq = a[q][r], vp = v[p][r], vq = v[q][r];
                    a[p][r] = __fadd_rn(__fmul_rn(cs, ap), __fmul_rn(sn, aq));
                    a[q][r] = __fsub_rn(__fmul_rn(cs, aq), __fmul_rn(sn, ap));
                    v[p][r] = __fadd_rn(__fmul_rn(cs, vp), __fmul_rn(sn, vq));
                    v[q][r] = __fsub_rn(__fmul_rn(cs, vq), __fmul_rn(sn, vp));
                }
            }
        if (!changed) break;
    }
    float w = dot4f(a[0], a[0]);
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = v[0][r];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const float wc = dot4f(a[c], a[c]);
        const bool less = wc < w;
        w = less ? wc : w;
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = less ? v[c][r] : x[r];
    }
}

// (x, y, z) = R * X + t of a [R | t] row as the reference evaluates Rcw.row(i).dot(x3Dt) + tcw(i): Mat::dot accumulates
// in double, the sum with the float translation is made in double and rounded once
__device__ __forceinline__ float row_dot_d(const float *T, int r, const float *X)
{
    const double d = ((double)T[r * 4] * (double)X[0] + (double)T[r * 4 + 1] * (double)X[1]) + (double)T[r * 4 + 2] * (double)X[2];
    return (float)(d + (double)T[r * 4 + 3]);
}
// Reprojection gate :362-413: true = fails
__device__ __forceinline__ bool reproj_fails(const orbhip_camera &cam, const float *T, const float *X, float z, bool stereo,
                                             float ku, float kv, float kur, float sigma2)
{
    const float x = row_dot_d(T, 0, X), y = row_dot_d(T, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(cam.fx, x), invz), cam.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(cam.fy, y), invz), cam.cy);
    const float ex = __fsub_rn(u, ku), ey = __fsub_rn(v, kv);
    float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (!stereo) return (double)e2 > 5.991 * (double)sigma2;
    const float er = __fsub_rn(__fsub_rn(u, __fmul_rn(cam.mbf, invz)), kur);
    e2 = __fadd_rn(e2, __fmul_rn(er, er));
    return (double)e2 > 7.8 * (double)sigma2;
}
// cos(2 atan2(mb/2, depth)) as (d^2 - h^2) / (d^2 + h^2) in double, h = mb/2 (:312-314)
__device__ __forceinline__ float cos_parallax_stereo(float mb, float depth)
{
    const double h = (double)__fmul_rn(mb, 0.5f), d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

__global__ __launch_bounds__(256) void k_cnmp_triangulate(CnmpArgs A, orbhip_camera cam, CnmpLevels L)
{
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const size_t c = (size_t)A.cur, f = (size_t)A.kf_index[k];
    const int n1 = max(min(A.n_dev[c], A.cap), 0);
    const size_t o = (size_t)k * A.cap + i;
    const int j = i < n1 ? A.matches12[o] : -1;
    const int cnt = __popcll(__ballot(j >= 0));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&A.nmatches[k], cnt);
    if (i >= n1) return;
    float X[3] = {0.f, 0.f, 0.f};
    int st = ORBHIP_NEWPOINT_NO_MATCH;
    if (j >= 0) {
        // the two poses are wave-uniform: held in scalar registers, the vector registers stay free for the 4x4 problem
        float T1[12], T2[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            T1[e] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(A.Tcw[c * 12 + e])));
            T2[e] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(A.Tcw[f * 12 + e])));
        }
        const orbhip_keypoint kp1 = A.keys[c * A.cap + i], kp2 = A.keys[f * A.cap + j];
        const float ur1 = A.u_right ? A.u_right[c * A.cap + i] : -1.0f, ur2 = A.u_right ? A.u_right[f * A.cap + j] : -1.0f;
        const bool s1 = ur1 >= 0, s2 = ur2 >= 0;
        const int o1 = min(max(kp1.octave, 0), ORBHIP_MAX_LEVELS - 1), o2 = min(max(kp2.octave, 0), ORBHIP_MAX_LEVELS - 1);
        const float invfx = __fdiv_rn(1.0f, cam.fx), invfy = __fdiv_rn(1.0f, cam.fy);
        // parallax between the rays, :300-305
        const float xn1[2] = {__fmul_rn(__fsub_rn(kp1.x, cam.cx), invfx), __fmul_rn(__fsub_rn(kp1.y, cam.cy), invfy)};
        const float xn2[2] = {__fmul_rn(__fsub_rn(kp2.x, cam.cx), invfx), __fmul_rn(__fsub_rn(kp2.y, cam.cy), invfy)};
        float r1[3], r2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            r1[r] = dot3f(T1[r], T1[4 + r], T1[8 + r], xn1[0], xn1[1], 1.0f);
            r2[r] = dot3f(T2[r], T2[4 + r], T2[8 + r], xn2[0], xn2[1], 1.0f);
        }
        const double dd = ((double)r1[0] * (double)r2[0] + (double)r1[1] * (double)r2[1]) + (double)r1[2] * (double)r2[2];
        const float cos_rays = (float)(dd / (norm3d(r1[0], r1[1], r1[2]) * norm3d(r2[0], r2[1], r2[2])));
        float cs1 = __fadd_rn(cos_rays, 1.0f), cs2 = cs1;
        if (s1) cs1 = cos_parallax_stereo(cam.mb, A.depth[c * A.cap + i]);
        else if (s2) cs2 = cos_parallax_stereo(cam.mb, A.depth[f * A.cap + j]);
        const float cs = fminf(cs1, cs2);
        bool have = true;
        if (cos_rays < cs && cos_rays > 0.f && (s1 || s2 || (double)cos_rays < 0.9998)) {
            // linear triangulation :322-337; a[col][row] of A
            float a[4][4], x[4];
#pragma unroll
            for (int col = 0; col < 4; ++col) {
                a[col][0] = __fsub_rn(__fmul_rn(xn1[0], T1[8 + col]), T1[col]);
                a[col][1] = __fsub_rn(__fmul_rn(xn1[1], T1[8 + col]), T1[4 + col]);
                a[col][2] = __fsub_rn(__fmul_rn(xn2[0], T2[8 + col]), T2[col]);
                a[col][3] = __fsub_rn(__fmul_rn(xn2[1], T2[8 + col]), T2[4 + col]);
            }
            jacobi_null4(a, x);
            if (x[3] == 0.f) { st = ORBHIP_NEWPOINT_W_ZERO; have = false; }
            else {
#pragma unroll
                for (int r = 0; r < 3; ++r) X[r] = __fdiv_rn(x[r], x[3]);
            }
        } else if (s1 && cs1 < cs2) {
            float Ow1[3];
            camera_centre(T1, Ow1);
            unproject_stereo(T1, Ow1, kp1.x, kp1.y, A.depth[c * A.cap + i], cam.cx, cam.cy, invfx, invfy, X);
        } else if (s2 && cs2 < cs1) {
            float Ow2[3];
            camera_centre(T2, Ow2);
            unproject_stereo(T2, Ow2, kp2.x, kp2.y, A.depth[f * A.cap + j], cam.cx, cam.cy, invfx, invfy, X);
        } else { st = ORBHIP_NEWPOINT_LOW_PARALLAX; have = false; }
        if (have) {
            const float z1 = row_dot_d(T1, 2, X), z2 = row_dot_d(T2, 2, X);
            if (z1 <= 0.f) st = ORBHIP_NEWPOINT_BEHIND_1;
            else if (z2 <= 0.f) st = ORBHIP_NEWPOINT_BEHIND_2;
            else if (reproj_fails(cam, T1, X, z1, s1, kp1.x, kp1.y, ur1, L.sigma2[o1])) st = ORBHIP_NEWPOINT_REPROJ_1;
            else if (reproj_fails(cam, T2, X, z2, s2, kp2.x, kp2.y, ur2, L.sigma2[o2])) st = ORBHIP_NEWPOINT_REPROJ_2;
            else {
                // scale consistency :415-431
                float Ow1[3], Ow2[3];
                camera_centre(T1, Ow1);
                camera_centre(T2, Ow2);
                const float d1 = (float)norm3d(__fsub_rn(X[0], Ow1[0]), __fsub_rn(X[1], Ow1[1]), __fsub_rn(X[2], Ow1[2]));
                const float d2 = (float)norm3d(__fsub_rn(X[0], Ow2[0]), __fsub_rn(X[1], Ow2[1]), __fsub_rn(X[2], Ow2[2]));
                if (d1 == 0.f || d2 == 0.f) st = ORBHIP_NEWPOINT_ZERO_DIST;
                else {
                    const float ratio_factor = __fmul_rn(1.5f, L.sf[cam.n_levels > 1 ? 1 : 0]);
                    const float ratio_dist = __fdiv_rn(d2, d1), ratio_oct = __fdiv_rn(L.sf[o1], L.sf[o2]);
                    st = (__fmul_rn(ratio_dist, ratio_factor) < ratio_oct || ratio_dist > __fmul_rn(ratio_oct, ratio_factor))
                             ? ORBHIP_NEWPOINT_SCALE : ORBHIP_NEWPOINT_CREATED;
                }
            }
        }
    }
    A.status[o] = (uint8_t)st;
    A.x3d[o * 3] = X[0]; A.x3d[o * 3 + 1] = X[1]; A.x3d[o * 3 + 2] = X[2];
}

// ---- independent best match per query (no slot blocking) ------------------------------------
// Inner loop of ORBmatcher::Fuse (ORBmatcher.cc:893-950, :1045-1075) and of both directions of SearchBySim3
// (:1199-1219, :1279-1299): GetFeaturesInArea window, level window, optional chi-square gate on the
// reprojection error (Fuse: 5.99 mono / 7.8 stereo, scaled by mvInvLevelSigma2[level]), Hamming argmin with the
// reference's first-minimum tie-break.  One wavefront per query.
__global__ __launch_bounds__(256) void k_best_in_window(DevFrame F, const uint32_t *__restrict__ ord,
                                                        const orbhip_query *__restrict__ q,
                                                        const uint8_t *__restrict__ qdesc, int nq, int chi2_gate,
                                                        SigmaTab sig, int *__restrict__ best_idx,
                                                        int *__restrict__ best_dist)
{
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const orbhip_query Q = q[qi];
    unsigned long long best = ~0ull;
    if (Q.valid) {
        const CellWindow W = cell_window(Q.u, Q.v, Q.radius, F.min_x, F.min_y, F.inv_w, F.inv_h);
        if (!W.empty()) {
            uint32_t qd[8];
            const uint32_t *qp = reinterpret_cast<const uint32_t *>(qdesc + (size_t)qi * 32);
#pragma unroll
            for (int i = 0; i < 8; ++i) qd[i] = qp[i];
            for (int j0 = 0; j0 < F.n; j0 += 64) {
                const int j = j0 + lane;
                if (j >= F.n) continue;
                const uint32_t o = ord[j];
                if (o == kNoCell) continue;
                const int cell = (int)(o >> 20);
                const int px = cell / GRID_ROWS, py = cell - px * GRID_ROWS;
                if (!(px >= W.x0 && px <= W.x1 && py >= W.y0 && py <= W.y1)) continue;
                int d;
                if (!fuse_candidate(F.keys, F.desc, F.u_right, j, Q.u, Q.v, Q.radius, Q.ur, Q.min_level, Q.max_level,
                                    chi2_gate != 0, sig, qd, &d)) continue;
                const unsigned long long key = ((unsigned long long)d << 32) | o;
                best = key < best ? key : best;
            }
        }
    }
    best = wave_min_u64(best);
    if (lane == 0) {
        best_idx[qi] = best == ~0ull ? -1 : (int)(best & 0xfffffu);
        best_dist[qi] = best == ~0ull ? 256 : (int)(best >> 32);
    }
}

// ---- parallel resolve: modes 0 / 1 (the SearchByProjection overloads) ------------------------------------------
// The sequential reference loop hands every query, in index order, the first candidate of its list (sorted by
// (distance, visiting order)) that is neither taken on entry nor already held by an accepted, observed query with a
// smaller index.  That is serial dictatorship.
//  * Mode 0 (frame-to-frame search): acceptance depends on the first usable entry alone, so nobody
//    ever gives a held slot up, and the outcome is the unique stable matching of "queries prefer list order, slots
//    prefer the smaller query index", which deferred acceptance reaches from any proposal order: unsettled queries
//    propose (atomicMin on the slot's holder) to the first entry no smaller query holds; a holder only ever gets
//    smaller, so each query's list cursor is monotone and the total walk is the list length, not list length x rounds.
//  * Mode 1 (map points): the ratio test applies only when best and second best share a level, so losing the second
//    candidate to a smaller query can turn an acceptance into a rejection -- holders are not monotone.  There the
//    rounds re-pick every query against the previous round's claims and rebuild the claims (fixed-point iteration).
// One workgroup per pair, state in LDS.
// State of the parallel resolve.  Up to kResolveMax train keypoints and queries it lives in LDS (GS = false); beyond
// that the same arrays are carved out of an HBM workspace (GS = true: same code, global loads / atomics).
struct ResolveParState {
    int *owner[2];                       // [0]: holder of every slot (smallest accepted, observed proposer); [1]: cursors
    int *choice;                         // slot picked by query i, -1 if none accepted
    float *t_angle, *q_angle;
    unsigned char *t_oct, *q_obs, *taken, *evbin;
    int *hist;                           // HISTO_LENGTH bins
    int *vars;                           // [0], [3], [4]: rotating "a choice changed" flags; [1] accepted; [2] culled
    unsigned short *cur1, *cur2;         // per query: first list entry not known to be unavailable (best / second best)
    int *q_cnt;                          // candidates per query (sign = unsorted)
    unsigned short *wl[2];               // work lists of the event-driven rounds (queries to step next)
    uint32_t *lc;                        // first lcn entries of every query's sorted list as (distance << 20 | slot), row
    int lcn;                             // stride lcn + 1: the steps re-read list heads and must not wait for HBM
};
constexpr int kResolveLdsBudget = 156 * 1024;   // dynamic LDS the LDS variant may ask for (160 KB per CU)
constexpr int kResolveHead = 8;
__host__ __device__ inline size_t resolve_par_bytes(size_t n, size_t nq, size_t lcn = 0)
{
    n = (n + 3) & ~(size_t)3; nq = (nq + 3) & ~(size_t)3;
    return (2 * n + nq + n + nq) * 4 + 2 * n + 2 * nq + (HISTO_LENGTH + 2 + 16) * 4 + 12 * nq + (lcn ? nq * (lcn + 1) * 4 : 0);
}
__device__ __forceinline__ void resolve_par_carve(ResolveParState &S, unsigned char *base, size_t n, size_t nq, int lcn = 0)
{
    n = (n + 3) & ~(size_t)3; nq = (nq + 3) & ~(size_t)3;
    S.lcn = lcn;
    S.lc = reinterpret_cast<uint32_t *>(base + resolve_par_bytes(n, nq, 0));
    int *p = reinterpret_cast<int *>(base);
    S.owner[0] = p; p += n; S.owner[1] = p; p += n; S.choice = p; p += nq;
    S.t_angle = reinterpret_cast<float *>(p); p += n; S.q_angle = reinterpret_cast<float *>(p); p += nq;
    S.hist = p; p += HISTO_LENGTH + 2; S.vars = p; p += 16;
    S.cur1 = reinterpret_cast<unsigned short *>(p); S.cur2 = S.cur1 + nq; p += nq;
    S.wl[0] = reinterpret_cast<unsigned short *>(p); S.wl[1] = S.wl[0] + nq; p += nq;
    S.q_cnt = p; p += nq;
    unsigned char *c = reinterpret_cast<unsigned char *>(p);
    S.t_oct = c; c += n; S.taken = c; c += n; S.q_obs = c; c += nq; S.evbin = c;
}

#ifdef ORBHIP_DEVTOOLS
__device__ unsigned int g_resolve_stats[4];   // development builds: {launched workgroups, sum of rounds, max rounds, -}
// Diagnostic build only (STAMPS = true is instantiated under -DORBHIP_DEVTOOLS alone): per-phase s_memtime sums of thread 0
// of every workgroup (each phase ends at a barrier, so its stamps are the workgroup's) -- {state init + head loads, first
// full step, event-driven rounds (mode 1: all rounds), unobserved pass, assign + histogram, cull, output, workgroups} --
// read by tools/bench_track_th.py through orbhip_dev_resolve_stamps.  Shares, not lengths, are meaningful (the stamps fence).
__device__ unsigned long long g_resolve_stamps[8];
#endif
// time stamp of the stamped instantiation; the wait and the scheduling barriers fence it
__device__ __forceinline__ unsigned long long resolve_stamp_now()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
template <bool GS, bool STAMPS = false>
__global__ __launch_bounds__(1024) void k_resolve_par(int mode, DevFrame F, const orbhip_query *__restrict__ q, int nq,
                                                      const unsigned long long *__restrict__ cand,
                                                      const unsigned long long *__restrict__ ccand,
                                                      const int *__restrict__ cnt, int stride,
                                                      const uint8_t *__restrict__ taken_in, float nnratio,
                                                      int check_ori, int *__restrict__ out, int *__restrict__ out_n, Batch B,
                                                      int th_accept, int all_block, unsigned char *__restrict__ gstate,
                                                      size_t gstate_stride, int lcn)
{
    extern __shared__ unsigned char resolve_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    unsigned long long tacc[7] = {0, 0, 0, 0, 0, 0, 0}, tprev = 0;
#define RESOLVE_STAMP(i) do { if constexpr (STAMPS) { const unsigned long long t_ = resolve_stamp_now(); tacc[i] += t_ - tprev; tprev = t_; } } while (0)
    if constexpr (STAMPS) tprev = resolve_stamp_now();
    {
        const int pair = blockIdx.x;
        batch_frame(F, B, pair);
        q += (size_t)pair * B.qcap;
        cand += (size_t)pair * B.qcap * stride;
        if (ccand) ccand += (size_t)pair * B.qcap * kCompact;
        cnt += (size_t)pair * B.qcap;
        if (taken_in) taken_in += (size_t)pair * B.cap;
        out += (size_t)pair * B.cap;
        out_n += pair;
        if (B.nq_dev) nq = min(B.nq_dev[pair], B.qcap);
    }
    const int n = F.n;
    ResolveParState S;
    if (GS) resolve_par_carve(S, gstate + (size_t)blockIdx.x * gstate_stride, (size_t)n, (size_t)nq);
    else resolve_par_carve(S, resolve_lds, (size_t)B.cap, (size_t)B.qcap, lcn);   // laid out for the capacities
    int *holder = S.owner[0];
    unsigned short *cur1 = S.cur1, *cur2 = S.cur2;
    // The list heads of this thread's first query are requested before anything else, without waiting for the list
    // length (a compact list always has its 64 entries allocated), so that ONE memory round trip covers them and the
    // per-frame state below; heads and lengths then live in LDS: the rounds must never wait for HBM.
    const bool lc_on = !GS && S.lcn > 0;
    unsigned long long hv[kResolveHead];
    int head_c = 0;
    if (tid < nq) {
        head_c = cnt[tid];
        if (lc_on && ccand) {
            const unsigned long long *l0 = ccand + (size_t)tid * kCompact;
#pragma unroll
            for (int e = 0; e < kResolveHead; ++e) hv[e] = l0[e];
        }
    }
    for (int i = tid; i < n; i += T) {
        holder[i] = INT_MAX;
        S.taken[i] = (unsigned char)(taken_in ? taken_in[i] != 0 : 0);
        S.t_angle[i] = F.keys[i].angle;
        S.t_oct[i] = (unsigned char)F.keys[i].octave;
    }
    for (int i = tid; i < nq; i += T) {
        S.choice[i] = -2;   // "not evaluated yet"
        S.q_angle[i] = q[i].angle;
        S.q_obs[i] = (unsigned char)(all_block || q[i].observed != 0);
        S.evbin[i] = 0xff;
        cur1[i] = 0; cur2[i] = 0;
        S.q_cnt[i] = i == tid ? head_c : cnt[i];
    }
    if (tid < HISTO_LENGTH) S.hist[tid] = 0;
    if (tid < 16) S.vars[tid] = 0;
    if (lc_on) {
        for (int i = tid; i < nq; i += T) {
            const int c = S.q_cnt[i];
            if (c == 0) continue;
            if (c < 0) {   // unsorted list: the window search left the head of its sorted order in the compact row
                if (ccand && S.lcn >= kHeadMax) {
                    const unsigned long long *hrow = ccand + (size_t)i * kCompact;
#pragma unroll
                    for (int e = 0; e < kHeadMax; ++e) {
                        const unsigned long long h = hrow[e];
                        S.lc[i * (S.lcn + 1) + e] = ((uint32_t)(h >> 32) << 20) | (uint32_t)(h & 0xfffffu);
                    }
                    S.lc[i * (S.lcn + 1) + S.lcn] = (uint32_t)hrow[kHeadMax];
                }
                continue;
            }
            if (i != tid || !ccand) {
                const unsigned long long *l0 = ccand ? ccand + (size_t)i * kCompact : cand + (size_t)i * stride;
#pragma unroll
                for (int e = 0; e < kResolveHead; ++e) hv[e] = (e < c && e < S.lcn) ? l0[e] : ~0ull;
            }
#pragma unroll
            for (int e = 0; e < kResolveHead; ++e)
                if (e < c && e < S.lcn) S.lc[i * (S.lcn + 1) + e] = ((uint32_t)(hv[e] >> 32) << 20) | (uint32_t)(hv[e] & 0xfffffu);
        }
    }
    __syncthreads();
    RESOLVE_STAMP(0);   // state init + head loads
    // One deferred-acceptance step of query i against the holders as they are right now (any interleaving of proposals
    // is a valid execution, the atomics are the only synchronisation the matching needs).  Returns "the choice changed".
    auto held_by_smaller = [&](int idx, int i) -> bool {
        return S.taken[idx] || __hip_atomic_load(&holder[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < i;
    };
    unsigned short *wl_next = nullptr;   // set by the event-driven rounds
    int *wl_count = nullptr;
    int *claim = holder;                 // where an accepted, observed query files its claim
    bool claims_rebuilt = false;         // mode 1: the claims are rebuilt from scratch every round
    // pick: best (and, mode 1, second best) available entry of query i's list.  A sorted list (<= 64 candidates) is walked
    // by the thread that owns the query; an unsorted one (more candidates: wide windows) by the whole wavefront, lanes over
    // the entries (step_group below).
    auto pick_sorted = [&](int i, int c, unsigned long long &k1, unsigned long long &k2) {
        const unsigned long long *list = ccand ? ccand + (size_t)i * kCompact : cand + (size_t)i * stride;
        const uint32_t *lrow = S.lc + i * (S.lcn + 1);
        auto entry = [&](int e) -> unsigned long long {
            if (e >= c) return ~0ull;
            if (!GS && e < S.lcn) { const uint32_t w = lrow[e]; return ((unsigned long long)(w >> 20) << 32) | (w & 0xfffffu); }
            return list[e];
        };
        // four entries per trip: their eight LDS reads (taken, holder) are in flight together
        int e1 = mode == 1 ? 0 : cur1[i];
        while (e1 < c) {
            const unsigned long long v0 = entry(e1), v1 = entry(e1 + 1), v2 = entry(e1 + 2), v3 = entry(e1 + 3);
            const bool a0 = !held_by_smaller((int)(v0 & 0xfffffu), i);
            const bool a1 = v1 != ~0ull && !held_by_smaller((int)(v1 & 0xfffffu), i);
            const bool a2 = v2 != ~0ull && !held_by_smaller((int)(v2 & 0xfffffu), i);
            const bool a3 = v3 != ~0ull && !held_by_smaller((int)(v3 & 0xfffffu), i);
            if (a0) { k1 = v0; break; }
            if (a1) { k1 = v1; e1 += 1; break; }
            if (a2) { k1 = v2; e1 += 2; break; }
            if (a3) { k1 = v3; e1 += 3; break; }
            e1 += 4;
        }
        e1 = min(e1, c);
        if (mode != 1) cur1[i] = (unsigned short)e1;
        if (mode == 1 && e1 < c) {
            for (int e2 = e1 + 1; e2 < c; ++e2) {
                const unsigned long long v = entry(e2);
                if (!held_by_smaller((int)(v & 0xfffffu), i)) { k2 = v; break; }
            }
        }
    };
    auto pick_unsorted_wave = [&](int i, int len, unsigned long long &k1, unsigned long long &k2) {   // every lane, same (i, len)
        const unsigned long long *list = cand + (size_t)i * stride;
        unsigned long long a1 = ~0ull, a2 = ~0ull;
        for (int e = (int)(threadIdx.x & 63); e < len; e += 64) {
            const unsigned long long v = list[e];
            if (held_by_smaller((int)(v & 0xfffffu), i)) continue;
            if (v < a1) { a2 = a1; a1 = v; } else if (v < a2) a2 = v;
        }
        k1 = wave_min_u64(a1);
        k2 = mode == 1 ? wave_min_u64(a1 == k1 ? a2 : a1) : ~0ull;   // keys are unique (the slot is part of the key)
    };
    auto commit = [&](int i, unsigned long long k1, unsigned long long k2) -> bool {
        int newc = -1;
        if (k1 != ~0ull) {
            const int bestDist = (int)(k1 >> 32), bestIdx = (int)(k1 & 0xfffffu);
            bool acc = bestDist <= th_accept;
            if (acc && mode == 1) {
                const int bestDist2 = k2 == ~0ull ? 256 : (int)(k2 >> 32);
                const int bestLevel = S.t_oct[bestIdx];
                const int bestLevel2 = k2 == ~0ull ? -1 : (int)S.t_oct[(int)(k2 & 0xfffffu)];
                if (bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2)) acc = false;
            }
            if (acc) newc = bestIdx;
        }
        const bool changed = newc != S.choice[i];
        if (!changed && !claims_rebuilt) return false;
        S.choice[i] = newc;
        if (newc >= 0 && S.q_obs[i]) {
            const int old = atomicMin(&claim[newc], i);
            // event-driven rounds: whoever loses the slot steps again -- me if a smaller query got there first, the
            // previous holder if I displaced it
            if (wl_next) {
                const int again = old < i ? i : (old != INT_MAX ? old : -1);
                if (again >= 0) wl_next[atomicAdd(wl_count, 1)] = (unsigned short)again;
            }
        }
        return changed;
    };
    // One deferred-acceptance / fixed-point step for the queries of a whole wavefront (lane: query i, `valid` false for
    // idle lanes; every lane of the wavefront must call).  Queries with unsorted lists are taken one after the other by
    // the whole wavefront -- a single thread re-scanning a 300-entry list in HBM on every step is what made wide windows
    // slow (th = 60: 293 us, th = 100: 556 us per 32 pairs).
    // Unsorted lists with a sorted head in LDS (the LDS variant with list heads; `head_on`): the owner thread walks the
    // head -- kHeadMax keys in list order, candidates taken on entry left out -- like a sorted list.  Frame search: the
    // cursor is monotone, and when the head runs out before the list does the wavefront refills it with the next keys
    // behind the last one (one scan of the list per kHeadMax steps instead of one per step).  Map-point search: first and
    // second free entry of the initial head; if the head cannot tell (not both found and the list goes on) the wavefront
    // scans the whole list.  Returns "needs the wavefront".
    const bool head_on = lc_on && S.lcn >= kHeadMax && ccand != nullptr;
    auto expand = [](uint32_t w) -> unsigned long long { return ((unsigned long long)(w >> 20) << 32) | (w & 0xfffffu); };
    auto head_walk = [&](int i, unsigned long long &k1, unsigned long long &k2) -> bool {
        const uint32_t *lrow = S.lc + i * (S.lcn + 1);
        const uint32_t meta = lrow[S.lcn];
        const int hl = (int)(meta & 0xffu);
        const bool complete = (meta & 0x100u) != 0;
        if (mode != 1) {
            int e = cur1[i];
            while (e < hl) {
                const uint32_t w = lrow[e];
                if (!held_by_smaller((int)(w & 0xfffffu), i)) { k1 = expand(w); break; }
                ++e;
            }
            cur1[i] = (unsigned short)e;
            return e >= hl && !complete;
        }
        k1 = k2 = ~0ull;
        for (int e = 0; e < hl; ++e) {
            const uint32_t w = lrow[e];
            if (held_by_smaller((int)(w & 0xfffffu), i)) continue;
            if (k1 == ~0ull) k1 = expand(w); else { k2 = expand(w); break; }
        }
        return k2 == ~0ull && !complete;
    };
    auto refill_head_wave = [&](int i, int len) {   // every lane, same (i, len): the next keys behind the head's last one
        const int lane = (int)(threadIdx.x & 63);
        uint32_t *lrow = S.lc + i * (S.lcn + 1);
        const int hl = (int)(lrow[S.lcn] & 0xffu);
        // the head's last key in full: the LDS copy holds (distance, slot); the cell bits of the key are the slot's grid
        // cell.  PosInGrid spelled out, without grid_cell's rejection select: a listed candidate is never a key point that
        // PosInGrid rejects, and with the select this kernel measured slower than the parent (profiles/grid_rules.json)
        unsigned long long cursor = 0ull;
        if (hl > 0) {
            const uint32_t w = lrow[hl - 1];
            const int slot = (int)(w & 0xfffffu);
            const orbhip_keypoint kp = F.keys[slot];
            const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, F.min_x), F.inv_w));
            const int py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, F.min_y), F.inv_h));
            cursor = ((unsigned long long)(w >> 20) << 32) | ((unsigned long long)(uint32_t)(px * GRID_ROWS + py) << 20) | (uint32_t)slot;
        }
        const unsigned long long *list = cand + (size_t)i * stride;
        unsigned long long a1 = ~0ull, a2 = ~0ull;
        int na = 0;
        for (int e = lane; e < len; e += 64) {
            const unsigned long long v = list[e];
            if ((hl > 0 && v <= cursor) || S.taken[(int)(v & 0xfffffu)]) continue;
            if (v < a1) { a2 = a1; a1 = v; } else if (v < a2) a2 = v;
            ++na;
        }
        unsigned long long head[kHeadMax];
        bool complete;
        const int nh = wave_sorted_head(a1, a2, na > 2, head, &complete);
        wave_lds_handoff();                               // every lane has read the old head
        if (lane < kHeadMax) {
            unsigned long long v = head[0];
#pragma unroll
            for (int k = 1; k < kHeadMax; ++k) if (lane == k) v = head[k];
            lrow[lane] = ((uint32_t)(v >> 32) << 20) | (uint32_t)(v & 0xfffffu);
        }
        if (lane == 0) lrow[S.lcn] = (uint32_t)nh | (complete ? 0x100u : 0u);
        wave_lds_handoff();                               // the owner of query i walks the new head
    };
    // One deferred-acceptance / fixed-point step for the queries of a whole wavefront (lane: query i, `valid` false for
    // idle lanes; every lane of the wavefront must call).  What an unsorted list needs from the whole wavefront -- a
    // refill of its head, or a scan -- is done for one query after the other, lanes over the list entries: a single
    // thread re-scanning a 300-entry list in HBM on every step is what made wide windows slow (th = 60: 293 us,
    // th = 100: 556 us per 32 pairs).
    auto step_group = [&](int i, bool valid) -> bool {
        const int lane = (int)(threadIdx.x & 63);
        const int c = valid ? S.q_cnt[i] : 0;
        unsigned long long k1 = ~0ull, k2 = ~0ull;
        if (c > 0) pick_sorted(i, c, k1, k2);
        bool need = c < 0;
        if (need && head_on) need = head_walk(i, k1, k2);
        if (head_on && mode != 1) {
            for (;;) {
                unsigned long long longs = __ballot(need);
                if (!longs) break;
                while (longs) {
                    const int src = __ffsll((long long)longs) - 1;
                    refill_head_wave(__builtin_amdgcn_readlane(i, src), -__builtin_amdgcn_readlane(c, src));
                    longs &= longs - 1;
                }
                if (need) { cur1[i] = 0; need = head_walk(i, k1, k2); }
            }
        } else {
            unsigned long long longs = __ballot(need);
            while (longs) {
                const int src = __ffsll((long long)longs) - 1;
                unsigned long long t1, t2;
                pick_unsorted_wave(__builtin_amdgcn_readlane(i, src), -__builtin_amdgcn_readlane(c, src), t1, t2);
                if (lane == src) { k1 = t1; k2 = t2; }
                longs &= longs - 1;
            }
        }
        return valid && c != 0 ? commit(i, k1, k2) : (valid ? commit(i, ~0ull, ~0ull) : false);
    };
    if (mode != 1) {
        // Event-driven rounds (no second candidate, so a query's choice can only change when it loses its slot): the
        // first round steps every query, every later one only the queries the previous round pushed out -- the whole
        // pair lives on one CU, so the rounds are bound by instruction issue, and the work lists keep most wavefronts
        // out of them.  Counters vars[5..7] rotate: read / filled / reset.  Queries that do not hold slots
        // (unobserved) are not told when their pick is taken, they take one more step at the end.
        int c_in = 5, c_out = 6, c_clr = 7, rounds = 0;
        unsigned short *w_in = S.wl[0], *w_out = S.wl[1];
        wl_next = w_out; wl_count = &S.vars[c_out];
        for (int i0 = 0; i0 < nq; i0 += T) step_group(i0 + tid, i0 + tid < nq);
        __syncthreads();
        RESOLVE_STAMP(1);   // first full step
        for (;; ++rounds) {
            { unsigned short *t_ = w_in; w_in = w_out; w_out = t_; }
            { const int t_ = c_in; c_in = c_out; c_out = c_clr; c_clr = t_; }
            const int nw = S.vars[c_in];
            if (nw == 0 || rounds > 65 * nq) break;
            if (tid == 0) S.vars[c_clr] = 0;
            wl_next = w_out; wl_count = &S.vars[c_out];
            for (int k0 = 0; k0 < nw; k0 += T) step_group(k0 + tid < nw ? (int)w_in[k0 + tid] : 0, k0 + tid < nw);
            __syncthreads();
        }
        wl_next = nullptr;
        RESOLVE_STAMP(2);   // event-driven rounds
        bool unobs = false;
        for (int i = tid; i < nq; i += T) unobs |= !S.q_obs[i];
        if (__syncthreads_or(unobs))
            for (int i0 = 0; i0 < nq; i0 += T) step_group(i0 + tid, i0 + tid < nq && !S.q_obs[i0 + tid]);
#ifdef ORBHIP_DEVTOOLS
        if (tid == 0) { atomicAdd(&g_resolve_stats[0], 1u); atomicAdd(&g_resolve_stats[1], (unsigned)rounds + 1); atomicMax(&g_resolve_stats[2], (unsigned)rounds + 1); }
#endif
    } else {
        // mode 1 (map points: second candidate, ratio test among candidates of the same level).  Here a query CAN have
        // to give a held slot up: when its second candidate is taken by a smaller query, the next one may sit on the best
        // candidate's level and fail the ratio test that the previous pair never had to take -- holders are not
        // monotone, so no deferred acceptance.  The sequential loop is still the unique solution of "every query picks
        // against the claims of the smaller queries", found by fixed-point iteration: each round all queries re-pick
        // against the claims of the previous round and the claims are rebuilt from scratch (query i is final once all
        // j < i are: at most nq + 1 rounds, a handful in practice).
        int *own_cur = S.owner[0], *own_nxt = S.owner[1];
        claims_rebuilt = true;
        for (int round = 0; round <= nq + 1; ++round) {
            if (tid == 0) S.vars[0] = 0;
            for (int c = tid; c < n; c += T) own_nxt[c] = INT_MAX;
            __syncthreads();
            holder = own_cur; claim = own_nxt;
            bool ch = false;
            for (int i0 = 0; i0 < nq; i0 += T) ch |= step_group(i0 + tid, i0 + tid < nq);
            if (ch) S.vars[0] = 1;
            __syncthreads();
            const int changed = S.vars[0];
            { int *t_ = own_cur; own_cur = own_nxt; own_nxt = t_; }
            __syncthreads();
            if (!changed) {
#ifdef ORBHIP_DEVTOOLS
                if (tid == 0) { atomicAdd(&g_resolve_stats[0], 1u); atomicAdd(&g_resolve_stats[1], (unsigned)round + 1); atomicMax(&g_resolve_stats[2], (unsigned)round + 1); }
#endif
                break;
            }
        }
    }
    __syncthreads();
    if (mode != 1) RESOLVE_STAMP(3); else RESOLVE_STAMP(2);   // unobserved pass; mode 1: its fixed-point rounds
    // ---- outputs: assign[slot] = last accepted query that picked it; rotation-histogram cull (mode 0) ----
    int *assign = S.owner[1];
    for (int c = tid; c < n; c += T) assign[c] = -1;
    __syncthreads();
    int acc_local = 0;
    const bool ori = mode == 0 && check_ori;
    for (int i0 = 0; i0 < nq; i0 += T) {
        const int i = i0 + tid;
        const int c = i < nq ? S.choice[i] : -1;
        int bin = -1;
        if (c >= 0) {
            ++acc_local;
            atomicMax(&assign[c], i);
            if (ori) {
                bin = rot_bin(S.q_angle[i], S.t_angle[c]);
                if (bin >= 0) S.evbin[i] = (unsigned char)bin;
            }
        }
        wave_hist_add(S.hist, bin);
    }
    acc_local = wave_sum(acc_local);
    if ((tid & 63) == 0 && acc_local) atomicAdd(&S.vars[1], acc_local);
    __syncthreads();
    RESOLVE_STAMP(4);   // assign + histogram
    if (ori) {
        rank_bins_once(S.hist, S.vars + 8);
        const int ind1 = S.vars[8], ind2 = S.vars[9], ind3 = S.vars[10];
        int cull = 0;
        for (int i = tid; i < nq; i += T) {
            if (rot_culled(S.evbin[i], ind1, ind2, ind3)) {
                assign[S.choice[i]] = -1;
                ++cull;
            }
        }
        cull = wave_sum(cull);
        if ((tid & 63) == 0 && cull) atomicAdd(&S.vars[2], cull);
        __syncthreads();
    }
    RESOLVE_STAMP(5);   // cull
    for (int c = tid; c < n; c += T) out[c] = assign[c];
    if (tid == 0) *out_n = S.vars[1] - S.vars[2];
    RESOLVE_STAMP(6);   // output (thread 0's share of it: nothing waits for the stores)
#ifdef ORBHIP_DEVTOOLS
    if constexpr (STAMPS) {
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 7; ++i) atomicAdd(&g_resolve_stamps[i], tacc[i]);
            atomicAdd(&g_resolve_stamps[7], 1ull);
        }
    }
#endif
#undef RESOLVE_STAMP
}

// ---- parallel resolve of SearchForInitialization (ORBmatcher.cc:405-520) -----------------------------------------
// The reference visits the queries in index order; a candidate slot b is usable for query i iff no earlier accepted
// query left a distance <= dist(i, b) on it (vMatchedDistance), the query takes its best usable candidate if it passes
// TH_LOW and the ratio test against the second best usable one, and a later, closer query steals the slot (the loser is
// NOT re-matched).  Every decision therefore depends only on the decisions of the queries with a smaller index: the
// sequential result is the unique fixed point of "every query decides against the claims of the smaller queries", and
// Jacobi iteration reaches it (query i is final once all j < i are).  A round rebuilds, per slot, a linked list of this
// round's claimants (atomicExch on the slot's head); the next round's queries walk the list of a candidate slot and take
// the minimum claimed distance among the claimants with a smaller index.  One workgroup per pair, state in LDS
// (n, nq <= kResolveMax: the limit the entry points already state, and the state fits the LDS budget there).
struct InitState {
    int *q_cnt; float *q_angle, *t_angle;
    uint32_t *claim[2];          // per query: distance << 20 | slot, or kNoClaim
    int *head[2];                // per slot: a claimant of this round, -1 if none
    unsigned short *next[2];     // per query: next claimant of the same slot, 0xffff = end
    unsigned char *evbin;
    int *hist, *vars;
    unsigned short *active;      // queries with a sorted list (<= 64 candidates), in index order (SearchForInitialization
                                 // only matches level-0 keypoints: about a fifth of the queries have candidates at all)
    unsigned short *active_u;    // queries with more than 64 candidates (unsorted list): a whole wavefront steps each
    uint32_t *lc; int lcn;
};
constexpr uint32_t kNoClaim = 0xffffffffu;
__host__ __device__ constexpr size_t init_state_bytes(size_t n, size_t nq, size_t lcn)
{
    n = (n + 3) & ~(size_t)3; nq = (nq + 3) & ~(size_t)3;
    return nq * 4 + nq * 4 + n * 4 + 2 * nq * 4 + 2 * n * 4 + 2 * nq * 2 + nq + 4 * nq + (HISTO_LENGTH + 2 + 64) * 4 + (lcn ? nq * (lcn + 1) * 4 : 0);
}
__global__ __launch_bounds__(1024) void k_resolve_init(DevFrame F, const orbhip_keypoint *__restrict__ qkeys, int nq,
                                                       const unsigned long long *__restrict__ cand,
                                                       const unsigned long long *__restrict__ ccand,
                                                       const int *__restrict__ cnt, int stride, float nnratio, int check_ori,
                                                       int *__restrict__ out, int *__restrict__ out_n, Batch B, int lcn)
{
    extern __shared__ unsigned char resolve_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    {
        const int pair = blockIdx.x;
        batch_frame(F, B, pair);
        if (qkeys) qkeys += (size_t)(B.qd0 + pair * B.qds) * B.qcap;
        cand += (size_t)pair * B.qcap * stride;
        ccand += (size_t)pair * B.qcap * kCompact;
        cnt += (size_t)pair * B.qcap;
        out += (size_t)pair * B.qcap;
        out_n += pair;
        if (B.nq_dev) nq = min(B.nq_dev[pair], B.qcap);
    }
    const int n = F.n;
    InitState S;
    {   // laid out for the capacities
        const size_t na = ((size_t)B.cap + 3) & ~(size_t)3, nqa = ((size_t)B.qcap + 3) & ~(size_t)3;
        int *p = reinterpret_cast<int *>(resolve_lds);
        S.q_cnt = p; p += nqa;
        S.q_angle = reinterpret_cast<float *>(p); p += nqa;
        S.t_angle = reinterpret_cast<float *>(p); p += na;
        S.claim[0] = reinterpret_cast<uint32_t *>(p); p += nqa; S.claim[1] = reinterpret_cast<uint32_t *>(p); p += nqa;
        S.head[0] = p; p += na; S.head[1] = p; p += na;
        S.hist = p; p += HISTO_LENGTH + 2; S.vars = p; p += 64;
        S.next[0] = reinterpret_cast<unsigned short *>(p); S.next[1] = S.next[0] + nqa; p += nqa;
        S.evbin = reinterpret_cast<unsigned char *>(p); p += nqa / 4;
        S.active = reinterpret_cast<unsigned short *>(p); p += nqa / 2;
        S.active_u = reinterpret_cast<unsigned short *>(p); p += nqa / 2;
        S.lc = reinterpret_cast<uint32_t *>(p); S.lcn = lcn;
    }
    // list heads of this thread's first query, requested before anything else (one memory round trip with the rest)
    unsigned long long hv[kResolveHead];
    int head_c = 0;
    if (tid < nq) {
        head_c = cnt[tid];
        if (S.lcn > 0) {
            const unsigned long long *l0 = ccand + (size_t)tid * kCompact;
#pragma unroll
            for (int e = 0; e < kResolveHead; ++e) hv[e] = l0[e];
        }
    }
    for (int i = tid; i < n; i += T) { S.t_angle[i] = F.keys[i].angle; S.head[0][i] = -1; }
    for (int i = tid; i < nq; i += T) {
        S.q_cnt[i] = i == tid ? head_c : cnt[i];
        S.q_angle[i] = qkeys[i].angle;
        S.claim[0][i] = kNoClaim; S.claim[1][i] = kNoClaim;
        S.next[0][i] = 0xffff;
        S.evbin[i] = 0xff;
    }
    if (tid < HISTO_LENGTH) S.hist[tid] = 0;
    if (tid < 64) S.vars[tid] = 0;
    if (S.lcn > 0) {
        for (int i = tid; i < nq; i += T) {
            const int c = i == tid ? head_c : cnt[i];
            if (c <= 0) continue;
            if (i != tid) {
                const unsigned long long *l0 = ccand + (size_t)i * kCompact;
#pragma unroll
                for (int e = 0; e < kResolveHead; ++e) hv[e] = (e < c && e < S.lcn) ? l0[e] : ~0ull;
            }
#pragma unroll
            for (int e = 0; e < kResolveHead; ++e)
                if (e < c && e < S.lcn) S.lc[i * (S.lcn + 1) + e] = ((uint32_t)(hv[e] >> 32) << 20) | (uint32_t)(hv[e] & 0xfffffu);
        }
    }
    __syncthreads();
    // compact the queries that have candidates (index order; sorted and unsorted lists separately): thread t owns
    // queries [t * per, (t + 1) * per)
    int nact, nact_u;
    {
        const int per = (nq + T - 1) / T, i_lo = tid * per, i_hi = min(i_lo + per, nq);
        int c = 0, cu = 0;
        for (int i = i_lo; i < i_hi; ++i) { c += S.q_cnt[i] > 0; cu += S.q_cnt[i] < 0; }
        const int incl = wave_incl_scan_add(c), inclu = wave_incl_scan_add(cu);
        if ((tid & 63) == 63) { S.vars[16 + (tid >> 6)] = incl; S.vars[32 + (tid >> 6)] = inclu; }
        __syncthreads();
        int base = incl - c, tot = 0, baseu = inclu - cu, totu = 0;
        for (int w = 0; w < (T >> 6); ++w) {
            const int v = S.vars[16 + w], vu = S.vars[32 + w];
            if (w < (tid >> 6)) { base += v; baseu += vu; }
            tot += v; totu += vu;
        }
        for (int i = i_lo; i < i_hi; ++i) {
            if (S.q_cnt[i] > 0) S.active[base++] = (unsigned short)i;
            else if (S.q_cnt[i] < 0) S.active_u[baseu++] = (unsigned short)i;
        }
        nact = tot; nact_u = totu;
        __syncthreads();
    }
    int cur = 0;
    // vars[0..2]: "a claim changed" flags in rotation (raised in a round, reset one round ahead)
    int f_cur = 0, f_nxt = 1;
    for (int round = 0; round <= nq + 1; ++round) {
        const int nxt = cur ^ 1;
        const uint32_t *claim_c = S.claim[cur];
        const int *head_c2 = S.head[cur];
        const unsigned short *next_c = S.next[cur];
        uint32_t *claim_n = S.claim[nxt];
        int *head_n = S.head[nxt];
        unsigned short *next_n = S.next[nxt];
        for (int b = tid; b < n; b += T) head_n[b] = -1;
        if (tid == 0) S.vars[f_nxt] = 0;
        __syncthreads();
        bool ch = false;
        for (int a = tid; a < nact; a += T) {
            const int i = S.active[a];
            const int c = S.q_cnt[i];
            uint32_t k1 = kNoClaim;
            int d2 = INT_MAX;
            // the smallest distance an accepted query with a smaller index has left on slot b (vMatchedDistance)
            auto left_on = [&](int b) -> int {
                int D = INT_MAX;
                for (int j = head_c2[b]; j >= 0; j = next_c[j] == 0xffff ? -1 : (int)next_c[j])
                    if (j < i) D = min(D, (int)(claim_c[j] >> 20));
                return D;
            };
            if (c > 0) {          // sorted by (distance, visiting order): first and second usable entry
                const unsigned long long *list = ccand + (size_t)i * kCompact;
                const uint32_t *lrow = S.lc + i * (S.lcn + 1);
                for (int e = 0; e < c; ++e) {
                    uint32_t w;
                    if (e < S.lcn) w = lrow[e];
                    else { const unsigned long long v = list[e]; w = ((uint32_t)(v >> 32) << 20) | (uint32_t)(v & 0xfffffu); }
                    const int d = (int)(w >> 20), b = (int)(w & 0xfffffu);
                    if (left_on(b) <= d) continue;
                    if (k1 == kNoClaim) k1 = w; else { d2 = d; break; }
                }
            }
            uint32_t mine = kNoClaim;
            if (k1 != kNoClaim) {
                const int d1 = (int)(k1 >> 20);
                // bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio, bestDist2 = INT_MAX when absent
                if (d1 <= TH_LOW && (float)d1 < __fmul_rn((float)d2, nnratio)) mine = k1;
            }
            claim_n[i] = mine;
            if (mine != kNoClaim) {
                const int old = atomicExch(&head_n[(int)(mine & 0xfffffu)], i);
                next_n[i] = old < 0 ? (unsigned short)0xffff : (unsigned short)old;
            }
            ch |= mine != claim_c[i];
        }
        // queries with more than 64 candidates (unsorted lists in HBM): one wavefront per query, lanes over the
        // candidates, two wave minima = smallest and second smallest usable key
        for (int u = tid >> 6; u < nact_u; u += T >> 6) {
            const int i = S.active_u[u];
            const int c = -S.q_cnt[i];
            const unsigned long long *list = cand + (size_t)i * stride;
            auto left_on = [&](int b) -> int {
                int D = INT_MAX;
                for (int j = head_c2[b]; j >= 0; j = next_c[j] == 0xffff ? -1 : (int)next_c[j])
                    if (j < i) D = min(D, (int)(claim_c[j] >> 20));
                return D;
            };
            unsigned long long m1 = ~0ull;
            for (int e = tid & 63; e < c; e += 64) {
                const unsigned long long v = list[e];
                if (left_on((int)(v & 0xfffffu)) > (int)(v >> 32)) m1 = v < m1 ? v : m1;
            }
            const unsigned long long k1v = wave_min_u64(m1);
            unsigned long long m2 = ~0ull;
            for (int e = tid & 63; e < c; e += 64) {
                const unsigned long long v = list[e];
                if (v != k1v && left_on((int)(v & 0xfffffu)) > (int)(v >> 32)) m2 = v < m2 ? v : m2;
            }
            const unsigned long long k2v = wave_min_u64(m2);
            if ((tid & 63) == 0) {
                uint32_t mine = kNoClaim;
                if (k1v != ~0ull) {
                    const int d1 = (int)(k1v >> 32), d2 = k2v == ~0ull ? INT_MAX : (int)(k2v >> 32);
                    if (d1 <= TH_LOW && (float)d1 < __fmul_rn((float)d2, nnratio)) mine = ((uint32_t)d1 << 20) | (uint32_t)(k1v & 0xfffffu);
                }
                claim_n[i] = mine;
                if (mine != kNoClaim) {
                    const int old = atomicExch(&head_n[(int)(mine & 0xfffffu)], i);
                    next_n[i] = old < 0 ? (unsigned short)0xffff : (unsigned short)old;
                }
                ch |= mine != claim_c[i];
            }
        }
        if (ch) S.vars[f_cur] = 1;
        __syncthreads();
        const int changed = S.vars[f_cur];
        cur = nxt;
        { const int t_ = f_cur; f_cur = f_nxt; f_nxt = 3 - t_ - f_nxt; }
        if (!changed) break;
    }
    // ---- outcome: a claim holds its slot unless a later query claimed the same slot (it was closer: it stole it);
    // every accepted query enters the rotation histogram, stolen or not, as the reference's rotHist does ----
    const uint32_t *claim = S.claim[cur];
    const int *head = S.head[cur];
    const unsigned short *next = S.next[cur];
    int kept = 0;
    for (int i0 = 0; i0 < nq; i0 += T) {
        const int i = i0 + tid;
        int m = -1, bin = -1;
        if (i < nq && claim[i] != kNoClaim) {
            const int b = (int)(claim[i] & 0xfffffu);
            bool stolen = false;
            for (int j = head[b]; j >= 0; j = next[j] == 0xffff ? -1 : (int)next[j]) stolen |= j > i;
            if (!stolen) m = b;
            if (check_ori) {
                bin = rot_bin(S.q_angle[i], S.t_angle[b]);
                if (bin >= 0) S.evbin[i] = (unsigned char)bin;
            }
        }
        if (i < nq) { S.q_cnt[i] = m; kept += m >= 0; }   // q_cnt is free now: vnMatches12
        wave_hist_add(S.hist, bin);
    }
    kept = wave_sum(kept);
    if ((tid & 63) == 0 && kept) atomicAdd(&S.vars[4], kept);
    __syncthreads();
    if (check_ori) {
        rank_bins_once(S.hist, S.vars + 8);
        const int ind1 = S.vars[8], ind2 = S.vars[9], ind3 = S.vars[10];
        int cull = 0;
        for (int i = tid; i < nq; i += T)
            if (rot_culled(S.evbin[i], ind1, ind2, ind3) && S.q_cnt[i] >= 0) { S.q_cnt[i] = -1; ++cull; }
        cull = wave_sum(cull);
        if ((tid & 63) == 0 && cull) atomicAdd(&S.vars[5], cull);
        __syncthreads();
    }
    for (int i = tid; i < nq; i += T) out[i] = S.q_cnt[i];
    if (tid == 0) *out_n = S.vars[4] - S.vars[5];
}

// ---- DescriptorDistance, batched (ORBmatcher.cc:1647-1663) --------------------------------
__global__ void k_distance_matrix(const uint8_t *__restrict__ a, int na, const uint8_t *__restrict__ b, int nb,
                                  int *__restrict__ dist)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= nb || i >= na) return;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(a + (size_t)i * 32);
    const uint32_t *pb = reinterpret_cast<const uint32_t *>(b + (size_t)j * 32);
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += __popc(pa[k] ^ pb[k]);
    dist[(size_t)i * nb + j] = d;
}

// ---- MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307), batched over map points ----------------
// One wavefront per map point with N observations: for every row i the lanes hold the distances d(i, j); the
// median vDists[0.5*(N-1)] of the sorted row (self distance 0 included) is the k-th smallest value, found by a
// 9-step bisection on the value range [0, 256] with ballot/popcount counting (rows longer than 64 keep their
// distances in LDS).  Smallest median wins, first index on ties (:296-300).
constexpr int kDistinctMax = 2048;

// The k-th smallest (k from 0) of one row of N distances, wave-uniform: lane j holds d0 = d(i, j) (any value above 256
// where j >= N), entries 64 and up are in srow.  Bisection on the value range [0, 256], counting with ballot / popcount.
__device__ __forceinline__ int row_kth_distance(int d0, const unsigned short *srow, int N, int k, int lane)
{
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = __popcll(__ballot(d0 <= mid));
        if (N > 64) {
            int c = 0;
            for (int j = lane + 64; j < N; j += 64) c += srow[j] <= mid;
            cnt += wave_sum(c);
        }
        if (cnt >= k + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_distinctive(const uint8_t *__restrict__ desc, const int *__restrict__ offsets,
                                                     int npoints, int *__restrict__ best)
{
    __shared__ unsigned short srow[4][kDistinctMax];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = blockIdx.x * 4 + wv;
    if (p >= npoints) return;
    const int o0 = offsets[p], N = offsets[p + 1] - o0;
    if (N <= 0) { if (lane == 0) best[p] = -1; return; }
    const uint8_t *D = desc + (size_t)o0 * 32;
    const int k = (N - 1) >> 1;   // (int)(0.5*(N-1))
    uint32_t t0[8];
    {
        const uint32_t *tp = reinterpret_cast<const uint32_t *>(D + (size_t)(lane < N ? lane : 0) * 32);
#pragma unroll
        for (int w = 0; w < 8; ++w) t0[w] = tp[w];
    }
    int bestMedian = INT_MAX, bestIdx = 0;
    for (int i = 0; i < N; ++i) {
        uint32_t di[8];
        const uint32_t *ip = reinterpret_cast<const uint32_t *>(D + (size_t)i * 32);
#pragma unroll
        for (int w = 0; w < 8; ++w) di[w] = ip[w];
        const int d0 = lane < N ? hamming256(di, t0) : 0x7fff;
        if (N > 64) {
            for (int j = lane + 64; j < N; j += 64) {
                const uint32_t *tp = reinterpret_cast<const uint32_t *>(D + (size_t)j * 32);
                uint32_t t[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) t[w] = tp[w];
                srow[wv][j] = (unsigned short)hamming256(di, t);
            }
            wave_lds_handoff();
        }
        const int lo = row_kth_distance(d0, srow[wv], N, k, lane);
        if (lo < bestMedian) { bestMedian = lo; bestIdx = i; }
        if (N > 64) wave_lds_handoff();   // the next row overwrites srow
    }
    if (lane == 0) best[p] = bestIdx;
}

// ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371) from an
// observation table over the key-frame bank: observation j of point p is key point obs_idx[o] of bank row obs_kf[o],
// o = obs_start[p] + j.  k_update_points gives a group of 16 lanes to a point with at most 16 observations, four points to
// a wavefront; longer lists go to a worklist that k_update_points_long walks with one wavefront per point.  The sum of
// the normal is taken in table order by one lane, and of several equal medians the first in table order wins.
constexpr int kUpdGroup = 16;         // lanes, and observations, of a point in k_update_points
constexpr int kUpdStage = 512;        // descriptors of a long point kept in LDS; the rest are read through their bank rows
constexpr int kUpdLongBlocks = 1024;  // grid of k_update_points_long, which loops over the worklist

struct UpdArgs {
    const float *Tcw;               // [rows][12]
    const orbhip_keypoint *keys;    // [rows][cap]
    const uint8_t *desc;            // [rows][cap][32]
    const uint8_t *kf_bad;          // [rows] or null
    const int *obs_start, *obs_kf, *obs_idx, *ref_obs;
    const float *world;             // [pcap][3]
    const uint8_t *flags;           // [pcap]
    uint8_t *point_desc;            // [pcap][32]
    float *normal, *max_dist, *min_dist;
    int *best_obs;                  // [np] or null
    uint8_t *status;                // [np]
    int *work;                      // [0] = number of long points, [1 + i] = their indices
    int cap, np, what;
};

// d = mWorldPos - Owi in float; v = normali / cv::norm(normali): the Mat times the double 1.0 / norm, element by element
__device__ __forceinline__ void upd_view_dir(const float *T, const float *X, float *d, float *v)
{
    float Ow[3];
    camera_centre(T, Ow);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = __fsub_rn(X[c], Ow[c]);
    const double inv = 1.0 / norm3d(d[0], d[1], d[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (float)(inv * (double)d[c]);
}
// mfMaxDistance / mfMinDistance (:359-368) from PC = Pos - Ow of the reference key frame and the octave of its observation
__device__ __forceinline__ void upd_depth_range(const float *pc, int level, const orbhip_camera &cam, float *mx, float *mn)
{
    const float dist = (float)norm3d(pc[0], pc[1], pc[2]);
    const float sf = level < 0 ? cam.scale_factors[0] : (level >= cam.n_levels ? 0.f : cam.scale_factors[level]);
    *mx = __fmul_rn(dist, sf);
    *mn = __fdiv_rn(*mx, cam.scale_factors[cam.n_levels - 1]);
}
// mNormalVector = normal / n (:369): the Mat times the double 1.0 / n
__device__ __forceinline__ void upd_store_normal(float *out, const float *sum, int n)
{
    const double inv = 1.0 / (double)n;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (float)(inv * (double)sum[c]);
}

__global__ __launch_bounds__(256) void k_update_points(UpdArgs A, orbhip_camera cam)
{
    __shared__ uint32_t sdesc[16][kUpdGroup][8];
    __shared__ float sdir[16][kUpdGroup][3];
    const int lane = threadIdx.x & 63, gl = lane & 15, g = threadIdx.x >> 4, gshift = lane & 48;
    const int p = blockIdx.x * 16 + g;
    const bool want_desc = (A.what & ORBHIP_UPDATE_DESCRIPTOR) != 0, want_nd = (A.what & ORBHIP_UPDATE_NORMAL_DEPTH) != 0;
    int N = 0, o0 = 0;
    if (p < A.np) {
        o0 = A.obs_start[p];
        N = A.obs_start[p + 1] - o0;
        int leave = -1;
        if (!(A.flags[p] & ORBHIP_POINT_PRESENT)) leave = ORBHIP_MAPPOINT_BAD;
        else if (N <= 0) leave = ORBHIP_MAPPOINT_NO_OBSERVATION;
        else if (N > kDistinctMax) leave = ORBHIP_MAPPOINT_TOO_MANY;
        if (leave >= 0) {
            if (gl == 0) {
                A.status[p] = (uint8_t)leave;
                if (want_desc && A.best_obs) A.best_obs[p] = -1;
            }
            N = 0;
        } else if (N > kUpdGroup) {
            if (gl == 0) A.work[1 + atomicAdd(A.work, 1)] = p;
            N = 0;
        }
    }
    // from here on every lane of the wavefront runs the same steps; a group without a point has N = 0 and stores nothing
    if (__ballot(N > 0) == 0) return;
    const bool mine = gl < N;
    int kf = 0, idx = 0;
    bool ok = false;
    if (mine) {
        kf = A.obs_kf[o0 + gl];
        idx = A.obs_idx[o0 + gl];
        ok = !(A.kf_bad && A.kf_bad[kf]);   // :265
    }
    int status = ORBHIP_MAPPOINT_UPDATED;
    if (want_desc) {
        uint32_t t0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (mine) {
            const uint32_t *tp = reinterpret_cast<const uint32_t *>(A.desc + ((size_t)kf * A.cap + idx) * 32);
#pragma unroll
            for (int w = 0; w < 8; ++w) t0[w] = tp[w];
        }
#pragma unroll
        for (int w = 0; w < 8; ++w) sdesc[g][gl][w] = t0[w];
        wave_lds_handoff();
        const uint32_t kept = (uint32_t)(__ballot(ok) >> gshift) & 0xffffu;   // vDescriptors, as a mask over the list
        const int k = (__popc(kept) - 1) >> 1;                                // (int)(0.5*(N-1))
        const int nmax = max(max(__builtin_amdgcn_readlane(N, 0), __builtin_amdgcn_readlane(N, 16)),
                             max(__builtin_amdgcn_readlane(N, 32), __builtin_amdgcn_readlane(N, 48)));
        int bestMedian = INT_MAX, bestIdx = -1;
        for (int i = 0; i < nmax; ++i) {
            uint32_t di[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) di[w] = sdesc[g][i][w];
            const int d = ok ? hamming256(di, t0) : 0x7fff;
            // the k-th smallest of the group's row: nine halvings of [0, 256], counted in the group's slice of the ballot
            int lo = 0, hi = 256;
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                const int mid = (lo + hi) >> 1;
                const int cnt = __popc((uint32_t)(__ballot(d <= mid) >> gshift) & 0xffffu);
                if (lo < hi) {
                    if (cnt >= k + 1) hi = mid; else lo = mid + 1;
                }
            }
            if (((kept >> i) & 1u) && lo < bestMedian) { bestMedian = lo; bestIdx = i; }   // :296-300
        }
        if (N > 0) {
            if (bestIdx >= 0) {
                if (gl < 8) reinterpret_cast<uint32_t *>(A.point_desc + (size_t)p * 32)[gl] = sdesc[g][bestIdx][gl];
            } else status = ORBHIP_MAPPOINT_NO_DESCRIPTOR;   // :269
            if (gl == 0 && A.best_obs) A.best_obs[p] = bestIdx;
        }
    }
    if (want_nd) {
        float d[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
        if (mine) upd_view_dir(A.Tcw + (size_t)kf * 12, A.world + (size_t)p * 3, d, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) sdir[g][gl][c] = v[c];
        wave_lds_handoff();
        if (N > 0) {
            const int r = A.ref_obs[p];
            if (r < 0 || r >= N) status = ORBHIP_MAPPOINT_BAD_REF;
            else {
                if (gl == r) {   // this lane's d is Pos - pRefKF->GetCameraCenter()
                    float mx, mn;
                    upd_depth_range(d, A.keys[(size_t)kf * A.cap + idx].octave, cam, &mx, &mn);
                    A.max_dist[p] = mx;
                    A.min_dist[p] = mn;
                }
                if (gl == 0) {
                    float sum[3] = {0.f, 0.f, 0.f};
                    for (int j = 0; j < N; ++j)
#pragma unroll
                        for (int c = 0; c < 3; ++c) sum[c] = __fadd_rn(sum[c], sdir[g][j][c]);
                    upd_store_normal(A.normal + (size_t)p * 3, sum, N);
                }
            }
        }
    }
    if (N > 0 && gl == 0) A.status[p] = (uint8_t)status;
}

// descriptor j of the kept observations of a long point: from LDS, or past kUpdStage through its bank row
__device__ __forceinline__ void upd_load_desc(const uint32_t (*sdesc)[8], const int *srow_of, const uint8_t *desc, int j,
                                              uint32_t *out)
{
    if (j < kUpdStage) {
#pragma unroll
        for (int w = 0; w < 8; ++w) out[w] = sdesc[j][w];
    } else {
        const uint32_t *tp = reinterpret_cast<const uint32_t *>(desc) + (size_t)srow_of[j] * 8;
#pragma unroll
        for (int w = 0; w < 8; ++w) out[w] = tp[w];
    }
}

__global__ __launch_bounds__(64) void k_update_points_long(UpdArgs A, orbhip_camera cam)
{
    __shared__ uint32_t sdesc[kUpdStage][8];
    __shared__ int srow_of[kDistinctMax];           // bank row * cap + key point of the kept observations
    __shared__ unsigned short spos[kDistinctMax];   // their positions in the point's list
    __shared__ unsigned short srow[kDistinctMax];   // distances of one row past lane 63
    __shared__ float sdir[64][3];
    const int lane = threadIdx.x;
    const bool want_desc = (A.what & ORBHIP_UPDATE_DESCRIPTOR) != 0, want_nd = (A.what & ORBHIP_UPDATE_NORMAL_DEPTH) != 0;
    const int count = A.work[0];
    for (int wi = blockIdx.x; wi < count; wi += gridDim.x) {
        const int p = A.work[1 + wi];
        const int o0 = A.obs_start[p], N = A.obs_start[p + 1] - o0;   // 16 < N <= kDistinctMax
        int status = ORBHIP_MAPPOINT_UPDATED;
        if (want_desc) {
            int M = 0;   // vDescriptors.size()
            for (int base = 0; base < N; base += 64) {
                const int j = base + lane;
                bool ok = false;
                int row = 0;
                if (j < N) {
                    const int kf = A.obs_kf[o0 + j];
                    ok = !(A.kf_bad && A.kf_bad[kf]);
                    row = kf * A.cap + A.obs_idx[o0 + j];
                }
                const unsigned long long mk = __ballot(ok);
                if (ok) {
                    const int pos = M + lane_prefix(mk);
                    srow_of[pos] = row;
                    spos[pos] = (unsigned short)j;
                }
                M += __popcll(mk);
            }
            wave_lds_handoff();
            const int staged = min(M, kUpdStage) * 8;
            for (int e = lane; e < staged; e += 64)
                (&sdesc[0][0])[e] = reinterpret_cast<const uint32_t *>(A.desc)[(size_t)srow_of[e >> 3] * 8 + (e & 7)];
            wave_lds_handoff();
            int bestIdx = -1;
            if (M > 0) {
                const int k = (M - 1) >> 1;
                uint32_t t0[8];
                upd_load_desc(sdesc, srow_of, A.desc, lane < M ? lane : 0, t0);
                int bestMedian = INT_MAX;
                for (int i = 0; i < M; ++i) {
                    uint32_t di[8];
                    upd_load_desc(sdesc, srow_of, A.desc, i, di);
                    const int d0 = lane < M ? hamming256(di, t0) : 0x7fff;
                    if (M > 64) {
                        for (int j = lane + 64; j < M; j += 64) {
                            uint32_t t[8];
                            upd_load_desc(sdesc, srow_of, A.desc, j, t);
                            srow[j] = (unsigned short)hamming256(di, t);
                        }
                        wave_lds_handoff();
                    }
                    const int lo = row_kth_distance(d0, srow, M, k, lane);
                    if (lo < bestMedian) { bestMedian = lo; bestIdx = i; }
                    if (M > 64) wave_lds_handoff();
                }
                if (lane < 8)
                    reinterpret_cast<uint32_t *>(A.point_desc + (size_t)p * 32)[lane] =
                        bestIdx < kUpdStage ? sdesc[bestIdx][lane]
                                            : reinterpret_cast<const uint32_t *>(A.desc)[(size_t)srow_of[bestIdx] * 8 + lane];
            } else status = ORBHIP_MAPPOINT_NO_DESCRIPTOR;
            if (lane == 0 && A.best_obs) A.best_obs[p] = bestIdx >= 0 ? (int)spos[bestIdx] : -1;
        }
        if (want_nd) {
            const int r = A.ref_obs[p];
            if (r < 0 || r >= N) status = ORBHIP_MAPPOINT_BAD_REF;
            else {
                float sum[3] = {0.f, 0.f, 0.f};
                for (int base = 0; base < N; base += 64) {
                    const int j = base + lane;
                    float d[3], v[3] = {0.f, 0.f, 0.f};
                    if (j < N) {
                        const int kf = A.obs_kf[o0 + j];
                        upd_view_dir(A.Tcw + (size_t)kf * 12, A.world + (size_t)p * 3, d, v);
                        if (j == r) {
                            float mx, mn;
                            upd_depth_range(d, A.keys[(size_t)kf * A.cap + A.obs_idx[o0 + j]].octave, cam, &mx, &mn);
                            A.max_dist[p] = mx;
                            A.min_dist[p] = mn;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) sdir[lane][c] = v[c];
                    wave_lds_handoff();
                    const int m = min(64, N - base);
                    for (int jj = 0; jj < m; ++jj)   // every lane the same sum, in table order
#pragma unroll
                        for (int c = 0; c < 3; ++c) sum[c] = __fadd_rn(sum[c], sdir[jj][c]);
                    wave_lds_handoff();
                }
                if (lane == 0) upd_store_normal(A.normal + (size_t)p * 3, sum, N);
            }
        }
        if (lane == 0) A.status[p] = (uint8_t)status;
        wave_lds_handoff();   // the next point reuses the LDS arrays
    }
}

// ---- Frame constructor glue on the device ------------------------------------------------
// Frame::AssignFeaturesToGrid (Frame.cc:230-245): mGrid[64][48] as CSR.  One workgroup per frame: keys
// (cell << 12 | index) are bitonic-sorted in LDS, which is push_back order inside every cell; cell sizes come from LDS
// atomics and an exclusive scan.
constexpr int kGridMax = 4096;
// F and the three output rows are those of the workgroup's frame already
__device__ __forceinline__ void grid_csr_body(const DevFrame &F, int *__restrict__ cell_of, int *__restrict__ cell_start,
                                              int *__restrict__ cell_items)
{
    __shared__ uint32_t key[kGridMax];
    __shared__ int cnt[kGridCells + 1];
    __shared__ int wsum[16];
    const int tid = threadIdx.x, NT = 1024;
    const int n = min(F.n, kGridMax);
    int P = 1024;
    while (P < n) P <<= 1;
    for (int c = tid; c <= kGridCells; c += NT) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < P; i += NT) {
        uint32_t k = 0xffffffffu;
        if (i < n) {
            const orbhip_keypoint kp = F.keys[i];
            const int c = grid_cell(kp.x, kp.y, F.min_x, F.min_y, F.inv_w, F.inv_h);
            cell_of[i] = c;
            if (c >= 0) { k = ((uint32_t)c << 12) | (uint32_t)i; atomicAdd(&cnt[c], 1); }
        }
        key[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t a = key[i], b = key[l];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[l] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += NT)
        if (key[i] != 0xffffffffu) cell_items[i] = (int)(key[i] & 0xfffu);
    // exclusive scan of the 3072 cell sizes: 3 per thread, wave scan, then the 16 wave totals
    const int c0 = tid * 3;
    const int v0 = cnt[c0], v1 = cnt[c0 + 1], v2 = cnt[c0 + 2];
    int incl = v0 + v1 + v2;
    const int lane = tid & 63, wv = tid >> 6;
    incl = wave_incl_scan_add(incl);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    const int excl = base + incl - (v0 + v1 + v2);
    cell_start[c0] = excl; cell_start[c0 + 1] = excl + v0; cell_start[c0 + 2] = excl + v0 + v1;
    if (tid == NT - 1) cell_start[kGridCells] = excl + v0 + v1 + v2;
}
__global__ __launch_bounds__(1024) void k_grid_csr(DevFrame F, Batch B, int *__restrict__ cell_of,
                                                   int *__restrict__ cell_start, int *__restrict__ cell_items)
{
    const int frame = blockIdx.x;
    batch_frame(F, B, frame);
    grid_csr_body(F, cell_of + (size_t)frame * B.cap, cell_start + (size_t)frame * (kGridCells + 1),
                  cell_items + (size_t)frame * B.cap);
}
// the same for the targets of orbhip_fuse_device: workgroup k builds the grid of frame row kf_index[k] into row k
__global__ __launch_bounds__(1024) void k_grid_csr_indexed(DevFrame F, const int *__restrict__ kf_index,
                                                           const int *__restrict__ n_dev, int cap, int *__restrict__ cell_of,
                                                           int *__restrict__ cell_start, int *__restrict__ cell_items)
{
    const int k = blockIdx.x;
    const size_t f = (size_t)kf_index[k];
    F.keys += f * cap;
    F.n = min(n_dev[f], cap);
    grid_csr_body(F, cell_of + (size_t)k * cap, cell_start + (size_t)k * (kGridCells + 1), cell_items + (size_t)k * cap);
}

// Frame::UndistortKeyPoints (Frame.cc:404-434) = cv::undistortPoints(mat, mat, mK, mDistCoef, Mat(), mK): OpenCV 2.4 - 3.3
// cvUndistortPoints restated from its published algorithm (double arithmetic, 5 fixed-point iterations of the inverse
// Brown model, re-projection with P = mK).  The translation unit is built with -ffp-contract=off, so every product
// and sum below rounds exactly like the C oracle's.
struct UndistortParams { double fx, fy, cx, cy, k[5]; };
__global__ void k_undistort(const orbhip_keypoint *__restrict__ keys, const int *__restrict__ n_dev, int n, int cap,
                            UndistortParams P, orbhip_keypoint *__restrict__ keys_un)
{
    const int frame = blockIdx.y;
    keys += (size_t)frame * cap; keys_un += (size_t)frame * cap;
    if (n_dev) n = min(n_dev[frame], cap);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    orbhip_keypoint kp = keys[i];
    const double ifx = 1. / P.fx, ify = 1. / P.fy;
    double x = kp.x, y = kp.y;
    const double x0 = x = (x - P.cx) * ifx;
    const double y0 = y = (y - P.cy) * ify;
    const double k0 = P.k[0], k1 = P.k[1], k2 = P.k[2], k3 = P.k[3], k4 = P.k[4];
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((0.0 * r2 + 0.0) * r2 + 0.0) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        const double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x);
        const double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = P.fx * x + 0.0 * y + P.cx;
    const double yy = 0.0 * x + P.fy * y + P.cy;
    const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
    kp.x = (float)(xx * ww);
    kp.y = (float)(yy * ww);
    keys_un[i] = kp;
}

// Frame::ComputeStereoFromRGBD (Frame.cc:643-664)
__global__ void k_stereo_from_rgbd(const orbhip_keypoint *__restrict__ keys, const orbhip_keypoint *__restrict__ keys_un,
                                   const int *__restrict__ n_dev, int n, int cap, const float *__restrict__ depth, int rows,
                                   int cols, int stride, size_t frame_stride, float mbf, float *__restrict__ u_right,
                                   float *__restrict__ depth_out)
{
    const int frame = blockIdx.y;
    keys += (size_t)frame * cap; keys_un += (size_t)frame * cap;
    u_right += (size_t)frame * cap; depth_out += (size_t)frame * cap;
    depth += (size_t)frame * frame_stride;
    if (n_dev) n = min(n_dev[frame], cap);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = (int)keys[i].y, u = (int)keys[i].x;      // Mat::at<float>(int,int) with float arguments: truncation
    float d = 0.f;
    if (v >= 0 && v < rows && u >= 0 && u < cols) d = depth[(size_t)v * stride + u];
    float ur = -1.0f, dp = -1.0f;
    if (d > 0) { dp = d; ur = __fsub_rn(keys_un[i].x, __fdiv_rn(mbf, d)); }
    u_right[i] = ur;
    depth_out[i] = dp;
}

// The same on the depth image as the sensor delivers it: Tracking::GrabImageRGBD's
//     if ((fabs(mDepthMapFactor - 1.0f) > 1e-5) || imDepth.type() != CV_32F) imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor);
// (src/Tracking.cc:227-228) is applied to the one sample a keypoint reads instead of to rows x cols pixels.  Equal bit
// for bit to convert-then-sample: convertTo with a zero shift computes saturate_cast<float>(src * alpha + 0) per pixel
// in float; a 16-bit integer is exact in float, and adding +0 to the rounded product -- or fusing it into an fma, whose
// single rounding is then the rounding of the product alone -- leaves fl(src * alpha).  (A product of -0 would become
// +0; neither passes d > 0.)  `convert`: that condition, evaluated once on the host.
template <typename T>
__global__ void k_stereo_from_rgbd_raw(const orbhip_keypoint *__restrict__ keys, const orbhip_keypoint *__restrict__ keys_un,
                                       const int *__restrict__ n_dev, int cap, const T *__restrict__ depth, int rows, int cols,
                                       int stride, size_t frame_stride, float factor, int convert, float mbf,
                                       float *__restrict__ u_right, float *__restrict__ depth_out)
{
    const int frame = blockIdx.y;
    keys += (size_t)frame * cap; keys_un += (size_t)frame * cap;
    u_right += (size_t)frame * cap; depth_out += (size_t)frame * cap;
    depth += (size_t)frame * frame_stride;
    const int n = min(n_dev[frame], cap);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = (int)keys[i].y, u = (int)keys[i].x;      // Mat::at<float>(int,int) with float arguments: truncation
    float d = 0.f;
    if (v >= 0 && v < rows && u >= 0 && u < cols) {
        d = (float)depth[(size_t)v * stride + u];
        if (convert) d = __fmul_rn(d, factor);
    }
    float ur = -1.0f, dp = -1.0f;
    if (d > 0) { dp = d; ur = __fsub_rn(keys_un[i].x, __fdiv_rn(mbf, d)); }
    u_right[i] = ur;
    depth_out[i] = dp;
}

// ---- Frame::ComputeStereoMatches (Frame.cc:466-640) -----------------------------------------
// ---------------------------------------------------------------------------
// Projection prologues (include/orbhip.h "projection prologues on the device"): one thread per map point.  Every
// float operation that feeds a comparison is written out un-contracted, in the order DESIGN.md section 3 states.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float dot3_row(const float *r, float x, float y, float z, float t)
{
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r[0], x), __fmul_rn(r[1], y)), __fmul_rn(r[2], z)), t);
}

// fdlibm log in IEEE double, separate operations, one rounding to float (the deterministic logf of DESIGN.md section 3)
__device__ __forceinline__ float det_logf(float xf)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    if (!(xf > 0.0f)) return xf == 0.0f ? -INFINITY : NAN;
    if (isinf(xf)) return xf;
    double x = (double)xf;
    unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    int hx = (int)(bits >> 32);
    int k = (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int i = (hx + 0x95f64) & 0x100000;
    bits = ((unsigned long long)(unsigned)(hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xffffffffull);
    x = __longlong_as_double((long long)bits);
    k += i >> 20;
    const double f = __dsub_rn(x, 1.0);
    const double s = __ddiv_rn(f, __dadd_rn(2.0, f));
    const double dk = (double)k;
    const double z = __dmul_rn(s, s);
    const double w = __dmul_rn(z, z);
    const double t1 = __dmul_rn(w, __dadd_rn(Lg2, __dmul_rn(w, __dadd_rn(Lg4, __dmul_rn(w, Lg6)))));
    const double t2 = __dmul_rn(z, __dadd_rn(Lg1, __dmul_rn(w, __dadd_rn(Lg3, __dmul_rn(w, __dadd_rn(Lg5, __dmul_rn(w, Lg7)))))));
    const double R = __dadd_rn(t2, t1);
    const double hfsq = __dmul_rn(__dmul_rn(0.5, f), f);
    const double r = __dsub_rn(__dmul_rn(dk, ln2_hi),
                               __dsub_rn(__dsub_rn(hfsq, __dadd_rn(__dmul_rn(s, __dadd_rn(hfsq, R)), __dmul_rn(dk, ln2_lo))), f));
    return (float)r;
}

struct ProjBatch {
    const float *Tcw, *Tlw;            // [pairs][12]
    const orbhip_keypoint *keys;       // [frames][cap]
    const int *n_dev;                  // [frames]
    const float *world;                // [frames][cap][3]
    const uint8_t *flags;              // [frames][cap]
    orbhip_query *q;                   // [pairs][cap]
    int *nq;                           // [pairs] or null
    int cap, l0, ls;
};

// src/ORBmatcher.cc:1339-1390
__device__ __forceinline__ void project_last_frame_body(const ProjBatch &B, const orbhip_camera &cam, const float th, const int mono,
                                                        const int pair, const int i)
{
    const size_t fl = (size_t)(B.l0 + pair * B.ls);
    const int n = min(B.n_dev[fl], B.cap);
    if (i == 0 && B.nq) B.nq[pair] = n;
    if (i >= n) return;
    const float *Tcw = B.Tcw + (size_t)pair * 12, *Tlw = B.Tlw + (size_t)pair * 12;
    orbhip_query Q;
    Q.valid = 0; Q.u = 0; Q.v = 0; Q.radius = 0; Q.min_level = 0; Q.max_level = 0; Q.ur = 0; Q.level_aux = 0; Q.angle = 0; Q.observed = 0;
    orbhip_query *dst = B.q + (size_t)pair * B.cap + i;
    const unsigned fg = B.flags[fl * B.cap + i];
    if (fg & ORBHIP_POINT_PRESENT) {
        // twc = -Rcw.t()*tcw; tlc = Rlw*twc+tlw (:1342-1347); a dozen flops, recomputed per thread
        float twc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            twc[c] = -__fadd_rn(__fadd_rn(__fmul_rn(Tcw[c], Tcw[3]), __fmul_rn(Tcw[4 + c], Tcw[7])), __fmul_rn(Tcw[8 + c], Tcw[11]));
        const float tlc_z = dot3_row(Tlw + 8, twc[0], twc[1], twc[2], Tlw[11]);
        const bool forward = tlc_z > cam.mb && !mono, backward = -tlc_z > cam.mb && !mono;
        const float *X = B.world + (fl * B.cap + i) * 3;
        const float x = X[0], y = X[1], z = X[2];
        const float xc = dot3_row(Tcw, x, y, z, Tcw[3]);
        const float yc = dot3_row(Tcw + 4, x, y, z, Tcw[7]);
        const float zc = dot3_row(Tcw + 8, x, y, z, Tcw[11]);
        const float invzc = (float)__ddiv_rn(1.0, (double)zc);
        if (!(invzc < 0)) {
            const float u = __fadd_rn(__fmul_rn(__fmul_rn(cam.fx, xc), invzc), cam.cx);
            const float v = __fadd_rn(__fmul_rn(__fmul_rn(cam.fy, yc), invzc), cam.cy);
            if (!(u < cam.min_x || u > cam.max_x) && !(v < cam.min_y || v > cam.max_y)) {
                const orbhip_keypoint kp = B.keys[fl * B.cap + i];
                const int o = kp.octave;
                Q.valid = 1; Q.u = u; Q.v = v;
                Q.radius = __fmul_rn(th, cam.scale_factors[min(max(o, 0), ORBHIP_MAX_LEVELS - 1)]);
                if (forward) { Q.min_level = o; Q.max_level = -1; }
                else if (backward) { Q.min_level = 0; Q.max_level = o; }
                else { Q.min_level = o - 1; Q.max_level = o + 1; }
                Q.ur = __fsub_rn(u, __fmul_rn(cam.mbf, invzc));
                Q.level_aux = o;
                Q.angle = kp.angle;
                Q.observed = (fg & ORBHIP_POINT_OBSERVED) ? 1 : 0;
            }
        }
    }
    *dst = Q;
}
__global__ __launch_bounds__(256) void k_project_last_frame(ProjBatch B, orbhip_camera cam, float th, int mono)
{
    project_last_frame_body(B, cam, th, mono, (int)blockIdx.y, (int)(blockIdx.x * 256 + threadIdx.x));
}
// TrackWithMotionModel's matching step: the projection prologue and the CSR grid of the current frames do not depend on
// each other, so they share one launch: per pair one workgroup builds the grid, `npb` workgroups project
__global__ __launch_bounds__(256) void k_grid_build_project(DevFrame F, int *__restrict__ cell_start, GridRec *__restrict__ rec,
                                                            uint4 *__restrict__ rdesc, float *__restrict__ rur, Batch B,
                                                            ProjBatch P, orbhip_camera cam, float th, int mono, int npb)
{
    const int pair = (int)blockIdx.x / (npb + 1), role = (int)blockIdx.x - pair * (npb + 1);
    if (role == 0) grid_build_body(F, cell_start, rec, rdesc, rur, B, pair);
    else project_last_frame_body(P, cam, th, mono, pair, (role - 1) * 256 + (int)threadIdx.x);
}
struct ProjLaunch { ProjBatch P; orbhip_camera cam; float th; int mono; };

struct FrustumBatch {
    const float *Tcw;                       // [frames][12]
    const int *np_dev;                      // [frames]
    const float *world, *normal;            // [frames][pcap][3]
    const float *max_dist, *min_dist;       // [frames][pcap]
    const uint8_t *flags;                   // [frames][pcap]
    orbhip_query *q;                        // [frames][pcap]
    float *view_cos;                        // [frames][pcap] or null
    int pcap;
};

// src/Frame.cc:269-325, src/MapPoint.cc:400-418, src/ORBmatcher.cc:52-69, :131-137
__global__ __launch_bounds__(256) void k_frustum_queries(FrustumBatch B, orbhip_camera cam, float cos_limit, float th)
{
    const int fr = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(B.np_dev[fr], B.pcap);
    if (i >= n) return;
    const size_t e = (size_t)fr * B.pcap + i;
    const float *Tcw = B.Tcw + (size_t)fr * 12;
    orbhip_query Q;
    Q.valid = 0; Q.u = 0; Q.v = 0; Q.radius = 0; Q.min_level = 0; Q.max_level = 0; Q.ur = 0; Q.level_aux = 0; Q.angle = 0; Q.observed = 0;
    float vc = 0.0f;
    const unsigned fg = B.flags[e];
    do {
        if (!(fg & ORBHIP_POINT_PRESENT)) break;
        float Ow[3];   // mOw = -mRcw.t()*mtcw
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Ow[c] = -__fadd_rn(__fadd_rn(__fmul_rn(Tcw[c], Tcw[3]), __fmul_rn(Tcw[4 + c], Tcw[7])), __fmul_rn(Tcw[8 + c], Tcw[11]));
        const float *P = B.world + e * 3;
        const float px = P[0], py = P[1], pz = P[2];
        const float PcX = dot3_row(Tcw, px, py, pz, Tcw[3]);
        const float PcY = dot3_row(Tcw + 4, px, py, pz, Tcw[7]);
        const float PcZ = dot3_row(Tcw + 8, px, py, pz, Tcw[11]);
        if (PcZ < 0.0f) break;
        const float invz = __fdiv_rn(1.0f, PcZ);
        const float u = __fadd_rn(__fmul_rn(__fmul_rn(cam.fx, PcX), invz), cam.cx);
        const float v = __fadd_rn(__fmul_rn(__fmul_rn(cam.fy, PcY), invz), cam.cy);
        if (u < cam.min_x || u > cam.max_x) break;
        if (v < cam.min_y || v > cam.max_y) break;
        const float md = B.max_dist[e];
        const float maxDistance = __fmul_rn(1.2f, md), minDistance = __fmul_rn(0.8f, B.min_dist[e]);
        const float ox = __fsub_rn(px, Ow[0]), oy = __fsub_rn(py, Ow[1]), oz = __fsub_rn(pz, Ow[2]);
        const double ss = __dadd_rn(__dadd_rn(__dmul_rn((double)ox, (double)ox), __dmul_rn((double)oy, (double)oy)), __dmul_rn((double)oz, (double)oz));
        const float dist = (float)__dsqrt_rn(ss);
        if (dist < minDistance || dist > maxDistance) break;
        const float *Pn = B.normal + e * 3;
        const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)ox, (double)Pn[0]), __dmul_rn((double)oy, (double)Pn[1])), __dmul_rn((double)oz, (double)Pn[2]));
        const float viewCos = (float)__ddiv_rn(dot, (double)dist);
        if (viewCos < cos_limit) break;
        const float ratio = __fdiv_rn(md, dist);
        const float fl = ceilf(__fdiv_rn(det_logf(ratio), cam.log_scale_factor));
        int nScale = fl >= (float)cam.n_levels ? cam.n_levels - 1 : (fl < 0 ? 0 : (int)fl);
        if (!(fl == fl)) nScale = 0;
        float r = (double)viewCos > 0.998 ? 2.5f : 4.0f;
        if (th != 1.0f) r = __fmul_rn(r, th);
        Q.valid = 1; Q.u = u; Q.v = v;
        Q.radius = __fmul_rn(r, cam.scale_factors[min(max(nScale, 0), ORBHIP_MAX_LEVELS - 1)]);
        Q.min_level = nScale - 1; Q.max_level = nScale;
        Q.ur = __fsub_rn(u, __fmul_rn(cam.mbf, invz));
        Q.level_aux = nScale;
        Q.observed = (fg & ORBHIP_POINT_OBSERVED) ? 1 : 0;
        vc = viewCos;
    } while (0);
    B.q[e] = Q;
    if (B.view_cos) B.view_cos[e] = vc;
}

// SearchForInitialization, device-resident form: queries = level-0 keypoints of F1 searched around vbPrevMatched
// (src/ORBmatcher.cc:418-425); `reset` first sets vbPrevMatched[i] = F1.mvKeysUn[i].pt (src/Tracking.cc:578-580).
__global__ __launch_bounds__(256) void k_init_queries(const orbhip_keypoint *__restrict__ keys, const int *__restrict__ n_dev,
                                                      int cap, int f0, int fs, float *__restrict__ prev, int reset,
                                                      float window, orbhip_query *__restrict__ q, int *__restrict__ nq)
{
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const size_t f1 = (size_t)(f0 + pair * fs);
    const int n = min(n_dev[f1], cap);
    if (i == 0) nq[pair] = n;
    if (i >= n) return;
    const orbhip_keypoint kp = keys[f1 * cap + i];
    float *pm = prev + ((size_t)pair * cap + i) * 2;
    if (reset) { pm[0] = kp.x; pm[1] = kp.y; }
    orbhip_query Q;
    Q.valid = kp.octave > 0 ? 0 : 1;
    Q.u = pm[0]; Q.v = pm[1];
    Q.radius = window;
    Q.min_level = kp.octave; Q.max_level = kp.octave;
    Q.ur = 0; Q.level_aux = 0; Q.angle = kp.angle; Q.observed = 0;
    q[(size_t)pair * cap + i] = Q;
}

// vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt for every match (src/ORBmatcher.cc:515-517)
__global__ __launch_bounds__(256) void k_init_update_prev(const orbhip_keypoint *__restrict__ keys, int cap, int f0, int fs,
                                                          const int *__restrict__ nq, const int *__restrict__ m12,
                                                          float *__restrict__ prev)
{
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq[pair]) return;
    const int j = m12[(size_t)pair * cap + i];
    if (j < 0) return;
    const orbhip_keypoint kp = keys[(size_t)(f0 + pair * fs) * cap + j];
    float *pm = prev + ((size_t)pair * cap + i) * 2;
    pm[0] = kp.x; pm[1] = kp.y;
}

// Prologue of ORBmatcher::Fuse (both overloads) and of one direction of SearchBySim3: see include/orbhip.h
// (orbhip_keyframe_queries).  One thread per map point.
struct KfQueryArgs {
    const float *T1, *T2;                   // 12 floats each (T2 unused in mode 0)
    const float *world, *normal, *max_dist, *min_dist;
    const uint8_t *flags;
    orbhip_query *q;
    int n, mode, double_invz;
};
// the record of map point i: the one statement of this float sequence, shared by k_keyframe_queries and k_fuse_batch
__device__ __forceinline__ orbhip_query keyframe_query(const KfQueryArgs &A, const orbhip_camera &cam, const float th, const int i)
{
    orbhip_query Q;
    Q.valid = 0; Q.u = 0; Q.v = 0; Q.radius = 0; Q.min_level = 0; Q.max_level = 0; Q.ur = 0; Q.level_aux = 0; Q.angle = 0; Q.observed = 0;
    do {
        if (!(A.flags[i] & ORBHIP_POINT_PRESENT)) break;
        const float *T1 = A.T1;
        const float *P = A.world + (size_t)i * 3;
        const float px = P[0], py = P[1], pz = P[2];
        float X = dot3_row(T1, px, py, pz, T1[3]);
        float Y = dot3_row(T1 + 4, px, py, pz, T1[7]);
        float Z = dot3_row(T1 + 8, px, py, pz, T1[11]);
        if (A.mode == 1) {
            const float *T2 = A.T2;
            const float x1 = X, y1 = Y, z1 = Z;
            X = dot3_row(T2, x1, y1, z1, T2[3]);
            Y = dot3_row(T2 + 4, x1, y1, z1, T2[7]);
            Z = dot3_row(T2 + 8, x1, y1, z1, T2[11]);
        }
        if (Z < 0.0f) break;
        const float invz = A.double_invz ? (float)__ddiv_rn(1.0, (double)Z) : __fdiv_rn(1.0f, Z);
        const float x = __fmul_rn(X, invz), y = __fmul_rn(Y, invz);
        const float u = __fadd_rn(__fmul_rn(cam.fx, x), cam.cx), v = __fadd_rn(__fmul_rn(cam.fy, y), cam.cy);
        if (!(u >= cam.min_x && u < cam.max_x && v >= cam.min_y && v < cam.max_y)) break;   // KeyFrame::IsInImage
        const float md = A.max_dist[i];
        const float maxDistance = __fmul_rn(1.2f, md), minDistance = __fmul_rn(0.8f, A.min_dist[i]);
        float dist3D;
        if (A.mode == 0) {
            float Ow[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                Ow[c] = -__fadd_rn(__fadd_rn(__fmul_rn(T1[c], T1[3]), __fmul_rn(T1[4 + c], T1[7])), __fmul_rn(T1[8 + c], T1[11]));
            const float ox = __fsub_rn(px, Ow[0]), oy = __fsub_rn(py, Ow[1]), oz = __fsub_rn(pz, Ow[2]);
            const double ss = __dadd_rn(__dadd_rn(__dmul_rn((double)ox, (double)ox), __dmul_rn((double)oy, (double)oy)), __dmul_rn((double)oz, (double)oz));
            dist3D = (float)__dsqrt_rn(ss);
            if (dist3D < minDistance || dist3D > maxDistance) break;
            const float *Pn = A.normal + (size_t)i * 3;
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)ox, (double)Pn[0]), __dmul_rn((double)oy, (double)Pn[1])), __dmul_rn((double)oz, (double)Pn[2]));
            if (dot < __dmul_rn(0.5, (double)dist3D)) break;
        } else {
            const double ss = __dadd_rn(__dadd_rn(__dmul_rn((double)X, (double)X), __dmul_rn((double)Y, (double)Y)), __dmul_rn((double)Z, (double)Z));
            dist3D = (float)__dsqrt_rn(ss);
            if (dist3D < minDistance || dist3D > maxDistance) break;
        }
        const float fl = ceilf(__fdiv_rn(det_logf(__fdiv_rn(md, dist3D)), cam.log_scale_factor));
        int lvl = fl >= (float)cam.n_levels ? cam.n_levels - 1 : (fl < 0 ? 0 : (int)fl);
        if (!(fl == fl)) lvl = 0;
        Q.valid = 1; Q.u = u; Q.v = v;
        Q.radius = __fmul_rn(th, cam.scale_factors[min(max(lvl, 0), ORBHIP_MAX_LEVELS - 1)]);
        Q.min_level = lvl - 1; Q.max_level = lvl;
        Q.ur = A.mode == 0 ? __fsub_rn(u, __fmul_rn(cam.mbf, invz)) : 0.0f;
        Q.level_aux = lvl;
    } while (0);
    return Q;
}
__global__ __launch_bounds__(256) void k_keyframe_queries(KfQueryArgs A, orbhip_camera cam, float th)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    A.q[i] = keyframe_query(A, cam, th, i);
}

// ORBmatcher::Fuse up to the decision for K key frames in one launch (LocalMapping::SearchInNeighbors,
// src/LocalMapping.cc:454-515; LoopClosing::SearchAndFuse, src/LoopClosing.cc:585-610): blockIdx.y = target k = frame row
// kf_index[k] of the extractor-layout arrays, blockIdx.x = 256 of the shared map points.
//   1. one thread per point: keyframe_query (the prologue of orbhip_fuse).  The records stay in registers; they reach
//      memory only when the caller asks for them (A.q).
//   2. the wavefront's valid records are packed to its low lanes with one ds_permute per field (a stable partition of
//      the 64 lanes, so every lane is a destination exactly once); no LDS allocation, no barrier.
//   3. LPQ lanes per query (64 / LPQ queries of the wavefront at a time) walk the window's cells in the order of
//      Frame::GetFeaturesInArea (src/Frame.cc:332-378): for every column ix the cells (ix, nMinCellY..nMaxCellY) are
//      consecutive in c = ix*48 + iy, so their key points are ONE run of cell_items.  Candidate p of the run goes to
//      lane p % LPQ: |dx|,|dy| < r, level window, chi-square gate, 256-bit Hamming distance: the test of fuse_candidate,
//      spelled out in the loop (through the helper this kernel measured 2 % slower than the parent).
//      The key is distance << 32 | position in cell_items << 12 | index: cell_items is sorted by (cell, index), so the
//      position orders candidates as cell << 20 | index does and the group minimum is the reference's first minimum.
struct FuseBatchArgs {
    const int *kf_index;                    // [K]
    const float *Tcw;                       // [K][12]
    const orbhip_keypoint *keys;            // [..][cap]
    const uint8_t *desc;                    // [..][cap][32]
    const int *n_dev;                       // [..]
    const float *u_right;                   // [..][cap] or null
    const int *cell_start, *cell_items;     // [..][3073], [..][cap]
    const float *world, *normal, *max_dist, *min_dist;
    const uint8_t *point_desc, *flags;      // [np][32], [K][pcap]
    int *best_idx, *best_dist;              // [K][pcap]
    orbhip_query *q;                        // [K][pcap] or null
    int cap, np, pcap;
    int sim3_form;                          // the Scw overload (src/ORBmatcher.cc:977-1100): invz = 1.0/z in double, no chi-square gate
    int csr_by_target;                      // CSR rows are indexed by k (built by this call), not by the frame row
    float min_x, min_y, inv_w, inv_h;
};

template <int LPQ>
__global__ __launch_bounds__(256) void k_fuse_batch(FuseBatchArgs A, orbhip_camera cam, float th, SigmaTab sig)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t f = (size_t)A.kf_index[k], orow = (size_t)k * A.pcap;
    orbhip_query Q;
    Q.valid = 0; Q.u = 0; Q.v = 0; Q.radius = 0; Q.min_level = 0; Q.ur = 0;
    if (i < A.np) {
        KfQueryArgs P;
        P.T1 = A.Tcw + (size_t)k * 12; P.T2 = nullptr;
        P.world = A.world; P.normal = A.normal; P.max_dist = A.max_dist; P.min_dist = A.min_dist;
        P.flags = A.flags + orow; P.q = nullptr; P.n = A.np; P.mode = 0; P.double_invz = A.sim3_form;
        Q = keyframe_query(P, cam, th, i);
        if (A.q) A.q[orow + i] = Q;
        if (!Q.valid) { A.best_idx[orow + i] = -1; A.best_dist[orow + i] = 256; }
    }
    const bool valid = i < A.np && Q.valid != 0;
    const unsigned long long vmask = __ballot(valid);
    const int nvalid = __popcll(vmask);
    if (nvalid == 0) return;                          // wave-uniform
    // stable partition: valid lanes to 0 .. nvalid-1 in lane order, the others behind them
    const int before = __popcll(vmask & ((1ull << lane) - 1ull));
    const int dest = (valid ? before : nvalid + (lane - before)) << 2;
    const float cu = __int_as_float(__builtin_amdgcn_ds_permute(dest, __float_as_int(Q.u)));
    const float cv = __int_as_float(__builtin_amdgcn_ds_permute(dest, __float_as_int(Q.v)));
    const float cr = __int_as_float(__builtin_amdgcn_ds_permute(dest, __float_as_int(Q.radius)));
    const float cur = __int_as_float(__builtin_amdgcn_ds_permute(dest, __float_as_int(Q.ur)));
    const int cml = __builtin_amdgcn_ds_permute(dest, Q.min_level);
    const int cqi = __builtin_amdgcn_ds_permute(dest, i);

    const int n = min(A.n_dev[f], A.cap);
    const orbhip_keypoint *keys = A.keys + f * A.cap;
    const uint8_t *desc = A.desc + f * A.cap * 32;
    const float *u_right = A.u_right ? A.u_right + f * A.cap : nullptr;
    const size_t crow = A.csr_by_target ? (size_t)k : f;
    const int *cs = A.cell_start + crow * (kGridCells + 1);
    const int *items = A.cell_items + crow * A.cap;

    constexpr int G = 64 / LPQ;
    const int sub = lane & (LPQ - 1), grp = lane / LPQ;
    for (int s0 = 0; s0 < nvalid; s0 += G) {          // wave-uniform trip count
        const int slot = s0 + grp;
        const bool active = slot < nvalid;
        const int src = active ? slot : 0;
        const float x = __shfl(cu, src), y = __shfl(cv, src), r = __shfl(cr, src), qur = __shfl(cur, src);
        const int min_level = __shfl(cml, src), qi = __shfl(cqi, src);
        unsigned long long best = ~0ull;
        if (active) {
            const CellWindow W = cell_window(x, y, r, A.min_x, A.min_y, A.inv_w, A.inv_h);
            if (!W.empty()) {
                uint32_t qd[8];
                const uint4 *qp = reinterpret_cast<const uint4 *>(A.point_desc + (size_t)qi * 32);
                const uint4 q0 = qp[0], q1 = qp[1];
                qd[0] = q0.x; qd[1] = q0.y; qd[2] = q0.z; qd[3] = q0.w; qd[4] = q1.x; qd[5] = q1.y; qd[6] = q1.z; qd[7] = q1.w;
                for (int ix = W.x0; ix <= W.x1; ++ix) {
                    const int c0 = ix * GRID_ROWS;
                    const int pb = max(cs[c0 + W.y0], 0), pe = min(cs[c0 + W.y1 + 1], A.cap);
                    for (int p = pb + sub; p < pe; p += LPQ) {
                        const int j = items[p];
                        if ((unsigned)j >= (unsigned)n) continue;   // never for a grid of these key points
                        // fuse_candidate, kept inline here (see 3. above); change the two together
                        const orbhip_keypoint kp = keys[j];
                        if (!(fabsf(__fsub_rn(kp.x, x)) < r && fabsf(__fsub_rn(kp.y, y)) < r)) continue;
                        if (kp.octave < min_level || kp.octave > min_level + 1) continue;   // kpLevel<pred-1 || kpLevel>pred
                        const float ex = __fsub_rn(x, kp.x), ey = __fsub_rn(y, kp.y);
                        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                        if (!A.sim3_form) {                 // the loop of the Scw overload (:1062-1079) has no chi-square gate
                            const float kpr = u_right ? u_right[j] : -1.0f;
                            const float is2 = sig.inv_sigma2[kp.octave & (ORBHIP_MAX_LEVELS - 1)];
                            if (kpr >= 0) {
                                const float er = __fsub_rn(qur, kpr);
                                e2 = __fadd_rn(e2, __fmul_rn(er, er));
                                if ((double)__fmul_rn(e2, is2) > 7.8) continue;
                            } else if ((double)__fmul_rn(e2, is2) > 5.99) continue;
                        }
                        const uint4 *tp = reinterpret_cast<const uint4 *>(desc + (size_t)j * 32);
                        const int d = hamming256(qd, tp[0], tp[1]);
                        const unsigned long long key = ((unsigned long long)d << 32) | ((uint32_t)p << 12) | (uint32_t)j;
                        best = key < best ? key : best;
                    }
                }
            }
        }
        best = group_min_u64<LPQ>(best);
        if (active && sub == 0) {
            A.best_idx[orow + qi] = best == ~0ull ? -1 : (int)(best & 0xfffu);
            A.best_dist[orow + qi] = best == ~0ull ? 256 : (int)(best >> 32);
        }
    }
}

struct StereoGeom {
    int nlevels, nrows;
    const uint8_t *left[ORBHIP_MAX_LEVELS], *right[ORBHIP_MAX_LEVELS];
    int pitch_l[ORBHIP_MAX_LEVELS], pitch_r[ORBHIP_MAX_LEVELS], cols_r[ORBHIP_MAX_LEVELS];
    float sf[ORBHIP_MAX_LEVELS], isf[ORBHIP_MAX_LEVELS];
    float mbf, mb;
};

// rows a right keypoint's band can reach from floor(y): ceil(2 * largest scale factor) + 1
static int stereo_row_reach(const StereoGeom &G)
{
    float mx = 0.f;
    for (int l = 0; l < G.nlevels; ++l) mx = std::max(mx, G.sf[l]);
    return (int)ceilf(2.0f * mx) + 1;
}
struct StereoScales;
static StereoScales stereo_scales(const StereoGeom &G);
// Batched stereo: pair p uses frame l0 + p*ls of the left arrays/pyramids and r0 + p*rs of the right ones.
struct StereoBatch {
    const int *n_l, *n_r;   // per-frame keypoint counts on the device
    int l0, ls, r0, rs;     // frame index mapping
    int cap;                // keypoint stride per frame
    unsigned fb_l, fb_r;    // pyramid bytes per frame of the two extractor handles
};

// Right keypoints bucketed by image row (counting sort on floor(y)): a left keypoint's candidates -- the right keypoints
// whose row band [floor(y - r), ceil(y + r)], r = 2 * scale[octave] (Frame.cc:483-493) contains its row -- all lie within
// R = ceil(2 * largest scale) + 1 rows of it, i.e. in ONE contiguous range of the sorted order, instead of anywhere among
// the nr right keypoints.  One workgroup per pair; rowstart[nrows + 1], order[nr] (order inside a row is irrelevant: the
// match is the minimum of (distance, index) keys).
constexpr int kStereoRowsMax = 4096;
struct StereoScales { float sf[ORBHIP_MAX_LEVELS]; };
__global__ __launch_bounds__(256) void k_stereo_sort(const orbhip_keypoint *__restrict__ kr, int nr, int nrows,
                                                     int *__restrict__ rowstart, int4 *__restrict__ order, StereoBatch B,
                                                     StereoScales SF)
{
    __shared__ int s_cnt[kStereoRowsMax];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, pair = blockIdx.x, fr = B.r0 + pair * B.rs;
    kr += (size_t)fr * B.cap;
    rowstart += (size_t)pair * (nrows + 1);
    order += (size_t)pair * B.cap;
    if (B.n_r) nr = min(B.n_r[fr], B.cap);   // always set; the test is kept because dropping it costs the kernel an SGPR
    for (int r = tid; r < nrows; r += 256) s_cnt[r] = 0;
    __syncthreads();
    for (int i = tid; i < nr; i += 256) atomicAdd(&s_cnt[min(max((int)floorf(kr[i].y), 0), nrows - 1)], 1);
    __syncthreads();
    const int per = (nrows + 255) / 256, r0 = tid * per, r1 = min(r0 + per, nrows);
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += s_cnt[r];
    const int incl = wave_incl_scan_add(sum);
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) base += s_wave[w];
    for (int r = r0; r < r1; ++r) { const int c = s_cnt[r]; s_cnt[r] = base; rowstart[r] = base; base += c; }
    if (tid == 255) rowstart[nrows] = base;
    __syncthreads();
    // the sorted order holds RECORDS, not indices: everything k_stereo_match needs to gate a candidate -- x, the row band
    // [floor(y - r), ceil(y + r)] with r = 2 * scale[octave] (same float operations as Frame.cc:483-493; clamped to
    // [0, 4095], which no comparison against an image row can tell), the octave, the index -- in one 16-byte load instead
    // of an index load followed by a dependent 28-byte keypoint load and a 15-way select of the scale per candidate
    for (int i = tid; i < nr; i += 256) {
        const orbhip_keypoint k = kr[i];
        float sfo = SF.sf[0];
#pragma unroll
        for (int l = 1; l < ORBHIP_MAX_LEVELS; ++l) sfo = k.octave == l ? SF.sf[l] : sfo;
        const float r = __fmul_rn(2.0f, sfo);
        const int minr = min(max((int)floorf(__fsub_rn(k.y, r)), 0), 4095), maxr = min(max((int)ceilf(__fadd_rn(k.y, r)), 0), 4095);
        const int pos = atomicAdd(&s_cnt[min(max((int)floorf(k.y), 0), nrows - 1)], 1);
        order[pos] = make_int4(__float_as_int(k.x), minr | (maxr << 12) | ((k.octave & 15) << 24), i, 0);
    }
}

__global__ __launch_bounds__(256) void k_stereo_match(const orbhip_keypoint *__restrict__ kl,
                                                      const uint8_t *__restrict__ dl,
                                                      const orbhip_keypoint *__restrict__ kr,
                                                      const uint8_t *__restrict__ dr,
                                                      const int *__restrict__ rowstart, const int4 *__restrict__ order, int R,
                                                      StereoGeom G,
                                                      float *__restrict__ uRight, float *__restrict__ depth,
                                                      int *__restrict__ sad, StereoBatch B)
{
    const int lane = threadIdx.x & 63;
    size_t pyr_off_l, pyr_off_r;   // this pair's frames inside the two pyramid batches
    int nl, nr;
    {
        const int pair = blockIdx.y, fl = B.l0 + pair * B.ls, fr = B.r0 + pair * B.rs;
        pyr_off_l = (size_t)fl * B.fb_l; pyr_off_r = (size_t)fr * B.fb_r;
        kl += (size_t)fl * B.cap; dl += (size_t)fl * B.cap * 32;
        kr += (size_t)fr * B.cap; dr += (size_t)fr * B.cap * 32;
        if (rowstart) { rowstart += (size_t)pair * (G.nrows + 1); order += (size_t)pair * B.cap; }
        uRight += (size_t)pair * B.cap; depth += (size_t)pair * B.cap; sad += (size_t)pair * B.cap;
        nl = min(B.n_l[fl], B.cap);
        nr = min(B.n_r[fr], B.cap);
    }
    const int iL = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (iL >= nl) return;
    if (lane == 0) { uRight[iL] = -1.0f; depth[iL] = -1.0f; sad[iL] = -1; }
    const orbhip_keypoint kpL = kl[iL];
    // one keypoint per wavefront: the level is wave-uniform, and saying so keeps the per-level tables of G in scalar
    // registers (a lane-indexed by-value array would be copied to scratch by every wave)
    const int levelL = __builtin_amdgcn_readfirstlane(kpL.octave);
    const float vL = kpL.y, uL = kpL.x;
    const int row = (int)vL;
    if (row < 0 || row >= G.nrows) return;
    const float minZ = G.mb, minD = 0.f;
    const float maxD = __fdiv_rn(G.mbf, minZ);
    const float minU = __fsub_rn(uL, maxD), maxU = __fsub_rn(uL, minD);
    if (maxU < 0) return;
    uint32_t qd[8];
    const uint32_t *qp = reinterpret_cast<const uint32_t *>(dl + (size_t)iL * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) qd[i] = qp[i];
    // The kernel is a chain of dependent memory round trips (keypoint -> row range -> candidate records -> descriptors ->
    // right patch), so what does not depend on the match leaves early: the left 11x11 patch of the sub-pixel refinement
    // (:555-592; it needs the left keypoint alone and lies inside the padded plane for every keypoint) is requested here.
    const float scaleFactor = G.isf[levelL];
    const float scaleduL = roundf(__fmul_rn(kpL.x, scaleFactor));
    const float scaledvL = roundf(__fmul_rn(kpL.y, scaleFactor));
    const int w = 5, L = 5;
    const uint8_t *imL = G.left[levelL] + pyr_off_l, *imR = G.right[levelL] + pyr_off_r;
    const int stL = G.pitch_l[levelL], stR = G.pitch_r[levelL];
    const int cu = (int)scaleduL, cv = (int)scaledvL;
    // Both patches travel as byte-unaligned DWORD loads into a per-wavefront LDS tile -- one load instruction for the left
    // 11 x 12-byte window, two for the right 11 x 24-byte one (11 x 21 needed: 11 columns x 11 shifts) -- and are read
    // from there byte by byte: the 35 byte-gather loads per lane this replaces (2 + 11 x 3) kept the texture addresser,
    // not the ALUs, busy (67 us per 64 pairs with any amount of arithmetic removed).
    __shared__ uint32_t s_patch[4][11 * 3 + 11 * 6 + 1];
    uint32_t *sl = s_patch[threadIdx.x >> 6], *sr = sl + 11 * 3;
    uint32_t lw = 0;
    if (lane < 33) {
        const int prow = (lane * 43) >> 7, pc = lane - prow * 3;     // lane / 3 for lane < 33
        __builtin_memcpy(&lw, imL + (ptrdiff_t)(cv - w + prow) * stL + (cu - w) + 4 * pc, 4);
    }
    // each lane owns up to 2 of the 121 patch pixels
    int dyv[2], dxv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int p = lane + 64 * t;
        dyv[t] = p / 11 - w; dxv[t] = p % 11 - w;
    }
    // best right keypoint on this row: smallest (dist, iR) with dist < TH_HIGH (:522-549).  Candidates: the rows within R
    // of this one in the row-sorted order (all right keypoints when there is no order)
    // key = distance << 20 | index (distances <= 256, indices < 2^20: checked on the host): the wave minimum is six
    // v_min_u32 on the DPP path instead of six 64-bit compare-select steps
    uint32_t best = (uint32_t)TH_HIGH << 20;
    float bestx = 0.f;               // x of this lane's best candidate (travels with the key: no keypoint reload after the minimum)
    int jb = 0, je = nr;
    if (rowstart) { jb = rowstart[max(row - R, 0)]; je = rowstart[min(row + R + 1, G.nrows)]; }
    for (int j0 = jb; j0 < je; j0 += 64) {
        const int j = j0 + lane;
        if (j < je) {
            int iR, minr, maxr, octR;
            float xR;
            if (rowstart) {
                const int4 rc = order[j];
                xR = __int_as_float(rc.x); minr = rc.y & 4095; maxr = (rc.y >> 12) & 4095; octR = rc.y >> 24; iR = rc.z;
            } else {
                iR = j;
                const orbhip_keypoint kpR = kr[iR];
                float sfo = G.sf[0];   // scale of the right keypoint's level, by selects (a lane-indexed read would put G into scratch)
#pragma unroll
                for (int l = 1; l < ORBHIP_MAX_LEVELS; ++l) sfo = kpR.octave == l ? G.sf[l] : sfo;
                const float r = __fmul_rn(2.0f, sfo);
                minr = (int)floorf(__fsub_rn(kpR.y, r)); maxr = (int)ceilf(__fadd_rn(kpR.y, r));
                octR = kpR.octave; xR = kpR.x;
            }
            if (row >= minr && row <= maxr && !(octR < levelL - 1 || octR > levelL + 1) && xR >= minU && xR <= maxU) {
                const uint32_t *tp = reinterpret_cast<const uint32_t *>(dr + (size_t)iR * 32);
                uint32_t td[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) td[i] = tp[i];
                const uint32_t key = ((uint32_t)hamming256(qd, td) << 20) | (uint32_t)iR;
                if (key < best) { best = key; bestx = xR; }
            }
        }
    }
    const uint32_t mine_key = best;
    best = (uint32_t)wave_min((int)best);          // keys are < 2^31: the signed minimum is the unsigned one
    const int bestDist = (int)(best >> 20);
    const int thOrbDist = (TH_HIGH + TH_LOW) / 2;
    if (!(bestDist < thOrbDist)) return;
    // sub-pixel refinement by 11x11 SAD over 11 shifts at the keypoint's level (:555-592); x of the winner from the lane that holds it
    const unsigned long long owner = __ballot(mine_key == best);
    const float uR0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bestx), __ffsll((long long)owner) - 1));
    const float scaleduR0 = roundf(__fmul_rn(uR0, scaleFactor));
    const float iniu = __fsub_rn(__fadd_rn(scaleduR0, (float)L), (float)w);
    const float endu = __fadd_rn(__fadd_rn(__fadd_rn(scaleduR0, (float)L), (float)w), 1.0f);
    if (iniu < 0 || endu >= (float)G.cols_r[levelL]) return;
    const int cr = (int)scaleduR0;
    // stage the two windows: right window = rows cv-5 .. cv+5, bytes cr-10 .. cr+13 (columns beyond cr+10 are never read;
    // they lie inside the padded plane: cr + 11 < cols was just checked)
    if (lane < 33) sl[lane] = lw;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int idx = lane + 64 * t;
        if (idx < 66) {
            const int prow = (idx * 43) >> 8, pc = idx - prow * 6;     // idx / 6 for idx < 66
            uint32_t rw;
            __builtin_memcpy(&rw, imR + (ptrdiff_t)(cv - w + prow) * stR + (cr - 2 * w) + 4 * pc, 4);
            sr[idx] = rw;
        }
    }
    wave_lds_handoff();                       // the two windows are read across lanes
    const uint8_t *bl = reinterpret_cast<const uint8_t *>(sl), *br = reinterpret_cast<const uint8_t *>(sr);
    const int cL = bl[5 * 12 + 5];
    int pl[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) pl[t] = lane + 64 * t < 121 ? (int)bl[(dyv[t] + w) * 12 + dxv[t] + w] - cL : 0;
    // SAD of the 11 shifts; a shift's total is at most 121 * 510 < 2^16, so two shifts share one wave sum
    int accs[11];
#pragma unroll
    for (int s = 0; s < 11; ++s) {
        const int incR = s - L;
        const int cR = br[5 * 24 + 2 * w + incR];
        int acc = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            int p = lane + 64 * t;
            if (p < 121) {
                int b = (int)br[(dyv[t] + w) * 24 + 2 * w + incR + dxv[t]] - cR;
                acc += abs(pl[t] - b);
            }
        }
        accs[s] = acc;
    }
    int dists[11];
#pragma unroll
    for (int s = 0; s < 10; s += 2) {
        const uint32_t two = (uint32_t)wave_sum(accs[s] | (accs[s + 1] << 16));
        dists[s] = (int)(two & 0xffffu); dists[s + 1] = (int)(two >> 16);
    }
    dists[10] = wave_sum(accs[10]);
    int bestD = INT_MAX, bestincR = 0;
#pragma unroll
    for (int s = 0; s < 11; ++s) if (dists[s] < bestD) { bestD = dists[s]; bestincR = s - L; }
    if (bestincR == -L || bestincR == L) return;
    float dist1 = 0, dist2 = 0, dist3 = 0;
#pragma unroll
    for (int s = 1; s < 10; ++s) if (s == L + bestincR) { dist1 = (float)dists[s - 1]; dist2 = (float)dists[s]; dist3 = (float)dists[s + 1]; }
    const float deltaR = __fdiv_rn(__fsub_rn(dist1, dist3),
                                   __fmul_rn(2.0f, __fsub_rn(__fadd_rn(dist1, dist3), __fmul_rn(2.0f, dist2))));
    if (deltaR < -1 || deltaR > 1) return;
    float bestuR = __fmul_rn(G.sf[levelL], __fadd_rn(__fadd_rn(scaleduR0, (float)bestincR), deltaR));
    float disparity = __fsub_rn(uL, bestuR);
    if (disparity >= minD && disparity < maxD) {
        if (disparity <= 0) {
            disparity = 0.01f;                              // float(0.01)
            bestuR = (float)((double)uL - 0.01);            // float - double literal
        }
        if (lane == 0) {
            depth[iL] = __fdiv_rn(G.mbf, disparity);
            uRight[iL] = bestuR;
            sad[iL] = bestD;
        }
    }
}

static StereoScales stereo_scales(const StereoGeom &G)
{
    StereoScales S;
    for (int l = 0; l < ORBHIP_MAX_LEVELS; ++l) S.sf[l] = G.sf[l < G.nlevels ? l : 0];
    return S;
}

// median-based outlier cull (:626-639): thDist = 1.5f*1.4f*median of the SAD list sorted by
// (dist, iL); entries with dist >= thDist are removed.
__global__ __launch_bounds__(256) void k_stereo_cull(const int *__restrict__ sad, float *__restrict__ uRight,
                                                     float *__restrict__ depth, int *__restrict__ out_n, StereoBatch B)
{
    __shared__ int s_nd, s_med, s_cnt;
    const int tid = threadIdx.x;
    int nl;
    {
        const int pair = blockIdx.x;
        sad += (size_t)pair * B.cap; uRight += (size_t)pair * B.cap; depth += (size_t)pair * B.cap;
        out_n += pair;
        nl = min(B.n_l[B.l0 + pair * B.ls], B.cap);
    }
    if (tid == 0) { s_nd = 0; s_med = 0; s_cnt = 0; }
    __syncthreads();
    int local = 0;
    for (int i = tid; i < nl; i += 256) local += sad[i] >= 0;
    atomicAdd(&s_nd, local);
    __syncthreads();
    const int nd = s_nd;
    if (nd == 0) { if (tid == 0) *out_n = 0; return; }
    const int target = nd / 2;
    // median = the (nd/2)-th smallest valid SAD (src/Frame.cc:628-630 sorts the (SAD, index) pairs and takes the middle
    // one; only its value is used).  One wavefront finds it by bisection on the value: count(d <= mid) over an LDS copy
    // of the list with a DPP wave sum per probe -- 16 probes, no barrier; the O(n^2) rank count this replaces took
    // 130 us per 64 pairs.  Lists longer than the LDS copy are read from HBM.
    __shared__ int s_sad[kResolveMax];
    const bool in_lds = nl <= kResolveMax;
    if (in_lds) for (int i = tid; i < nl; i += 256) s_sad[i] = sad[i];
    __syncthreads();
    // The values are L1 norms of two 11 x 11 byte windows, each minus its centre pixel: <= 11 * 11 * 510 < 2^16.  Two-level
    // radix select over all 256 threads: histogram of the high bytes, the bin that holds rank `target` (smallest v with
    // count(d <= v) > target), then the histogram of the low bytes inside that bin -- four barriers instead of 16
    // dependent bisection probes by one wavefront (26 -> 9 us per 64 pairs).
    __shared__ int s_hist[256];
    __shared__ int s_bin, s_rank;
    int rank = target, value = 0;
#pragma unroll 1
    for (int level = 0; level < 2; ++level) {
        s_hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < nl; i += 256) {
            const int d = in_lds ? s_sad[i] : sad[i];
            if (d < 0) continue;
            if (level == 0) atomicAdd(&s_hist[d >> 8], 1);
            else if ((d >> 8) == value) atomicAdd(&s_hist[d & 255], 1);
        }
        __syncthreads();
        if (tid < 64) {
            const int h0 = s_hist[4 * tid], h1 = s_hist[4 * tid + 1], h2 = s_hist[4 * tid + 2], h3 = s_hist[4 * tid + 3];
            const int sum = h0 + h1 + h2 + h3, incl = wave_incl_scan_add(sum);
            const unsigned long long over = __ballot(incl > rank);       // non-empty: the total count exceeds the rank
            if (tid == __ffsll((long long)over) - 1) {
                int c = incl - sum, bin = 4 * tid;                        // first bin of this lane whose running count passes the rank
                if (c + h0 > rank) { }
                else if (c + h0 + h1 > rank) { c += h0; bin += 1; }
                else if (c + h0 + h1 + h2 > rank) { c += h0 + h1; bin += 2; }
                else { c += h0 + h1 + h2; bin += 3; }
                s_bin = bin; s_rank = rank - c;
            }
        }
        __syncthreads();
        value = level == 0 ? s_bin : (value << 8) | s_bin;
        rank = s_rank;
        __syncthreads();
    }
    if (tid == 0) s_med = value;
    __syncthreads();
    const float median = (float)s_med;
    const float thDist = __fmul_rn(1.5f * 1.4f, median);
    int kept = 0;
    for (int i = tid; i < nl; i += 256) {
        const int d = sad[i];
        if (d < 0) continue;
        if (!((float)d < thDist)) { uRight[i] = -1; depth[i] = -1; }
        else kept++;
    }
    atomicAdd(&s_cnt, kept);
    __syncthreads();
    if (tid == 0) *out_n = s_cnt;
}

// ---- Seeding stereo / RGB-D map points: Tracking::UpdateLastFrame (src/Tracking.cc:812-864), CreateNewKeyFrame
// (:1073-1133), StereoInitialization (:523-538), all through Frame::UnprojectStereo (src/Frame.cc:666-680) ------------
// One workgroup per frame.  The keypoints with a positive depth are compacted in index order (vDepthIdx before the sort);
// mode CLOSEST sorts them by (z, i): for z > 0 the float's bit pattern is monotone as an unsigned integer, so the 64-bit
// key bits(z) << 32 | i sorted as an integer is std::sort's order on pair<float,int> (a total order: +inf last, no ties).
// The walk with its stop rule (:833-864) visits the first min(n_valid, max(101, c + 1)) sorted entries, c = the number of
// entries that do not satisfy z > mThDepth: nPoints is j + 1 after entry j, so the loop breaks at the first j >= 100 whose
// z exceeds the threshold, which in sorted order is j = max(100, c), and that entry is still processed.
// LDS: 32 KB of keys + 4 KB of created marks.
constexpr int kSeedMax = 4096;
struct SeedBatch {
    const float *Tcw;                  // [frames][12]
    const orbhip_keypoint *keys;       // [..][cap], frame k0 + f*ks
    const int *n_dev;                  // [..], frame k0 + f*ks
    const float *depth;                // [frames][cap]
    float *world;                      // [frames][cap][3] in/out
    uint8_t *flags;                    // [frames][cap] in/out
    int *order;                        // [frames][cap] or null
    uint8_t *created;                  // [frames][cap] or null
    int *counts;                       // [frames][3]
    int cap, k0, ks;
};

__device__ __forceinline__ void seed_compare_exchange(unsigned long long *key, int t, int j, int k)
{
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const unsigned long long a = key[i], b = key[l];
    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[l] = a; }
}

__global__ __launch_bounds__(1024) void k_seed_stereo_points(SeedBatch B, float fx, float fy, float cx, float cy, float th_depth,
                                                             int mode, int created_flags)
{
    __shared__ unsigned long long key[kSeedMax];
    __shared__ uint8_t made[kSeedMax];
    __shared__ int wsum[16];
    __shared__ int s_close, s_created;
    int unit, f;
    xcd_remap(unit, f);
    const int tid = threadIdx.x, NT = 1024, lane = tid & 63, wv = tid >> 6;
    const size_t kf = (size_t)(B.k0 + f * B.ks);
    const int n = max(min(min(B.n_dev[kf], B.cap), kSeedMax), 0);
    const orbhip_keypoint *keys = B.keys + kf * B.cap;
    const float *depth = B.depth + (size_t)f * B.cap;
    float *world = B.world + (size_t)f * B.cap * 3;
    uint8_t *flags = B.flags + (size_t)f * B.cap;
    if (tid == 0) { s_close = 0; s_created = 0; }
    // compaction in index order: thread t owns keypoints 4t .. 4t+3
    float z[4];
    int cnt = 0, close = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = 4 * tid + e;
        z[e] = i < n ? depth[i] : 0.f;
        const bool ok = z[e] > 0.f;                  // drops NaN, -1 and 0 (:818-822)
        cnt += ok;
        close += ok && !(z[e] > th_depth);
        made[i] = 0;
    }
    const int incl = wave_incl_scan_add(cnt);
    if (lane == 63) wsum[wv] = incl;
    close = wave_sum(close);
    __syncthreads();
    if (lane == 0 && close) atomicAdd(&s_close, close);
    int pos = incl - cnt, n_valid = 0;
    for (int w = 0; w < 16; ++w) {
        const int s = wsum[w];
        if (w < wv) pos += s;
        n_valid += s;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (z[e] > 0.f) key[pos++] = ((unsigned long long)__float_as_uint(z[e]) << 32) | (uint32_t)(4 * tid + e);
    int P = 2;
    if (mode == ORBHIP_SEED_CLOSEST) {
        while (P < n_valid) P <<= 1;
        for (int i = n_valid + tid; i < P; i += NT) key[i] = ~0ull;
    }
    __syncthreads();
    int n_visit = n_valid;
    if (mode == ORBHIP_SEED_CLOSEST) {
        // bitonic sort of P keys, one compare-exchange per pair index t.  Pairs 64c .. 64c+63 of a stride <= 64 touch keys
        // 128c .. 128c+127 only: one wavefront takes those strides of its chunks without a workgroup barrier.
        const int half = P >> 1;
        for (int k = 2; k <= P; k <<= 1) {
            int j = k >> 1;
            for (; j > 64; j >>= 1) {
                for (int t = tid; t < half; t += NT) seed_compare_exchange(key, t, j, k);
                __syncthreads();
            }
            for (int c = wv; c * 64 < half; c += 16) {
                const int t = c * 64 + lane;
                for (int jj = j; jj > 0; jj >>= 1) {
                    if (t < half) seed_compare_exchange(key, t, jj, k);
                    wave_lds_handoff();
                }
            }
            __syncthreads();
        }
        n_visit = min(n_valid, max(101, s_close + 1));
    }
    // mRwc = mRcw^T, mOw = -mRcw^T * mtcw (src/Frame.cc:258-264); a dozen flops, recomputed per thread
    const float *T = B.Tcw + (size_t)f * 12;
    float Ow[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        Ow[c] = -__fadd_rn(__fadd_rn(__fmul_rn(T[c], T[3]), __fmul_rn(T[4 + c], T[7])), __fmul_rn(T[8 + c], T[11]));
    const float invfx = __fdiv_rn(1.0f, fx), invfy = __fdiv_rn(1.0f, fy);      // src/Frame.cc:108-109
    int *order = B.order ? B.order + (size_t)f * B.cap : nullptr;
    int made_cnt = 0;
    for (int j = tid; j < n_visit; j += NT) {
        const unsigned long long kk = key[j];
        const int i = (int)(uint32_t)kk;
        const float zz = __uint_as_float((uint32_t)(kk >> 32));
        if (order) order[j] = i;
        bool create = mode == ORBHIP_SEED_ALL;
        if (!create) {
            const unsigned fg = flags[i];          // :839-845: no map point, or one nobody observes
            create = !(fg & ORBHIP_POINT_PRESENT) || !(fg & ORBHIP_POINT_OBSERVED);
        }
        if (create) {
            const orbhip_keypoint kp = keys[i];
            float X[3];
            unproject_stereo(T, Ow, kp.x, kp.y, zz, cx, cy, invfx, invfy, X);
#pragma unroll
            for (int r = 0; r < 3; ++r) world[(size_t)i * 3 + r] = X[r];
            flags[i] = (uint8_t)created_flags;
            made[i] = 1;
            ++made_cnt;
        }
    }
    made_cnt = wave_sum(made_cnt);
    if (lane == 0 && made_cnt) atomicAdd(&s_created, made_cnt);
    __syncthreads();
    if (B.created) {
        uint8_t *created = B.created + (size_t)f * B.cap;
        for (int i = tid; i < n; i += NT) created[i] = made[i];
    }
    if (tid == 0) {
        int *counts = B.counts + (size_t)f * 3;
        counts[0] = n_valid; counts[1] = n_visit; counts[2] = s_created;
    }
}

// Tracking::NeedNewKeyFrame's close-point counts (src/Tracking.cc:1006-1015): one workgroup per frame
__global__ __launch_bounds__(256) void k_count_close_points(const float *__restrict__ depth, const uint8_t *__restrict__ flags,
                                                            const int *__restrict__ n_dev, int cap, float th_depth,
                                                            int *__restrict__ counts)
{
    __shared__ int s_cnt[2];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(n_dev[f], cap);
    depth += (size_t)f * cap; flags += (size_t)f * cap;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    int tracked = 0, other = 0;
    for (int i = tid; i < n; i += 256) {
        const float z = depth[i];
        if (z > 0.f && z < th_depth) {
            if (flags[i] & ORBHIP_POINT_PRESENT) ++tracked; else ++other;
        }
    }
    tracked = wave_sum(tracked); other = wave_sum(other);
    if ((tid & 63) == 0) { if (tracked) atomicAdd(&s_cnt[0], tracked); if (other) atomicAdd(&s_cnt[1], other); }
    __syncthreads();
    if (tid < 2) counts[(size_t)f * 2 + tid] = s_cnt[tid];
}

}  // namespace orbhip

// =============================================================================================
using namespace orbhip;

struct orbhip_matcher {
    int device = 0;
    hipStream_t stream = nullptr;       // stream every launch goes to
    hipStream_t own_stream = nullptr;   // created with the handle
    // grow-only device scratch
    void *buf[30] = {};
    size_t cap[30] = {};
    bool lds_attr_set = false, bow_attr_set = false;
#ifdef ORBHIP_DEVTOOLS
    int window_lanes = 0;               // development build: lanes per query of k_window_search forced to 16 / 64 (0: the rule)
    bool resolve_stamps = false;        // development build: k_resolve_par<false> runs its stamped instantiation
#endif
    // pinned host staging: all inputs of a call travel in one DMA, all outputs in one
    uint8_t *h_stage = nullptr; size_t h_stage_bytes = 0;
    uint8_t *h_out = nullptr; size_t h_out_bytes = 0;
    void *h_eg = nullptr;               // pinned: the state record of the essential-graph optimisation, read once per trial
    int eg_counters[2] = {0, 0};        // synchronisations and launches of the last essential-graph call
    void *h_gba = nullptr;              // pinned: the state record of global bundle adjustment, read once per trial
    int gba_counters[2] = {0, 0};       // synchronisations and launches of the last global-bundle-adjustment call
    // Sim3 RANSAC: the iteration limit per correspondence count, [sim3_cap + 1], rebuilt when a parameter changes
    std::vector<int> sim3_limit;
    double sim3_prob = 0.0;
    int sim3_min_inliers = 0, sim3_max_its = 0, sim3_cap = -1;
    // PnP RANSAC: the adjusted (min inliers, limit) per correspondence count, [pnp_cap + 1][2], rebuilt when a parameter changes
    std::vector<int> pnp_tab;
    orbhip_pnp_params pnp_params = {0.0, 0, 0, 0, 0.f, 0.f};
    int pnp_cap = -1;
};

static int scratch(orbhip_matcher *m, int slot, size_t bytes, void **out)
{
    if (bytes < 256) bytes = 256;
    if (bytes > m->cap[slot]) {
        ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
        (void)hipFree(m->buf[slot]);
        m->buf[slot] = nullptr; m->cap[slot] = 0;
        ORBHIP_HIP_CHECK(hipMalloc(&m->buf[slot], bytes));
        m->cap[slot] = bytes;
    }
    *out = m->buf[slot];
    return ORBHIP_OK;
}

// Test hook (include/orbhip.h): every byte a later call could find in the handle's workspaces becomes `byte`.  The device
// slots are filled on the handle's stream, the pinned buffers once it drained.  The two slots that cache a host-built table
// (S_SIM3LIM, S_PNPTAB) lose their keys, so the next setup call uploads the table again.
int orbhip_matcher_fill_scratch(orbhip_matcher *m, int byte, unsigned long long *bytes_filled)
{
    if (!m || byte < 0 || byte > 255) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    unsigned long long total = 0;
    for (size_t i = 0; i < sizeof(m->buf) / sizeof(m->buf[0]); ++i) {
        if (!m->buf[i]) continue;
        ORBHIP_HIP_CHECK(hipMemsetAsync(m->buf[i], byte, m->cap[i], m->stream));
        total += m->cap[i];
    }
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->h_stage) { memset(m->h_stage, byte, m->h_stage_bytes); total += m->h_stage_bytes; }
    if (m->h_out) { memset(m->h_out, byte, m->h_out_bytes); total += m->h_out_bytes; }
    if (m->h_eg) { memset(m->h_eg, byte, sizeof(EgState)); total += sizeof(EgState); }
    if (m->h_gba) { memset(m->h_gba, byte, sizeof(LbaState)); total += sizeof(LbaState); }
    m->sim3_cap = -1;
    m->pnp_cap = -1;
    if (bytes_filled) *bytes_filled = total;
    return ORBHIP_OK;
}

// ---- the host side of the frame grid ---------------------------------------------------------------------------------
// Frame::ComputeImageBounds / mfGridElement{Width,Height}Inv (src/Frame.cc:99-100) from a camera's bounds
struct GridInv { float w, h; };
static GridInv grid_inv(const orbhip_camera *cam)
{
    return {(float)GRID_COLS / (cam->max_x - cam->min_x), (float)GRID_ROWS / (cam->max_y - cam->min_y)};
}
// the train frame of a device call: n = capacity of a row (Batch::n_dev holds the counts), or 0 where only keys are read
static DevFrame dev_frame(int n, const void *d_kps, const void *d_desc, const void *d_u_right, float min_x, float min_y,
                          float inv_w, float inv_h)
{
    return {n, (const orbhip_keypoint *)d_kps, (const uint8_t *)d_desc, (const float *)d_u_right, min_x, min_y, inv_w, inv_h};
}
// the train frame of a host call: keys, descriptors and u_right go into the staging buffer, in this order
static DevFrame dev_frame(const orbhip_frame_view *f, Stage &st)
{
    const size_t n = (size_t)f->n;
    const orbhip_keypoint *keys = st.put(f->keys, n);
    const uint8_t *desc = st.put(f->desc, n * 32);
    return {f->n, keys, desc, f->u_right ? st.put(f->u_right, n) : nullptr, f->min_x, f->min_y, f->grid_inv_w, f->grid_inv_h};
}
// mvInvLevelSigma2 of the first n_levels levels (null: no table, every entry 0)
static SigmaTab sigma_tab(const float *inv_level_sigma2, int n_levels)
{
    SigmaTab sig;
    memset(&sig, 0, sizeof(sig));
    if (inv_level_sigma2) for (int l = 0; l < std::min(n_levels, ORBHIP_MAX_LEVELS); ++l) sig.inv_sigma2[l] = inv_level_sigma2[l];
    return sig;
}
// the optimisers' copy of it: every level of the table, 0 past the camera's
static void fill_inv_sigma2(float (&inv)[ORBHIP_MAX_LEVELS], const orbhip_camera *cam, const float *inv_level_sigma2)
{
    for (int l = 0; l < ORBHIP_MAX_LEVELS; ++l) inv[l] = l < cam->n_levels ? inv_level_sigma2[l] : 0.f;
}
// the optimisers' camera: thHuber of the mono and stereo edges from their chi-square values, a float widened
static PoCam po_cam(const orbhip_camera *cam, double chi2_mono, double chi2_stereo)
{
    return {(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->mbf,
            (double)(float)std::sqrt(chi2_mono), (double)(float)std::sqrt(chi2_stereo)};
}

enum { S_KEYS = 0, S_DESC, S_UR, S_ORD, S_Q, S_QDESC, S_CAND, S_CNT, S_TAKEN, S_OUT, S_QKEYS, S_MISC, S_STATE, S_CSR, S_CCAND, S_TRI, S_UPD, S_LMAP, S_COVIS, S_CULL, S_SIM3, S_SIM3LIM, S_SIM3SOLV, S_PNP, S_PNPTAB, S_PNPSOLV, S_LBA, S_EG, S_GBA, S_GBAAPPLY, S_NSLOTS };
static_assert(S_NSLOTS == sizeof(orbhip_matcher::buf) / sizeof(void *), "one scratch buffer per slot");

// The buffers of a staging image of `total` bytes: the pinned one and S_MISC, grown when too small.  Waits for the
// stream first, because the previous call's copy may still read the pinned buffer.
static int stage_begin(orbhip_matcher *m, size_t total, Stage *st)
{
    total = al256(total);
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));   // previous call's staging is free
    if (total + 256 > m->h_stage_bytes) {
        if (m->h_stage) (void)hipHostFree(m->h_stage);
        m->h_stage = nullptr; m->h_stage_bytes = 0;
        ORBHIP_HIP_CHECK(hipHostMalloc((void **)&m->h_stage, total + 256, hipHostMallocDefault));
        m->h_stage_bytes = total + 256;
    }
    void *d;
    int rc = scratch(m, S_MISC, total + 256, &d);
    if (rc) return rc;
    *st = Stage();
    st->h = m->h_stage; st->d = (uint8_t *)d;
    return ORBHIP_OK;
}
static int stage_commit(orbhip_matcher *m, Stage *st)
{
    ORBHIP_HIP_CHECK(hipMemcpyAsync(st->d, st->h, st->off, hipMemcpyHostToDevice, m->stream));
    return ORBHIP_OK;
}
// a zeroed stand-in for an empty in/out array: a piece the kernels are handed but, with no element, never index
template <class T> static T *stage_zeros(Stage &st, size_t count)
{
    return st.fill<T>(count, [=](T *h) { memset(h, 0, count * sizeof(T)); });
}
// The staging image of a host-form call (orbhip_stage.h): `pieces` states what is staged, once.  stage_send sizes the
// buffers from a measuring pass over it, runs it for real and sends the image in one copy.
template <class F> static int stage_send(orbhip_matcher *m, Stage *st, F &&pieces)
{
    bool out_overflow;
    const size_t total = stage_measure(pieces, &out_overflow);
    if (out_overflow) { set_error("matcher: a call records more than %d outputs", (int)Stage::kMaxOut); return ORBHIP_E_CAPACITY; }
    if (int rc = stage_begin(m, total, st)) return rc;
    pieces(*st);
    return stage_commit(m, st);
}
// The outputs of a call, `bytes` at d, in one copy to the pinned out-buffer: *h = its host address once the stream drained
static int read_back(orbhip_matcher *m, const void *d, size_t bytes, const uint8_t **h)
{
    ORBHIP_HIP_CHECK(hipGetLastError());
    if (bytes > m->h_out_bytes) {
        if (m->h_out) (void)hipHostFree(m->h_out);
        m->h_out = nullptr; m->h_out_bytes = 0;
        ORBHIP_HIP_CHECK(hipHostMalloc((void **)&m->h_out, bytes, hipHostMallocDefault));
        m->h_out_bytes = bytes;
    }
    ORBHIP_HIP_CHECK(hipMemcpyAsync(m->h_out, d, bytes, hipMemcpyDeviceToHost, m->stream));
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
    *h = m->h_out;
    return ORBHIP_OK;
}

// The recorded outputs of a call (Stage::back / out / inout) in one copy, each then to its host array
static int stage_fetch(orbhip_matcher *m, Stage *st)
{
    const uint8_t *h;
    if (int rc = read_back(m, st->d + st->out_begin(), st->out_end() - st->out_begin(), &h)) return rc;
    st->scatter(h);
    return ORBHIP_OK;
}

static int ensure_resolve_attr(orbhip_matcher *m)
{
    if (!m->lds_attr_set) {   // > 64 KB of dynamic LDS needs the opt-in attribute (per device)
        ORBHIP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve_par<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             kResolveLdsBudget));
        ORBHIP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve_init), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             kResolveLdsBudget));
#ifdef ORBHIP_DEVTOOLS
        ORBHIP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_resolve_par<false, true>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kResolveLdsBudget));
#endif
        m->lds_attr_set = true;
    }
    return ORBHIP_OK;
}

// SearchForInitialization's state always fits the LDS budget within the kResolveMax limit of its entry points
static_assert(init_state_bytes(kResolveMax, kResolveMax, 0) <= (size_t)kResolveLdsBudget, "k_resolve_init state exceeds LDS");

// launch of the parallel resolve, sized by the batch's capacities: LDS state up to kResolveMax train keypoints / queries,
// HBM state beyond
static int launch_resolve_par(orbhip_matcher *m, int pairs, int mode, const DevFrame &D, const orbhip_query *d_q,
                              const unsigned long long *d_cand, const unsigned long long *d_ccand, const int *d_cnt, int stride,
                              const uint8_t *d_taken, float nnratio, int check_ori, int *d_out, int *d_out_n, const Batch &B,
                              int th_accept, int all_block)
{
    if (B.cap <= kResolveMax && B.qcap <= kResolveMax) {
        // the list heads go to LDS when the budget allows
        const int lcn = resolve_par_bytes((size_t)B.cap, (size_t)B.qcap, kResolveHead) <= (size_t)kResolveLdsBudget ? kResolveHead : 0;
#ifdef ORBHIP_DEVTOOLS
        if (m->resolve_stamps) {
            hipLaunchKernelGGL((k_resolve_par<false, true>), dim3(pairs), dim3(1024),
                               resolve_par_bytes((size_t)B.cap, (size_t)B.qcap, (size_t)lcn), m->stream, mode, D, d_q, B.qcap, d_cand, d_ccand,
                               d_cnt, stride, d_taken, nnratio, check_ori, d_out, d_out_n, B, th_accept, all_block,
                               (unsigned char *)nullptr, (size_t)0, lcn);
            return ORBHIP_OK;
        }
#endif
        hipLaunchKernelGGL(k_resolve_par<false>, dim3(pairs), dim3(1024), resolve_par_bytes((size_t)B.cap, (size_t)B.qcap, (size_t)lcn),
                           m->stream, mode, D, d_q, B.qcap, d_cand, d_ccand, d_cnt, stride, d_taken, nnratio, check_ori, d_out, d_out_n, B,
                           th_accept, all_block, (unsigned char *)nullptr, (size_t)0, lcn);
    } else {
        const size_t per = al256(resolve_par_bytes((size_t)B.cap, (size_t)B.qcap));
        void *p;
        int rc = scratch(m, S_STATE, per * (size_t)pairs, &p);
        if (rc) return rc;
        hipLaunchKernelGGL(k_resolve_par<true>, dim3(pairs), dim3(1024), 0, m->stream, mode, D, d_q, B.qcap, d_cand, d_ccand, d_cnt,
                           stride, d_taken, nnratio, check_ori, d_out, d_out_n, B, th_accept, all_block, (unsigned char *)p, per, 0);
    }
    return ORBHIP_OK;
}

// The windowed searches, `pairs` pairs of batch B (D.n = B.cap): CSR grid of the train frames (the projection prologue
// rides in that launch when `proj` is given), the cell-window search, then the resolve -- k_resolve_par for modes 0 / 1
// (SearchByProjection overloads), k_resolve_init for mode 2 (SearchForInitialization, query keypoints d_qkeys).
// Modes 0 / 1 only: d_taken (slots blocked on entry, nullable), th_accept (acceptance distance of mode 0), all_block
// (every accepted match blocks its slot, not only observed ones), use_ur (stereo gate).  Outputs d_out, d_out_n.
//
// Lanes per query of the window search: the SearchByProjection family (modes 0 / 1) has short lists
// -- a 64-lane pass over one would be mostly idle -- and takes 16; SearchForInitialization's 100-px windows hold more than
// 64 candidates as a rule and keep the whole wavefront.  The tracking step knows its radius factor on the host: the two
// widths' times cross at th 19 (32 pairs) / 23 (85 pairs) -- 16 lanes win at 7 / 15 and lose at 30 / 60 / 100,
// profiles/window_groups_track_th.json -- so a search wider than th 20 takes the wavefront form.  The other mode 0 / 1
// entries get their radii in the query records and are not measured per radius: they take 16 lanes.
constexpr float kWindowLanesTh = 20.0f;
static int window_lanes(const orbhip_matcher *m, int mode, const ProjLaunch *proj = nullptr)
{
#ifdef ORBHIP_DEVTOOLS
    if (m->window_lanes) return m->window_lanes;
#endif
    if (proj && proj->th > kWindowLanesTh) return 64;
    return mode == 2 ? 64 : 16;
}
static int launch_search(orbhip_matcher *m, int mode, int pairs, const DevFrame &D, const Batch &B, const orbhip_query *d_q,
                         const uint8_t *d_qdesc, const orbhip_keypoint *d_qkeys, const uint8_t *d_taken, float nnratio,
                         int check_ori, int th_accept, int all_block, int use_ur, int *d_out, int *d_out_n, const int lanes,
                         const ProjLaunch *proj = nullptr)
{
    void *p;
    int rc;
    const int stride = (B.cap + 1) & ~1;
    const size_t nql = (size_t)pairs * B.qcap;   // query lists
    if ((rc = scratch(m, S_CAND, nql * stride * sizeof(unsigned long long), &p))) return rc;
    unsigned long long *d_cand = (unsigned long long *)p;
    if ((rc = scratch(m, S_CNT, nql * sizeof(int), &p))) return rc;
    int *d_cnt = (int *)p;
    if ((rc = scratch(m, S_CCAND, nql * kCompact * sizeof(unsigned long long), &p))) return rc;
    unsigned long long *d_ccand = (unsigned long long *)p;
    // CSR workspace per pair: cell table, records (16 B), descriptors (32 B), uRight (4 B) in CSR order
    const size_t start_bytes = al256((size_t)pairs * (kGridCells + 1) * sizeof(int));
    const size_t nrec = (size_t)pairs * B.cap;
    if ((rc = scratch(m, S_CSR, start_bytes + al256(nrec * sizeof(GridRec)) + al256(nrec * 32) + al256(nrec * 4), &p))) return rc;
    static_assert(sizeof(GridRec) == 16, "GridRec is one dwordx4");
    int *d_start = (int *)p;
    GridRec *d_rec = (GridRec *)((uint8_t *)p + start_bytes);
    uint4 *d_rdesc = (uint4 *)((uint8_t *)d_rec + al256(nrec * sizeof(GridRec)));
    float *d_rur = (float *)((uint8_t *)d_rdesc + al256(nrec * 32));
    if ((rc = ensure_resolve_attr(m))) return rc;
    if (mode == 2) { d_taken = nullptr; use_ur = 0; }
    if (proj) {
        const int npb = (proj->P.cap + 255) / 256;
        hipLaunchKernelGGL(k_grid_build_project, dim3(pairs * (npb + 1)), dim3(256), 0, m->stream, D, d_start, d_rec, d_rdesc, d_rur, B,
                           proj->P, proj->cam, proj->th, proj->mono, npb);
    } else {
        hipLaunchKernelGGL(k_grid_build, dim3(pairs), dim3(256), 0, m->stream, D, d_start, d_rec, d_rdesc, d_rur, B);
    }
    // searches that take the best candidate alone list nothing beyond their acceptance threshold
    const int max_dist = mode == 0 ? th_accept : 256;
    if (lanes == 16)
        hipLaunchKernelGGL(k_window_search<16>, dim3((B.qcap + 15) / 16, pairs), dim3(256), 0, m->stream, D, d_start, d_rec, d_rdesc,
                           d_rur, d_q, d_qdesc, d_cand, d_ccand, d_cnt, stride, use_ur, B, d_taken, max_dist);
    else
        hipLaunchKernelGGL(k_window_search<64>, dim3((B.qcap + 3) / 4, pairs), dim3(256), 0, m->stream, D, d_start, d_rec, d_rdesc,
                           d_rur, d_q, d_qdesc, d_cand, d_ccand, d_cnt, stride, use_ur, B, d_taken, max_dist);
    if (mode == 2) {   // match stealing depends on the running minimum distance per slot
        const int lcn = init_state_bytes((size_t)B.cap, (size_t)B.qcap, kResolveHead) <= (size_t)kResolveLdsBudget ? kResolveHead : 0;
        hipLaunchKernelGGL(k_resolve_init, dim3(pairs), dim3(1024), init_state_bytes((size_t)B.cap, (size_t)B.qcap, (size_t)lcn),
                           m->stream, D, d_qkeys, B.qcap, d_cand, d_ccand, d_cnt, stride, nnratio, check_ori, d_out, d_out_n, B, lcn);
    } else if ((rc = launch_resolve_par(m, pairs, mode, D, d_q, d_cand, d_ccand, d_cnt, stride, d_taken, nnratio, check_ori, d_out,
                                        d_out_n, B, th_accept, all_block))) {
        return rc;
    }
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

// Host-pointer windowed searches, one pair.  Modes 0 / 1 (the SearchByProjection family): queries with valid == 0 (no
// map point, not in view, ...) never reach the device -- local maps and loop-closing point sets are mostly that -- and
// there is no size limit (beyond kResolveMax the resolve state moves from LDS to HBM).  Mode 2 (SearchForInitialization)
// keeps its state in LDS: <= kResolveMax.
static int run_search(orbhip_matcher *m, int mode, const orbhip_frame_view *train, const orbhip_query *q,
                      const uint8_t *qdesc, const orbhip_keypoint *qkeys, int nq, const uint8_t *taken,
                      float nnratio, int check_ori, int32_t *out, int nout, int *nmatches, int th_accept = TH_HIGH,
                      int all_block = 0, int use_ur = 1)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    if (mode == 2 && (train->n > kResolveMax || nq > kResolveMax)) {
        set_error("SearchForInitialization: %d / %d keypoints exceed the LDS-resident limit %d", train->n, nq, kResolveMax);
        return ORBHIP_E_CAPACITY;
    }
    if (train->n >= (1 << 20)) { set_error("matcher: too many train keypoints"); return ORBHIP_E_CAPACITY; }
    for (int i = 0; i < nout; ++i) out[i] = -1;
    *nmatches = 0;
    if (nq == 0 || train->n == 0) return ORBHIP_OK;
    // stable compaction of the valid queries (order = the reference's loop order)
    static thread_local std::vector<int> vidx;
    vidx.clear();
    if (mode != 2) {
        for (int i = 0; i < nq; ++i) if (q[i].valid) vidx.push_back(i);
        if (vidx.empty()) return ORBHIP_OK;
    }
    const bool compact = mode != 2 && (int)vidx.size() < nq;
    const int nqv = compact ? (int)vidx.size() : nq;
    const size_t n = (size_t)train->n;
    Stage st;
    int rc;
    DevFrame D;
    const uint8_t *d_taken, *d_qdesc;
    const orbhip_query *d_q;
    const orbhip_keypoint *d_qkeys;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            D = dev_frame(train, stg);
            d_taken = taken ? stg.put(taken, n) : nullptr;
            if (compact) {
                d_q = stg.fill<orbhip_query>((size_t)nqv, [&](orbhip_query *hq) { for (int k = 0; k < nqv; ++k) hq[k] = q[vidx[k]]; });
                d_qdesc = stg.fill<uint8_t>((size_t)nqv * 32, [&](uint8_t *hd) {
                    for (int k = 0; k < nqv; ++k) memcpy(hd + (size_t)k * 32, qdesc + (size_t)vidx[k] * 32, 32);
                });
            } else {
                d_q = stg.put(q, (size_t)nq);
                d_qdesc = stg.put(qdesc, (size_t)nq * 32);
            }
            d_qkeys = qkeys ? stg.put(qkeys, (size_t)nq) : nullptr;
        }))) return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)(nout + 1) * sizeof(int), &p))) return rc;
    int *d_out = (int *)p;
    const Batch B = {nullptr, nullptr, train->n, nqv};
    if ((rc = launch_search(m, mode, 1, D, B, d_q, d_qdesc, d_qkeys, d_taken, nnratio, check_ori, th_accept, all_block, use_ur,
                            d_out, d_out + nout, window_lanes(m, mode))))
        return rc;
    const uint8_t *h;
    if ((rc = read_back(m, d_out, (size_t)(nout + 1) * sizeof(int), &h))) return rc;
    memcpy(out, h, (size_t)nout * sizeof(int));
    if (compact)   // slots hold indices into the compacted query list: map them back
        for (int i = 0; i < nout; ++i) if (out[i] >= 0) out[i] = vidx[out[i]];
    *nmatches = reinterpret_cast<const int *>(h)[nout];
    return ORBHIP_OK;
}

// processing order of the reference: FeatureVector nodes ascending, feature indices ascending inside a node
static void node_order(const uint32_t *node, const uint8_t *valid, int n, std::vector<int> &order)
{
    static thread_local std::vector<unsigned long long> keys;
    keys.clear();
    keys.reserve(n);
    for (int i = 0; i < n; ++i)
        if (node[i] != ORBHIP_NO_NODE && (!valid || valid[i])) keys.push_back(((unsigned long long)node[i] << 32) | (unsigned)i);
    std::sort(keys.begin(), keys.end());
    order.resize(keys.size());
    for (size_t k = 0; k < keys.size(); ++k) order[k] = (int)(uint32_t)keys[k];
}

// SearchByBoW, both overloads
static int run_bow(orbhip_matcher *m, const orbhip_frame_view *f1, const uint32_t *node1, const uint8_t *valid1,
                   const orbhip_frame_view *f2, const uint32_t *node2, const uint8_t *blocked2, int max_dist,
                   float nnratio, int check_ori, int32_t *matches12, int *nmatches)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const int n1 = f1->n, n2 = f2->n;
    for (int i = 0; i < n1; ++i) matches12[i] = -1;
    *nmatches = 0;
    if (n1 == 0 || n2 == 0) return ORBHIP_OK;
    std::vector<int> order, torder;
    node_order(node1, valid1, n1, order);
    node_order(node2, nullptr, n2, torder);   // blocked features keep their slot: they only start out "matched"
    const int nq = (int)order.size(), nt = (int)torder.size();
    if (nq == 0 || nt == 0) return ORBHIP_OK;
    std::vector<NodeGroup> groups;            // common nodes, the merge of ORBmatcher.cc:185-286
    for (int a = 0, b = 0; a < nq && b < nt;) {
        const uint32_t na = node1[order[a]], nb = node2[torder[b]];
        if (na == nb) {
            int ae = a, be = b;
            while (ae < nq && node1[order[ae]] == na) ++ae;
            while (be < nt && node2[torder[be]] == na) ++be;
            groups.push_back(NodeGroup{a, ae, b, be});
            a = ae; b = be;
        } else if (na < nb) ++a;
        else ++b;
    }
    const int ng = (int)groups.size();
    if (ng == 0) return ORBHIP_OK;
    const size_t n = (size_t)n2;
    Stage st;
    int rc;
    const orbhip_keypoint *d_tkeys;
    const uint8_t *d_tdesc, *d_qdesc;
    const uint32_t *d_torder;
    uint8_t *d_matched;
    const float *d_qangle;
    const NodeGroup *d_groups;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_tkeys = stg.put(f2->keys, n);
            d_tdesc = stg.put(f2->desc, n * 32);
            d_torder = stg.put(reinterpret_cast<const uint32_t *>(torder.data()), (size_t)nt);
            d_matched = stg.fill<uint8_t>((size_t)nt, [&](uint8_t *hm) {
                for (int c = 0; c < nt; ++c) hm[c] = (uint8_t)(blocked2 && blocked2[torder[c]]);
            });
            d_qdesc = stg.fill<uint8_t>((size_t)nq * 32, [&](uint8_t *hqd) {
                for (int p = 0; p < nq; ++p) memcpy(hqd + (size_t)p * 32, f1->desc + (size_t)order[p] * 32, 32);
            });
            d_qangle = stg.fill<float>((size_t)nq, [&](float *hqa) { for (int p = 0; p < nq; ++p) hqa[p] = f1->keys[order[p]].angle; });
            d_groups = stg.put(groups.data(), (size_t)ng);
        }))) return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)(nq + 1) * sizeof(int), &p))) return rc;
    int *d_out = (int *)p;
    // queries whose node does not occur in f2 belong to no group: they stay at -1
    ORBHIP_HIP_CHECK(hipMemsetAsync(d_out, 0xff, (size_t)nq * sizeof(int), m->stream));
    hipLaunchKernelGGL(k_bow_groups, dim3((ng + 3) / 4), dim3(256), 0, m->stream, d_groups, ng, d_qdesc, d_torder, d_tdesc,
                       d_matched, max_dist, nnratio, d_out);
    hipLaunchKernelGGL(k_rot_cull, dim3(1), dim3(1024), 0, m->stream, d_out, nq, (const void *)d_qangle, 4, d_tkeys, check_ori,
                       d_out + nq);
    const uint8_t *h;
    if ((rc = read_back(m, d_out, (size_t)(nq + 1) * sizeof(int), &h))) return rc;
    const int *res = reinterpret_cast<const int *>(h);
    for (const NodeGroup &G : groups)
        for (int q = G.q_begin; q < G.q_end; ++q) matches12[order[q]] = res[q];
    *nmatches = res[nq];
    return ORBHIP_OK;
}

// SearchForTriangulation.  The kResolveMax size limit is the one include/orbhip.h documents for the entry point (n1, n2 <=
// 4096); nothing on this path sizes device state by it.
static int run_tri(orbhip_matcher *m, const TriParams *tri, const orbhip_frame_view *f1, const uint32_t *node1,
                   const uint8_t *valid1, const orbhip_frame_view *f2, const uint32_t *node2, const uint8_t *valid2,
                   int only_stereo, int check_ori, int32_t *matches12, int *nmatches)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const int n1 = f1->n, n2 = f2->n;
    if (n1 > kResolveMax || n2 > kResolveMax) {
        set_error("matcher: %d / %d keypoints exceed the LDS-resident limit %d", n1, n2, kResolveMax);
        return ORBHIP_E_CAPACITY;
    }
    for (int i = 0; i < n1; ++i) matches12[i] = -1;
    *nmatches = 0;
    if (n1 == 0 || n2 == 0) return ORBHIP_OK;
    std::vector<int> order;
    node_order(node1, valid1, n1, order);
    if (only_stereo) {   // :706-708
        size_t w = 0;
        for (size_t r = 0; r < order.size(); ++r)
            if (f1->u_right && f1->u_right[order[r]] >= 0) order[w++] = order[r];
        order.resize(w);
    }
    const int nq = (int)order.size();
    if (nq == 0) return ORBHIP_OK;
    const size_t n = (size_t)n2;
    Stage st;
    int rc;
    DevFrame D;
    D.n = n2; D.min_x = D.min_y = 0.f; D.inv_w = D.inv_h = 0.f;
    const uint32_t *d_tnode;
    const uint8_t *d_mask, *d_qdesc;
    const orbhip_query *d_q;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            D.keys = stg.put(f2->keys, n);
            D.desc = stg.put(f2->desc, n * 32);
            D.u_right = f2->u_right ? stg.put(f2->u_right, n) : nullptr;
            d_tnode = stg.put(node2, n);
            d_mask = nullptr;   // candidate filter: no map point yet (+ bOnlyStereo :725-729)
            if (valid2 || only_stereo)
                d_mask = stg.fill<uint8_t>(n, [&](uint8_t *hm) {
                    for (int j = 0; j < n2; ++j)
                        hm[j] = (uint8_t)((!valid2 || valid2[j]) && (!only_stereo || (f2->u_right && f2->u_right[j] >= 0)));
                });
            d_q = stg.fill<orbhip_query>((size_t)nq, [&](orbhip_query *hq) {
                for (int p = 0; p < nq; ++p) {
                    const int i = order[p];
                    orbhip_query &Q = hq[p];
                    memset(&Q, 0, sizeof(Q));
                    Q.valid = 1;
                    Q.u = f1->keys[i].x; Q.v = f1->keys[i].y;
                    Q.ur = f1->u_right ? f1->u_right[i] : -1.0f;
                    Q.level_aux = (int32_t)node1[i];
                    Q.angle = f1->keys[i].angle;
                }
            });
            d_qdesc = stg.fill<uint8_t>((size_t)nq * 32, [&](uint8_t *hqd) {
                for (int p = 0; p < nq; ++p) memcpy(hqd + (size_t)p * 32, f1->desc + (size_t)order[p] * 32, 32);
            });
        }))) return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)(nq + 1) * sizeof(int), &p))) return rc;
    int *d_out = (int *)p;
    hipLaunchKernelGGL(k_tri_search, dim3((nq + 3) / 4), dim3(256), 0, m->stream, D, d_tnode, d_mask, d_q, d_qdesc, nq, d_out,
                       *tri);
    hipLaunchKernelGGL(k_rot_cull, dim3(1), dim3(1024), 0, m->stream, d_out, nq, (const void *)&d_q->angle,
                       (int)sizeof(orbhip_query), D.keys, check_ori, d_out + nq);
    const uint8_t *h;
    if ((rc = read_back(m, d_out, (size_t)(nq + 1) * sizeof(int), &h))) return rc;
    const int *res = reinterpret_cast<const int *>(h);
    for (int q = 0; q < nq; ++q) matches12[order[q]] = res[q];
    *nmatches = res[nq];
    return ORBHIP_OK;
}

// ComputeStereoMatches of `pairs` pairs.  B: counts, frame mapping and keypoint capacity of the key arrays (pair p = left
// frame l0 + p*ls against right frame r0 + p*rs); the pyramids are read at the same frame index plus pyr_l / pyr_r frames
// (the host entry stages one pair's keypoints as frame 0 of frames pyr_l / pyr_r).  uRight, depth: [pairs][cap].
static int launch_stereo(orbhip_matcher *m, orbhip_extractor *left, int pyr_l, orbhip_extractor *right, int pyr_r, int pairs,
                         StereoBatch B, const orbhip_keypoint *d_kl, const uint8_t *d_dl, const orbhip_keypoint *d_kr,
                         const uint8_t *d_dr, float mbf, float mb, float *d_u_right, float *d_depth, int *d_nmatches)
{
    StereoGeom G;
    memset(&G, 0, sizeof(G));
    G.nlevels = left->nlevels; G.nrows = left->G.lv[0].h; G.mbf = mbf; G.mb = mb;
    for (int l = 0; l < G.nlevels; ++l) {
        const LevelGeom &A = left->G.lv[l], &Bv = right->G.lv[l];
        G.left[l] = left->d_pyr + (size_t)pyr_l * left->G.frame_bytes + A.plane_off + (size_t)kEdge * A.pitch + kPadL;
        G.right[l] = right->d_pyr + (size_t)pyr_r * right->G.frame_bytes + Bv.plane_off + (size_t)kEdge * Bv.pitch + kPadL;
        G.pitch_l[l] = A.pitch; G.pitch_r[l] = Bv.pitch; G.cols_r[l] = Bv.w;
        G.sf[l] = left->sf[l]; G.isf[l] = left->isf[l];
    }
    for (int l = G.nlevels; l < ORBHIP_MAX_LEVELS; ++l) { G.left[l] = G.left[0]; G.right[l] = G.right[0]; }
    B.fb_l = left->G.frame_bytes; B.fb_r = right->G.frame_bytes;
    const int cap = B.cap;
    void *p;
    int rc;
    const size_t rs_bytes = al256((size_t)pairs * ((size_t)G.nrows + 1) * sizeof(int));
    if ((rc = scratch(m, S_ORD, rs_bytes + (size_t)pairs * cap * sizeof(int4), &p))) return rc;
    int *d_rowstart = (int *)p;
    int4 *d_order = reinterpret_cast<int4 *>((uint8_t *)p + rs_bytes);
    if ((rc = scratch(m, S_CNT, (size_t)pairs * cap * sizeof(int), &p))) return rc;
    int *d_sad = (int *)p;
    if (G.nrows <= kStereoRowsMax)
        hipLaunchKernelGGL(k_stereo_sort, dim3(pairs), dim3(256), 0, m->stream, d_kr, cap, G.nrows, d_rowstart, d_order, B, stereo_scales(G));
    else d_rowstart = nullptr;   // taller images: every right keypoint is a candidate
    hipLaunchKernelGGL(k_stereo_match, dim3((cap + 3) / 4, pairs), dim3(256), 0, m->stream, d_kl, d_dl, d_kr, d_dr,
                       (const int *)d_rowstart, (const int4 *)d_order, stereo_row_reach(G), G, d_u_right, d_depth, d_sad, B);
    hipLaunchKernelGGL(k_stereo_cull, dim3(pairs), dim3(256), 0, m->stream, d_sad, d_u_right, d_depth, d_nmatches, B);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

extern "C" {

int orbhip_matcher_create(int device, orbhip_matcher **out)
{
    if (!out) return ORBHIP_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_error("no HIP device %d (found %d)", device, ndev);
        return ORBHIP_E_NODEVICE;
    }
    orbhip_matcher *m = new (std::nothrow) orbhip_matcher();
    if (!m) return ORBHIP_E_ARG;
    m->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipSetDevice/hipStreamCreate failed");
        delete m;
        return ORBHIP_E_HIP;
    }
    m->stream = m->own_stream;
    *out = m;
    return ORBHIP_OK;
}

void orbhip_matcher_destroy(orbhip_matcher *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (int i = 0; i < S_NSLOTS; ++i) (void)hipFree(m->buf[i]);
    if (m->h_stage) (void)hipHostFree(m->h_stage);
    if (m->h_out) (void)hipHostFree(m->h_out);
    if (m->h_eg) (void)hipHostFree(m->h_eg);
    if (m->h_gba) (void)hipHostFree(m->h_gba);
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    delete m;
}

int orbhip_descriptor_distance(orbhip_matcher *m, const uint8_t *a, int na, const uint8_t *b, int nb, int32_t *dist)
{
    if (!m || !a || !b || !dist || na < 0 || nb < 0) return ORBHIP_E_ARG;
    if (na == 0 || nb == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *pa, *pb, *pd;
    int rc;
    if ((rc = scratch(m, S_DESC, (size_t)na * 32, &pa))) return rc;
    if ((rc = scratch(m, S_QDESC, (size_t)nb * 32, &pb))) return rc;
    if ((rc = scratch(m, S_CAND, (size_t)na * nb * sizeof(int), &pd))) return rc;
    ORBHIP_HIP_CHECK(hipMemcpyAsync(pa, a, (size_t)na * 32, hipMemcpyHostToDevice, m->stream));
    ORBHIP_HIP_CHECK(hipMemcpyAsync(pb, b, (size_t)nb * 32, hipMemcpyHostToDevice, m->stream));
    hipLaunchKernelGGL(k_distance_matrix, dim3((nb + 255) / 256, na), dim3(256), 0, m->stream, (const uint8_t *)pa, na,
                       (const uint8_t *)pb, nb, (int *)pd);
    ORBHIP_HIP_CHECK(hipGetLastError());
    ORBHIP_HIP_CHECK(hipMemcpyAsync(dist, pd, (size_t)na * nb * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
    return ORBHIP_OK;
}

int orbhip_search_for_initialization(orbhip_matcher *m, const orbhip_frame_view *f1, const orbhip_frame_view *f2,
                                     float *prev_matched_xy, int32_t *matches12, int window_size, float nnratio,
                                     int check_ori, int *nmatches)
{
    if (!m || !f1 || !f2 || !prev_matched_xy || !matches12 || !nmatches) return ORBHIP_E_ARG;
    const int n1 = f1->n;
    // queries: level-0 keypoints of F1 searched around vbPrevMatched (ORBmatcher.cc:418-425)
    std::vector<orbhip_query> q((size_t)std::max(n1, 1));
    for (int i = 0; i < n1; ++i) {
        orbhip_query &Q = q[i];
        memset(&Q, 0, sizeof(Q));
        const int level1 = f1->keys[i].octave;
        Q.valid = level1 > 0 ? 0 : 1;
        Q.u = prev_matched_xy[2 * i]; Q.v = prev_matched_xy[2 * i + 1];
        Q.radius = (float)window_size;
        Q.min_level = level1; Q.max_level = level1;
        Q.angle = f1->keys[i].angle;
    }
    int rc = run_search(m, 2, f2, q.data(), f1->desc, f1->keys, n1, nullptr, nnratio, check_ori, matches12, n1, nmatches);
    if (rc) return rc;
    for (int i = 0; i < n1; ++i)  // :515-517
        if (matches12[i] >= 0) {
            prev_matched_xy[2 * i] = f2->keys[matches12[i]].x;
            prev_matched_xy[2 * i + 1] = f2->keys[matches12[i]].y;
        }
    return ORBHIP_OK;
}

int orbhip_search_by_projection_frame(orbhip_matcher *m, const orbhip_frame_view *cur, const orbhip_query *q,
                                      const uint8_t *qdesc, int nq, const uint8_t *taken, int32_t *assign,
                                      int check_ori, int *nmatches)
{
    if (!m || !cur || (nq > 0 && (!q || !qdesc)) || !assign || !nmatches || nq < 0) return ORBHIP_E_ARG;
    return run_search(m, 0, cur, q, qdesc, nullptr, nq, taken, 0.f, check_ori, assign, cur->n, nmatches);
}

int orbhip_search_by_projection_keyframe(orbhip_matcher *m, const orbhip_frame_view *cur, const orbhip_query *q,
                                         const uint8_t *qdesc, int nq, const uint8_t *taken, int32_t *assign,
                                         int orb_dist, int check_ori, int *nmatches)
{
    if (!m || !cur || (nq > 0 && (!q || !qdesc)) || !assign || !nmatches || nq < 0) return ORBHIP_E_ARG;
    return run_search(m, 0, cur, q, qdesc, nullptr, nq, taken, 0.f, check_ori, assign, cur->n, nmatches, orb_dist, 1, 0);
}

int orbhip_search_by_projection_sim3(orbhip_matcher *m, const orbhip_frame_view *kf, const orbhip_query *q,
                                     const uint8_t *qdesc, int nq, const uint8_t *matched, int32_t *assign, int *nmatches)
{
    if (!m || !kf || (nq > 0 && (!q || !qdesc)) || !assign || !nmatches || nq < 0) return ORBHIP_E_ARG;
    return run_search(m, 0, kf, q, qdesc, nullptr, nq, matched, 0.f, 0, assign, kf->n, nmatches, TH_LOW, 1, 0);
}

int orbhip_assign_features_to_grid_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap,
                                          float min_x, float min_y, float grid_inv_w, float grid_inv_h, void *d_cell_of,
                                          void *d_cell_start, void *d_cell_items)
{
    if (!m || frames < 0 || cap < 1 || !d_kps || !d_n || !d_cell_of || !d_cell_start || !d_cell_items) return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("assign_features_to_grid: capacity %d exceeds %d", cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const DevFrame D = dev_frame(0, d_kps, nullptr, nullptr, min_x, min_y, grid_inv_w, grid_inv_h);
    const Batch B = {(const int *)d_n, nullptr, cap, 0};
    hipLaunchKernelGGL(k_grid_csr, dim3(frames), dim3(1024), 0, m->stream, D, B, (int *)d_cell_of, (int *)d_cell_start,
                       (int *)d_cell_items);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_assign_features_to_grid(orbhip_matcher *m, const orbhip_frame_view *f, int32_t *cell_of, int32_t *cell_start,
                                   int32_t *cell_items)
{
    if (!m || !f || f->n < 0 || !cell_start || (f->n > 0 && (!f->keys || !cell_of || !cell_items))) return ORBHIP_E_ARG;
    const int n = f->n;
    if (n > kGridMax) { set_error("assign_features_to_grid: %d keypoints exceed %d", n, kGridMax); return ORBHIP_E_CAPACITY; }
    if (n == 0) { for (int c = 0; c <= kGridCells; ++c) cell_start[c] = 0; return ORBHIP_OK; }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    int rc;
    const orbhip_keypoint *d_keys;
    const int *d_n;
    if ((rc = stage_send(m, &st, [&](Stage &stg) { d_keys = stg.put(f->keys, (size_t)n); d_n = stg.put(&n, 1); }))) return rc;
    const size_t ob = ((size_t)2 * n + kGridCells + 1) * sizeof(int);
    void *p;
    if ((rc = scratch(m, S_OUT, ob, &p))) return rc;
    int *d_out = (int *)p;
    if ((rc = orbhip_assign_features_to_grid_device(m, 1, d_keys, d_n, n, f->min_x, f->min_y, f->grid_inv_w, f->grid_inv_h,
                                                    d_out, d_out + 2 * n, d_out + n))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, d_out, ob, &h))) return rc;
    const int *r = reinterpret_cast<const int *>(h);
    memcpy(cell_of, r, (size_t)n * sizeof(int));
    memcpy(cell_items, r + n, (size_t)n * sizeof(int));
    memcpy(cell_start, r + 2 * n, (size_t)(kGridCells + 1) * sizeof(int));
    return ORBHIP_OK;
}

int orbhip_undistort_keypoints_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap, float fx,
                                      float fy, float cx, float cy, const float *dist5, void *d_kps_un)
{
    if (!m || frames < 0 || cap < 1 || !d_kps || !d_n || !dist5 || !d_kps_un || fx == 0.f || fy == 0.f) return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    if (dist5[0] == 0.0f) {   // mvKeysUn = mvKeys (:406-410)
        if (d_kps_un != d_kps)
            ORBHIP_HIP_CHECK(hipMemcpyAsync(d_kps_un, d_kps, (size_t)frames * cap * sizeof(orbhip_keypoint), hipMemcpyDeviceToDevice, m->stream));
        return ORBHIP_OK;
    }
    UndistortParams P;
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy;
    for (int i = 0; i < 5; ++i) P.k[i] = dist5[i];
    hipLaunchKernelGGL(k_undistort, dim3((cap + 255) / 256, frames), dim3(256), 0, m->stream, (const orbhip_keypoint *)d_kps,
                       (const int *)d_n, 0, cap, P, (orbhip_keypoint *)d_kps_un);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_undistort_keypoints(orbhip_matcher *m, const orbhip_keypoint *keys, int n, float fx, float fy, float cx, float cy,
                               const float *dist5, orbhip_keypoint *keys_un)
{
    if (!m || n < 0 || (n > 0 && (!keys || !keys_un)) || !dist5 || fx == 0.f || fy == 0.f) return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    int rc;
    const orbhip_keypoint *d_keys;
    const int *d_n;
    if ((rc = stage_send(m, &st, [&](Stage &stg) { d_keys = stg.put(keys, (size_t)n); d_n = stg.put(&n, 1); }))) return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)n * sizeof(orbhip_keypoint), &p))) return rc;
    if ((rc = orbhip_undistort_keypoints_device(m, 1, d_keys, d_n, n, fx, fy, cx, cy, dist5, p))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, p, (size_t)n * sizeof(orbhip_keypoint), &h))) return rc;
    memcpy(keys_un, h, (size_t)n * sizeof(orbhip_keypoint));
    return ORBHIP_OK;
}

int orbhip_compute_stereo_from_rgbd_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_kps_un,
                                           const void *d_n, int cap, const void *d_depth, int rows, int cols,
                                           int stride_floats, size_t frame_stride_floats, float mbf, void *d_u_right,
                                           void *d_depth_out)
{
    if (!m || frames < 0 || cap < 1 || !d_kps || !d_n || !d_depth || rows < 1 || cols < 1 || stride_floats < cols ||
        !d_u_right || !d_depth_out)
        return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    hipLaunchKernelGGL(k_stereo_from_rgbd, dim3((cap + 255) / 256, frames), dim3(256), 0, m->stream,
                       (const orbhip_keypoint *)d_kps, (const orbhip_keypoint *)(d_kps_un ? d_kps_un : d_kps), (const int *)d_n,
                       0, cap, (const float *)d_depth, rows, cols, stride_floats, frame_stride_floats, mbf, (float *)d_u_right,
                       (float *)d_depth_out);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_compute_stereo_from_rgbd(orbhip_matcher *m, const orbhip_keypoint *keys, const orbhip_keypoint *keys_un, int n,
                                    const float *depth, int rows, int cols, int stride_floats, float mbf, float *u_right,
                                    float *depth_out)
{
    if (!m || n < 0 || (n > 0 && (!keys || !u_right || !depth_out)) || !depth || rows < 1 || cols < 1 || stride_floats < cols)
        return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    if (!keys_un) keys_un = keys;
    // the depth image travels like the grey image does for extraction: packed rows through the pinned staging buffer
    Stage st;
    int rc;
    const orbhip_keypoint *d_keys, *d_un;
    const float *d_depth;
    const int *d_n;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_keys = stg.put(keys, (size_t)n);
            d_un = stg.put(keys_un, (size_t)n);
            d_depth = stg.fill<float>((size_t)rows * cols, [&](float *hd) {
                for (int r = 0; r < rows; ++r) memcpy(hd + (size_t)r * cols, depth + (size_t)r * stride_floats, (size_t)cols * sizeof(float));
            });
            d_n = stg.put(&n, 1);
        }))) return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)2 * n * sizeof(float), &p))) return rc;
    float *d_out = (float *)p;
    if ((rc = orbhip_compute_stereo_from_rgbd_device(m, 1, d_keys, d_un, d_n, n, d_depth, rows, cols, cols, 0, mbf, d_out,
                                                     d_out + n))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, d_out, (size_t)2 * n * sizeof(float), &h))) return rc;
    memcpy(u_right, h, (size_t)n * sizeof(float));
    memcpy(depth_out, h + (size_t)n * sizeof(float), (size_t)n * sizeof(float));
    return ORBHIP_OK;
}

int orbhip_compute_stereo_from_rgbd_raw_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_kps_un,
                                               const void *d_n, int cap, const void *d_depth, int depth_type, int rows, int cols,
                                               int stride_elems, size_t frame_stride_elems, float depth_factor, float mbf,
                                               void *d_u_right, void *d_depth_out)
{
    if (!m || frames < 0 || cap < 1 || !d_kps || !d_n || !d_depth || rows < 1 || cols < 1 || stride_elems < cols ||
        !d_u_right || !d_depth_out || (depth_type != ORBHIP_DEPTH_U16 && depth_type != ORBHIP_DEPTH_F32))
        return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const orbhip_keypoint *k = (const orbhip_keypoint *)d_kps, *ku = (const orbhip_keypoint *)(d_kps_un ? d_kps_un : d_kps);
    const dim3 grid((cap + 255) / 256, frames);
    if (depth_type == ORBHIP_DEPTH_U16) {
        hipLaunchKernelGGL(k_stereo_from_rgbd_raw<uint16_t>, grid, dim3(256), 0, m->stream, k, ku, (const int *)d_n, cap,
                           (const uint16_t *)d_depth, rows, cols, stride_elems, frame_stride_elems, depth_factor, 1, mbf,
                           (float *)d_u_right, (float *)d_depth_out);
    } else {
        volatile float diff = depth_factor - 1.0f;   // float subtraction, then fabs and the comparison in double (:227)
        const int convert = fabs((double)diff) > 1e-5;
        hipLaunchKernelGGL(k_stereo_from_rgbd_raw<float>, grid, dim3(256), 0, m->stream, k, ku, (const int *)d_n, cap,
                           (const float *)d_depth, rows, cols, stride_elems, frame_stride_elems, depth_factor, convert, mbf,
                           (float *)d_u_right, (float *)d_depth_out);
    }
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_compute_stereo_from_rgbd_raw(orbhip_matcher *m, const orbhip_keypoint *keys, const orbhip_keypoint *keys_un, int n,
                                        const void *depth, int depth_type, int rows, int cols, int stride_elems,
                                        float depth_factor, float mbf, float *u_right, float *depth_out)
{
    if (!m || n < 0 || (n > 0 && (!keys || !u_right || !depth_out)) || !depth || rows < 1 || cols < 1 || stride_elems < cols ||
        (depth_type != ORBHIP_DEPTH_U16 && depth_type != ORBHIP_DEPTH_F32))
        return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    if (!keys_un) keys_un = keys;
    // the raw depth image travels as the float one does: packed rows through the pinned staging buffer, half the bytes for uint16
    Stage st;
    int rc;
    const size_t esz = depth_type == ORBHIP_DEPTH_U16 ? 2 : 4, rb = (size_t)cols * esz;
    const orbhip_keypoint *d_keys, *d_un;
    const uint8_t *d_depth;
    const int *d_n;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_keys = stg.put(keys, (size_t)n);
            d_un = stg.put(keys_un, (size_t)n);
            d_depth = stg.fill<uint8_t>((size_t)rows * rb, [&](uint8_t *hd) {
                for (int r = 0; r < rows; ++r) memcpy(hd + (size_t)r * rb, (const uint8_t *)depth + (size_t)r * stride_elems * esz, rb);
            });
            d_n = stg.put(&n, 1);
        }))) return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)2 * n * sizeof(float), &p))) return rc;
    float *d_out = (float *)p;
    if ((rc = orbhip_compute_stereo_from_rgbd_raw_device(m, 1, d_keys, d_un, d_n, n, d_depth, depth_type, rows, cols, cols, 0,
                                                         depth_factor, mbf, d_out, d_out + n))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, d_out, (size_t)2 * n * sizeof(float), &h))) return rc;
    memcpy(u_right, h, (size_t)n * sizeof(float));
    memcpy(depth_out, h + (size_t)n * sizeof(float), (size_t)n * sizeof(float));
    return ORBHIP_OK;
}

int orbhip_distinctive_descriptors(orbhip_matcher *m, const uint8_t *desc, const int32_t *offsets, int npoints,
                                   int32_t *best_idx)
{
    if (!m || npoints < 0 || (npoints > 0 && (!offsets || !best_idx))) return ORBHIP_E_ARG;
    if (npoints == 0) return ORBHIP_OK;
    if (offsets[0] < 0) return ORBHIP_E_ARG;
    for (int p = 0; p < npoints; ++p) {
        const long long N = (long long)offsets[p + 1] - offsets[p];
        if (N < 0) { set_error("distinctive_descriptors: offsets must be non-decreasing (point %d)", p); return ORBHIP_E_ARG; }
        if (N > kDistinctMax) {
            set_error("distinctive_descriptors: map point %d has %lld observations (limit %d)", p, N, kDistinctMax);
            return ORBHIP_E_CAPACITY;
        }
    }
    const size_t total = (size_t)offsets[npoints];
    if (total > 0 && !desc) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    int rc;
    const uint8_t *d_desc;
    const int *d_off;
    if ((rc = stage_send(m, &st, [&](Stage &stg) { d_desc = stg.put(desc, total * 32); d_off = stg.put(offsets, (size_t)npoints + 1); })))
        return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)npoints * sizeof(int), &p))) return rc;
    hipLaunchKernelGGL(k_distinctive, dim3((npoints + 3) / 4), dim3(256), 0, m->stream, d_desc, d_off, npoints, (int *)p);
    const uint8_t *h;
    if ((rc = read_back(m, p, (size_t)npoints * sizeof(int), &h))) return rc;
    memcpy(best_idx, h, (size_t)npoints * sizeof(int));
    return ORBHIP_OK;
}

int orbhip_search_by_bow(orbhip_matcher *m, const orbhip_frame_view *f1, const uint32_t *node1, const uint8_t *valid1,
                         const orbhip_frame_view *f2, const uint32_t *node2, const uint8_t *blocked2, int max_dist,
                         float nnratio, int check_ori, int32_t *matches12, int *nmatches)
{
    if (!m || !f1 || !f2 || !matches12 || !nmatches || f1->n < 0 || f2->n < 0) return ORBHIP_E_ARG;
    if ((f1->n > 0 && (!node1 || !f1->keys || !f1->desc)) || (f2->n > 0 && (!node2 || !f2->keys || !f2->desc)))
        return ORBHIP_E_ARG;
    return run_bow(m, f1, node1, valid1, f2, node2, blocked2, max_dist, nnratio, check_ori, matches12, nmatches);
}

int orbhip_search_by_bow_device(orbhip_matcher *m, int pairs, int cap, const void *d_kps1, const void *d_desc1,
                                const void *d_n1, const void *d_node1, const void *d_valid1, int f1_first, int f1_step,
                                const void *d_kps2, const void *d_desc2, const void *d_n2, const void *d_node2,
                                const void *d_blocked2, int f2_first, int f2_step, int max_dist, float nnratio,
                                int check_ori, void *d_matches12, void *d_nmatches)
{
    if (!m || pairs < 0 || cap < 1 || !d_kps1 || !d_desc1 || !d_n1 || !d_node1 || !d_kps2 || !d_desc2 || !d_n2 || !d_node2 ||
        !d_matches12 || !d_nmatches || f1_first < 0 || f2_first < 0 || f1_step < 0 || f2_step < 0)
        return ORBHIP_E_ARG;
    if (cap > kBowPairMax) {
        set_error("search_by_bow_device: capacity %d exceeds the LDS-resident limit %d", cap, kBowPairMax);
        return ORBHIP_E_CAPACITY;
    }
    if (pairs == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    if (!m->bow_attr_set) {
        ORBHIP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bow_pairs),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BowPairShared)));
        m->bow_attr_set = true;
    }
    const BowSide Q = {(const orbhip_keypoint *)d_kps1, (const uint8_t *)d_desc1, (const int *)d_n1, (const uint32_t *)d_node1,
                       (const uint8_t *)d_valid1, f1_first, f1_step};
    const BowSide T = {(const orbhip_keypoint *)d_kps2, (const uint8_t *)d_desc2, (const int *)d_n2, (const uint32_t *)d_node2,
                       (const uint8_t *)d_blocked2, f2_first, f2_step};
    hipLaunchKernelGGL(k_bow_pairs, dim3(pairs), dim3(1024), sizeof(BowPairShared), m->stream, Q, T, cap, max_dist, nnratio,
                       check_ori, (int *)d_matches12, (int *)d_nmatches);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_search_for_triangulation(orbhip_matcher *m, const orbhip_frame_view *f1, const uint32_t *node1,
                                    const uint8_t *valid1, const orbhip_frame_view *f2, const uint32_t *node2,
                                    const uint8_t *valid2, const float *f12, float ex, float ey,
                                    const float *level_sigma2, int only_stereo, int check_ori, int32_t *matches12,
                                    int *nmatches)
{
    if (!m || !f1 || !f2 || !f12 || !level_sigma2 || !matches12 || !nmatches || f1->n < 0 || f2->n < 0) return ORBHIP_E_ARG;
    if ((f1->n > 0 && (!node1 || !f1->keys || !f1->desc)) || (f2->n > 0 && (!node2 || !f2->keys || !f2->desc)))
        return ORBHIP_E_ARG;
    if (f2->n_levels < 1 || f2->n_levels > ORBHIP_MAX_LEVELS || !f2->scale_factors) {
        set_error("search_for_triangulation: f2 needs n_levels in [1,%d] and scale_factors", ORBHIP_MAX_LEVELS);
        return ORBHIP_E_ARG;
    }
    TriParams P;
    memset(&P, 0, sizeof(P));
    for (int i = 0; i < 9; ++i) P.f12[i] = f12[i];
    P.ex = ex; P.ey = ey;
    for (int l = 0; l < f2->n_levels; ++l) { P.sigma2[l] = level_sigma2[l]; P.sf[l] = f2->scale_factors[l]; }
    for (int j = 0; j < f2->n; ++j)
        if (f2->keys[j].octave < 0 || f2->keys[j].octave >= f2->n_levels) {
            set_error("search_for_triangulation: keypoint %d has octave %d outside [0,%d)", j, f2->keys[j].octave, f2->n_levels);
            return ORBHIP_E_ARG;
        }
    return run_tri(m, &P, f1, node1, valid1, f2, node2, valid2, only_stereo, check_ori, matches12, nmatches);
}

int orbhip_search_best_in_window(orbhip_matcher *m, const orbhip_frame_view *kf, const orbhip_query *q,
                                 const uint8_t *qdesc, int nq, int chi2_gate, const float *inv_level_sigma2,
                                 int32_t *best_idx, int32_t *best_dist)
{
    if (!m || !kf || nq < 0 || (nq > 0 && (!q || !qdesc || !best_idx || !best_dist)) || (chi2_gate && !inv_level_sigma2))
        return ORBHIP_E_ARG;
    for (int i = 0; i < nq; ++i) { best_idx[i] = -1; best_dist[i] = 256; }
    if (nq == 0 || kf->n == 0) return ORBHIP_OK;
    if (kf->n >= (1 << 20)) { set_error("too many keypoints"); return ORBHIP_E_CAPACITY; }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t n = (size_t)kf->n;
    Stage st;
    int rc;
    DevFrame D;
    const orbhip_query *d_q;
    const uint8_t *d_qdesc;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            D = dev_frame(kf, stg);
            d_q = stg.put(q, (size_t)nq);
            d_qdesc = stg.put(qdesc, (size_t)nq * 32);
        }))) return rc;
    void *p;
    if ((rc = scratch(m, S_ORD, n * sizeof(uint32_t), &p))) return rc;
    uint32_t *d_ord = (uint32_t *)p;
    if ((rc = scratch(m, S_OUT, (size_t)nq * 2 * sizeof(int), &p))) return rc;
    int *d_out = (int *)p;
    const SigmaTab sig = sigma_tab(inv_level_sigma2, kf->n_levels);
    const Batch B = {nullptr, nullptr, kf->n, nq};
    hipLaunchKernelGGL(k_grid_order, dim3((kf->n + 255) / 256), dim3(256), 0, m->stream, D, d_ord, B);
    hipLaunchKernelGGL(k_best_in_window, dim3((nq + 3) / 4), dim3(256), 0, m->stream, D, d_ord, d_q, d_qdesc, nq, chi2_gate,
                       sig, d_out, d_out + nq);
    const uint8_t *h;
    if ((rc = read_back(m, d_out, (size_t)nq * 2 * sizeof(int), &h))) return rc;
    memcpy(best_idx, h, (size_t)nq * sizeof(int));
    memcpy(best_dist, h + (size_t)nq * sizeof(int), (size_t)nq * sizeof(int));
    return ORBHIP_OK;
}

int orbhip_search_by_projection_points(orbhip_matcher *m, const orbhip_frame_view *f, const orbhip_query *q,
                                       const uint8_t *qdesc, int nq, const uint8_t *taken, int32_t *assign,
                                       float nnratio, int *nmatches)
{
    if (!m || !f || (nq > 0 && (!q || !qdesc)) || !assign || !nmatches || nq < 0) return ORBHIP_E_ARG;
    return run_search(m, 1, f, q, qdesc, nullptr, nq, taken, nnratio, 0, assign, f->n, nmatches);
}

static int search_device(orbhip_matcher *m, int mode, int pairs, const void *d_kps, const void *d_desc, const void *d_n,
                         int cap, const void *d_u_right, const void *d_taken, float min_x, float min_y, float grid_inv_w,
                         float grid_inv_h, const void *d_q, const void *d_qdesc, const void *d_nq, int qcap, float nnratio,
                         int check_ori, void *d_assign, void *d_nmatches, int t0 = 0, int ts = 1, int qd0 = 0, int qds = 1,
                         const ProjLaunch *proj = nullptr)
{
    if (!m || pairs <= 0 || !d_kps || !d_desc || !d_n || !d_q || !d_qdesc || !d_nq || !d_assign || !d_nmatches || cap <= 0 || qcap <= 0)
        return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const DevFrame D = dev_frame(cap, d_kps, d_desc, d_u_right, min_x, min_y, grid_inv_w, grid_inv_h);
    const Batch B = {(const int *)d_n, (const int *)d_nq, cap, qcap, t0, ts, qd0, qds};
    return launch_search(m, mode, pairs, D, B, (const orbhip_query *)d_q, (const uint8_t *)d_qdesc, nullptr, (const uint8_t *)d_taken,
                         nnratio, check_ori, TH_HIGH, 0, 1, (int *)d_assign, (int *)d_nmatches, window_lanes(m, mode, proj), proj);
}

int orbhip_search_by_projection_frame_device(orbhip_matcher *m, int pairs, const void *d_kps, const void *d_desc,
                                             const void *d_n, int cap, const void *d_u_right, const void *d_taken,
                                             float min_x, float min_y, float grid_inv_w, float grid_inv_h,
                                             const void *d_q, const void *d_qdesc, const void *d_nq, int qcap,
                                             int check_ori, void *d_assign, void *d_nmatches)
{
    return search_device(m, 0, pairs, d_kps, d_desc, d_n, cap, d_u_right, d_taken, min_x, min_y, grid_inv_w, grid_inv_h, d_q,
                         d_qdesc, d_nq, qcap, 0.f, check_ori, d_assign, d_nmatches);
}

int orbhip_search_by_projection_points_device(orbhip_matcher *m, int pairs, const void *d_kps, const void *d_desc,
                                              const void *d_n, int cap, const void *d_u_right, const void *d_taken,
                                              float min_x, float min_y, float grid_inv_w, float grid_inv_h,
                                              const void *d_q, const void *d_qdesc, const void *d_nq, int qcap,
                                              float nnratio, void *d_assign, void *d_nmatches)
{
    return search_device(m, 1, pairs, d_kps, d_desc, d_n, cap, d_u_right, d_taken, min_x, min_y, grid_inv_w, grid_inv_h, d_q,
                         d_qdesc, d_nq, qcap, nnratio, 0, d_assign, d_nmatches);
}

int orbhip_compute_stereo_matches_device(orbhip_matcher *m, orbhip_extractor *left, int l0, int ls,
                                         orbhip_extractor *right, int r0, int rs, int pairs, const void *d_kps_l,
                                         const void *d_desc_l, const void *d_n_l, const void *d_kps_r,
                                         const void *d_desc_r, const void *d_n_r, int cap, float mbf, float mb,
                                         void *d_u_right, void *d_depth, void *d_nmatches)
{
    if (!m || !left || !right || pairs <= 0 || cap <= 0 || !d_kps_l || !d_desc_l || !d_n_l || !d_kps_r || !d_desc_r ||
        !d_n_r || !d_u_right || !d_depth || !d_nmatches) return ORBHIP_E_ARG;
    if (!left->bound || !right->bound || left->device != m->device || right->device != m->device ||
        left->nlevels != right->nlevels || l0 < 0 || r0 < 0 || ls < 0 || rs < 0 ||
        l0 + (pairs - 1) * ls >= left->last_batch || r0 + (pairs - 1) * rs >= right->last_batch) {
        set_error("stereo: extractor handles do not hold the requested frames on device %d", m->device);
        return ORBHIP_E_ARG;
    }
    if (cap > (1 << 20)) { set_error("stereo: capacity %d exceeds the 2^20 keypoints the match key holds", cap); return ORBHIP_E_CAPACITY; }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    // mvImagePyramid[0] of handles that produce it on demand; this launch is ordered behind the copy
    if (int rc = ensure_level0(left, m->stream)) return rc;
    if (right != left) { if (int rc = ensure_level0(right, m->stream)) return rc; }
    // The REFLECT_101 frames of the levels >= 1, which an extraction does not write in full, are NOT asked for
    // (ensure_frames): no byte of them reaches a result.  k_stereo_match stages rows cv-5 .. cv+5, bytes cu-5 .. cu+6 (left)
    // and cr-10 .. cr+13 (right), and reads cr-10 .. cr+10 of the latter.  The keypoints are those of the handles'
    // extraction: 16 px inside their own level (cu in [16, w-17], cv in [16, h-17]), the right one at most one level from
    // the left one's, i.e. at 16 / 1.2 = 13.3 <= x <= w - 13.2 of the left one's level after scaling: cr in [13, w-13].
    // Every byte that is read lies in columns [3, w-3] and rows [11, h-12] of the interior; of the staged bytes only
    // cr+11 .. cr+13, which nothing reads, can reach column w, the first frame byte
    const StereoBatch B = {(const int *)d_n_l, (const int *)d_n_r, l0, ls, r0, rs, cap, 0, 0};
    return launch_stereo(m, left, 0, right, 0, pairs, B, (const orbhip_keypoint *)d_kps_l, (const uint8_t *)d_desc_l,
                         (const orbhip_keypoint *)d_kps_r, (const uint8_t *)d_desc_r, mbf, mb, (float *)d_u_right, (float *)d_depth,
                         (int *)d_nmatches);
}

int orbhip_search_for_initialization_device(orbhip_matcher *m, int pairs, const void *d_kps, const void *d_desc,
                                            const void *d_n, int cap, int f1_first, int f1_step, int f2_first,
                                            int f2_step, float min_x, float min_y, float grid_inv_w, float grid_inv_h,
                                            int reset_prev, void *d_prev_matched, int window_size, float nnratio,
                                            int check_ori, void *d_matches12, void *d_nmatches)
{
    if (!m || pairs <= 0 || cap <= 0 || !d_kps || !d_desc || !d_n || !d_prev_matched || !d_matches12 || !d_nmatches)
        return ORBHIP_E_ARG;
    if (cap > kResolveMax) {
        set_error("matcher: cap %d exceeds the LDS-resident limit %d", cap, kResolveMax);
        return ORBHIP_E_CAPACITY;
    }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    int rc;
    void *p;
    if ((rc = scratch(m, S_Q, (size_t)pairs * cap * sizeof(orbhip_query), &p))) return rc;
    orbhip_query *d_q = (orbhip_query *)p;
    if ((rc = scratch(m, S_TAKEN, (size_t)pairs * sizeof(int), &p))) return rc;
    int *d_nq = (int *)p;
    const orbhip_keypoint *keys = (const orbhip_keypoint *)d_kps;
    hipLaunchKernelGGL(k_init_queries, dim3((cap + 255) / 256, pairs), dim3(256), 0, m->stream, keys, (const int *)d_n, cap,
                       f1_first, f1_step, (float *)d_prev_matched, reset_prev, (float)window_size, d_q, d_nq);
    const DevFrame D = dev_frame(cap, keys, d_desc, nullptr, min_x, min_y, grid_inv_w, grid_inv_h);
    const Batch B = {(const int *)d_n, d_nq, cap, cap, f2_first, f2_step, f1_first, f1_step};
    if ((rc = launch_search(m, 2, pairs, D, B, d_q, (const uint8_t *)d_desc, keys, nullptr, nnratio, check_ori, TH_HIGH, 0, 0,
                            (int *)d_matches12, (int *)d_nmatches, window_lanes(m, 2))))
        return rc;
    hipLaunchKernelGGL(k_init_update_prev, dim3((cap + 255) / 256, pairs), dim3(256), 0, m->stream, keys, cap, f2_first, f2_step,
                       d_nq, (const int *)d_matches12, (float *)d_prev_matched);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_project_last_frame_device(orbhip_matcher *m, int pairs, const orbhip_camera *cam, const void *d_Tcw,
                                     const void *d_Tlw, const void *d_kps, const void *d_n, int cap, int last_first,
                                     int last_step, const void *d_world, const void *d_flags, float th, int mono,
                                     void *d_q, void *d_nq)
{
    if (!m || !cam || pairs <= 0 || cap <= 0 || !d_Tcw || !d_Tlw || !d_kps || !d_n || !d_world || !d_flags || !d_q ||
        cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS)
        return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    ProjBatch B = {(const float *)d_Tcw, (const float *)d_Tlw, (const orbhip_keypoint *)d_kps, (const int *)d_n,
                   (const float *)d_world, (const uint8_t *)d_flags, (orbhip_query *)d_q, (int *)d_nq, cap, last_first, last_step};
    hipLaunchKernelGGL(k_project_last_frame, dim3((cap + 255) / 256, pairs), dim3(256), 0, m->stream, B, *cam, th, mono);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_track_last_frame_device(orbhip_matcher *m, int pairs, const orbhip_camera *cam, const void *d_Tcw,
                                   const void *d_Tlw, const void *d_kps, const void *d_desc, const void *d_n, int cap,
                                   int cur_first, int cur_step, int last_first, int last_step, const void *d_world,
                                   const void *d_flags, const void *d_u_right, const void *d_taken, float th, int mono,
                                   int check_ori, void *d_assign, void *d_nmatches)
{
    if (!m || !cam || pairs <= 0 || cap <= 0 || !d_desc) return ORBHIP_E_ARG;
    if (!d_Tcw || !d_Tlw || !d_kps || !d_n || !d_world || !d_flags || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS)
        return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));   // before scratch(): its buffers must land on the matcher's device
    int rc;
    void *p;
    if ((rc = scratch(m, S_Q, (size_t)pairs * cap * sizeof(orbhip_query), &p))) return rc;
    orbhip_query *d_q = (orbhip_query *)p;
    if ((rc = scratch(m, S_TAKEN, (size_t)pairs * sizeof(int), &p))) return rc;   // per-pair query counts
    int *d_nq = (int *)p;
    ProjLaunch proj;
    proj.P = {(const float *)d_Tcw, (const float *)d_Tlw, (const orbhip_keypoint *)d_kps, (const int *)d_n,
              (const float *)d_world, (const uint8_t *)d_flags, d_q, d_nq, cap, last_first, last_step};
    proj.cam = *cam; proj.th = th; proj.mono = mono;
    const GridInv inv = grid_inv(cam);
    return search_device(m, 0, pairs, d_kps, d_desc, d_n, cap, d_u_right, d_taken, cam->min_x, cam->min_y, inv.w, inv.h, d_q,
                         d_desc, d_nq, cap, 0.f, check_ori, d_assign, d_nmatches, cur_first, cur_step, last_first, last_step, &proj);
}

int orbhip_frustum_queries_device(orbhip_matcher *m, int frames, const orbhip_camera *cam, const void *d_Tcw, int pcap,
                                  const void *d_np, const void *d_world, const void *d_normal, const void *d_max_dist,
                                  const void *d_min_dist, const void *d_flags, float viewing_cos_limit, float th,
                                  void *d_q, void *d_view_cos)
{
    if (!m || !cam || frames <= 0 || pcap <= 0 || !d_Tcw || !d_np || !d_world || !d_normal || !d_max_dist || !d_min_dist ||
        !d_flags || !d_q || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS)
        return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    FrustumBatch B = {(const float *)d_Tcw, (const int *)d_np, (const float *)d_world, (const float *)d_normal,
                      (const float *)d_max_dist, (const float *)d_min_dist, (const uint8_t *)d_flags, (orbhip_query *)d_q,
                      (float *)d_view_cos, pcap};
    hipLaunchKernelGGL(k_frustum_queries, dim3((pcap + 255) / 256, frames), dim3(256), 0, m->stream, B, *cam, viewing_cos_limit, th);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_project_last_frame(orbhip_matcher *m, const orbhip_camera *cam, const float *Tcw, const float *Tlw, int n,
                              const float *world, const uint8_t *flags, const orbhip_keypoint *last_keys, float th,
                              int mono, orbhip_query *q)
{
    if (!m || !cam || n < 0 || !Tcw || !Tlw || !q || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS) return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    if (!world || !flags || !last_keys) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    const float *dT, *dL, *dW;
    const uint8_t *dF;
    const orbhip_keypoint *dK;
    const int *dN;
    int rc = stage_send(m, &st, [&](Stage &stg) {
        dT = stg.put(Tcw, 12); dL = stg.put(Tlw, 12);
        dW = stg.put(world, (size_t)n * 3);
        dF = stg.put(flags, (size_t)n);
        dK = stg.put(last_keys, (size_t)n);
        dN = stg.put(&n, 1);
    });
    if (rc) return rc;
    void *p;
    if ((rc = scratch(m, S_Q, (size_t)n * sizeof(orbhip_query), &p))) return rc;
    if ((rc = orbhip_project_last_frame_device(m, 1, cam, dT, dL, dK, dN, n, 0, 0, dW, dF, th, mono, p, nullptr))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, p, (size_t)n * sizeof(orbhip_query), &h))) return rc;
    memcpy(q, h, (size_t)n * sizeof(orbhip_query));
    return ORBHIP_OK;
}

int orbhip_frustum_queries(orbhip_matcher *m, const orbhip_camera *cam, const float *Tcw, int n, const float *world,
                           const float *normal, const float *max_dist, const float *min_dist, const uint8_t *flags,
                           float viewing_cos_limit, float th, orbhip_query *q, float *view_cos)
{
    if (!m || !cam || n < 0 || !Tcw || !q || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS) return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    if (!world || !normal || !max_dist || !min_dist || !flags) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    const float *dT, *dW, *dNr, *dMx, *dMn;
    const uint8_t *dF;
    const int *dN;
    int rc = stage_send(m, &st, [&](Stage &stg) {
        dT = stg.put(Tcw, 12);
        dW = stg.put(world, (size_t)n * 3); dNr = stg.put(normal, (size_t)n * 3);
        dMx = stg.put(max_dist, (size_t)n); dMn = stg.put(min_dist, (size_t)n);
        dF = stg.put(flags, (size_t)n);
        dN = stg.put(&n, 1);
    });
    if (rc) return rc;
    // outputs contiguous: q[n] | view_cos[n] (when asked for)
    const size_t qb = (size_t)n * sizeof(orbhip_query), ob = qb + (view_cos ? (size_t)n * sizeof(float) : 0);
    void *p;
    if ((rc = scratch(m, S_OUT, ob, &p))) return rc;
    if ((rc = orbhip_frustum_queries_device(m, 1, cam, dT, n, dN, dW, dNr, dMx, dMn, dF, viewing_cos_limit, th, p,
                                            view_cos ? (uint8_t *)p + qb : nullptr)))
        return rc;
    const uint8_t *h;
    if ((rc = read_back(m, p, ob, &h))) return rc;
    memcpy(q, h, qb);
    if (view_cos) memcpy(view_cos, h + qb, (size_t)n * sizeof(float));
    return ORBHIP_OK;
}

static bool seed_args_ok(const orbhip_camera *cam, int mode, int created_flags)
{
    return cam && cam->fx != 0.f && cam->fy != 0.f && (mode == ORBHIP_SEED_ALL || mode == ORBHIP_SEED_CLOSEST) &&
           created_flags >= 0 && created_flags <= 255;
}

int orbhip_seed_stereo_points_device(orbhip_matcher *m, int frames, const orbhip_camera *cam, const void *d_Tcw, const void *d_kps,
                                     const void *d_n, int cap, int kp_first, int kp_step, const void *d_depth, float th_depth,
                                     int mode, int created_flags, void *d_world, void *d_flags, void *d_order, void *d_created,
                                     void *d_counts)
{
    if (!m || frames < 0 || cap < 1 || !seed_args_ok(cam, mode, created_flags) || !d_Tcw || !d_kps || !d_n || !d_depth ||
        !d_world || !d_flags || !d_counts || kp_first < 0 || kp_step < 0)
        return ORBHIP_E_ARG;
    if (cap > kSeedMax) { set_error("seed_stereo_points: capacity %d exceeds %d", cap, kSeedMax); return ORBHIP_E_CAPACITY; }
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const SeedBatch B = {(const float *)d_Tcw, (const orbhip_keypoint *)d_kps, (const int *)d_n, (const float *)d_depth,
                         (float *)d_world, (uint8_t *)d_flags, (int *)d_order, (uint8_t *)d_created, (int *)d_counts,
                         cap, kp_first, kp_step};
    hipLaunchKernelGGL(k_seed_stereo_points, dim3(1, frames), dim3(1024), 0, m->stream, B, cam->fx, cam->fy, cam->cx, cam->cy,
                       th_depth, mode, created_flags);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_seed_stereo_points(orbhip_matcher *m, const orbhip_camera *cam, const float *Tcw, const orbhip_keypoint *keys,
                              const float *depth, int n, float th_depth, int mode, int created_flags, float *world,
                              uint8_t *flags, int32_t *order, uint8_t *created, int32_t *counts)
{
    if (!m || !seed_args_ok(cam, mode, created_flags) || !Tcw || !counts || n < 0 ||
        (n > 0 && (!keys || !depth || !world || !flags)))
        return ORBHIP_E_ARG;
    if (n > kSeedMax) { set_error("seed_stereo_points: %d keypoints exceed %d", n, kSeedMax); return ORBHIP_E_CAPACITY; }
    counts[0] = counts[1] = counts[2] = 0;
    if (n == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    // inputs in one copy; world | flags are staged last and order | created | counts follow them, so that everything the
    // call returns comes back in one copy as well
    Stage st;
    int rc;
    const float *dT, *dZ;
    const int *dN;
    const orbhip_keypoint *dK;
    float *dW;
    uint8_t *dF, *d_created;
    int *d_order, *d_counts;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dT = stg.put(Tcw, 12);
            dN = stg.put(&n, 1);
            dK = stg.put(keys, (size_t)n);
            dZ = stg.put(depth, (size_t)n);
            dW = stg.inout(world, (size_t)n * 3);
            dF = stg.inout(flags, (size_t)n);
            d_order = stg.out((int *)nullptr, (size_t)n);   // the caller gets the first counts[1] entries, below
            d_created = created ? stg.out(created, (size_t)n) : stg.room<uint8_t>((size_t)n);
            d_counts = stg.out(counts, 3);
        }))) return rc;
    if ((rc = orbhip_seed_stereo_points_device(m, 1, cam, dT, dK, dN, n, 0, 0, dZ, th_depth, mode, created_flags, dW, dF, d_order,
                                               d_created, d_counts))) return rc;
    if ((rc = stage_fetch(m, &st))) return rc;
    if (order) memcpy(order, st.image(d_order), (size_t)counts[1] * sizeof(int));
    return ORBHIP_OK;
}

int orbhip_count_close_points_device(orbhip_matcher *m, int frames, const void *d_depth, const void *d_flags, const void *d_n,
                                     int cap, float th_depth, void *d_counts)
{
    if (!m || frames < 0 || cap < 1 || !d_depth || !d_flags || !d_n || !d_counts) return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    hipLaunchKernelGGL(k_count_close_points, dim3(frames), dim3(256), 0, m->stream, (const float *)d_depth, (const uint8_t *)d_flags,
                       (const int *)d_n, cap, th_depth, (int *)d_counts);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_count_close_points(orbhip_matcher *m, const float *depth, const uint8_t *flags, int n, float th_depth, int *tracked,
                              int *non_tracked)
{
    if (!m || n < 0 || (n > 0 && (!depth || !flags)) || !tracked || !non_tracked) return ORBHIP_E_ARG;
    *tracked = *non_tracked = 0;
    if (n == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    int rc;
    const float *dZ;
    const uint8_t *dF;
    const int *dN;
    if ((rc = stage_send(m, &st, [&](Stage &stg) { dZ = stg.put(depth, (size_t)n); dF = stg.put(flags, (size_t)n); dN = stg.put(&n, 1); })))
        return rc;
    void *p;
    if ((rc = scratch(m, S_OUT, 2 * sizeof(int), &p))) return rc;
    if ((rc = orbhip_count_close_points_device(m, 1, dZ, dF, dN, n, th_depth, p))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, p, 2 * sizeof(int), &h))) return rc;
    *tracked = reinterpret_cast<const int *>(h)[0];
    *non_tracked = reinterpret_cast<const int *>(h)[1];
    return ORBHIP_OK;
}

static bool update_args_ok(const orbhip_camera *cam, int what)
{
    if (what == 0 || (what & ~(ORBHIP_UPDATE_DESCRIPTOR | ORBHIP_UPDATE_NORMAL_DEPTH))) return false;
    if ((what & ORBHIP_UPDATE_NORMAL_DEPTH) && (!cam || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS)) return false;
    return true;
}

int orbhip_update_map_points_device(orbhip_matcher *m, const orbhip_camera *cam, int what, const void *d_Tcw, const void *d_kps,
                                    const void *d_desc, const void *d_n, int cap, const void *d_kf_bad, int np, int pcap,
                                    const void *d_obs_start, const void *d_obs_kf, const void *d_obs_idx, const void *d_ref_obs,
                                    const void *d_world, const void *d_flags, void *d_point_desc, void *d_normal,
                                    void *d_max_dist, void *d_min_dist, void *d_best_obs, void *d_status)
{
    (void)d_n;
    if (!m || !update_args_ok(cam, what) || np < 0 || np > pcap || cap < 1) return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("update_map_points: capacity %d exceeds %d", cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (np == 0) return ORBHIP_OK;
    if (!d_obs_start || !d_obs_kf || !d_obs_idx || !d_flags || !d_status) return ORBHIP_E_ARG;
    if ((what & ORBHIP_UPDATE_DESCRIPTOR) && (!d_desc || !d_point_desc)) return ORBHIP_E_ARG;
    if ((what & ORBHIP_UPDATE_NORMAL_DEPTH) &&
        (!d_Tcw || !d_kps || !d_ref_obs || !d_world || !d_normal || !d_max_dist || !d_min_dist))
        return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *work;
    if (int rc = scratch(m, S_UPD, ((size_t)np + 1) * sizeof(int), &work)) return rc;
    UpdArgs A;
    A.Tcw = (const float *)d_Tcw; A.keys = (const orbhip_keypoint *)d_kps; A.desc = (const uint8_t *)d_desc;
    A.kf_bad = (const uint8_t *)d_kf_bad;
    A.obs_start = (const int *)d_obs_start; A.obs_kf = (const int *)d_obs_kf; A.obs_idx = (const int *)d_obs_idx;
    A.ref_obs = (const int *)d_ref_obs;
    A.world = (const float *)d_world; A.flags = (const uint8_t *)d_flags;
    A.point_desc = (uint8_t *)d_point_desc; A.normal = (float *)d_normal; A.max_dist = (float *)d_max_dist;
    A.min_dist = (float *)d_min_dist; A.best_obs = (int *)d_best_obs; A.status = (uint8_t *)d_status;
    A.work = (int *)work; A.cap = cap; A.np = np; A.what = what;
    orbhip_camera c;
    memset(&c, 0, sizeof(c));
    if (cam) c = *cam;
    ORBHIP_HIP_CHECK(hipMemsetAsync(work, 0, sizeof(int), m->stream));
    hipLaunchKernelGGL(k_update_points, dim3((np + 15) / 16), dim3(256), 0, m->stream, A, c);
    hipLaunchKernelGGL(k_update_points_long, dim3(std::min(np, kUpdLongBlocks)), dim3(64), 0, m->stream, A, c);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_update_map_points(orbhip_matcher *m, const orbhip_camera *cam, int what, int K, const orbhip_frame_view *const *kfs,
                             const float *Tcw, const uint8_t *kf_bad, int np, const int32_t *obs_start, const int32_t *obs_kf,
                             const int32_t *obs_idx, const int32_t *ref_obs, const float *world, const uint8_t *flags,
                             uint8_t *point_desc, float *normal, float *max_dist, float *min_dist, int32_t *best_obs,
                             uint8_t *status)
{
    if (!m || !update_args_ok(cam, what) || K < 0 || np < 0) return ORBHIP_E_ARG;
    if (np == 0) return ORBHIP_OK;
    const bool wd = (what & ORBHIP_UPDATE_DESCRIPTOR) != 0, wn = (what & ORBHIP_UPDATE_NORMAL_DEPTH) != 0;
    if (!obs_start || !flags || !status || (K > 0 && !kfs) || (wd && !point_desc) ||
        (wn && (!ref_obs || !world || !normal || !max_dist || !min_dist || (K > 0 && !Tcw))))
        return ORBHIP_E_ARG;
    int cap = 1;
    for (int k = 0; k < K; ++k) {
        if (!kfs[k] || kfs[k]->n < 0 || (kfs[k]->n > 0 && ((wn && !kfs[k]->keys) || (wd && !kfs[k]->desc)))) return ORBHIP_E_ARG;
        cap = std::max(cap, kfs[k]->n);
    }
    if (cap > kGridMax) { set_error("update_map_points: a key frame has %d key points (limit %d)", cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (obs_start[0] < 0) return ORBHIP_E_ARG;
    for (int p = 0; p < np; ++p)
        if (obs_start[p + 1] < obs_start[p]) {
            set_error("update_map_points: obs_start must be non-decreasing (point %d)", p);
            return ORBHIP_E_ARG;
        }
    const size_t o_first = (size_t)obs_start[0], nobs = (size_t)obs_start[np];
    if (nobs > o_first && (!obs_kf || !obs_idx)) return ORBHIP_E_ARG;
    for (size_t o = o_first; o < nobs; ++o)
        if (obs_kf[o] < 0 || obs_kf[o] >= K || obs_idx[o] < 0 || obs_idx[o] >= kfs[obs_kf[o]]->n) {
            set_error("update_map_points: observation %zu (row %d, key point %d) is outside the bank", o, obs_kf[o], obs_idx[o]);
            return ORBHIP_E_ARG;
        }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    // inputs in one copy; the in/out arrays and the two reports are staged last and next to each other, so that
    // everything the call returns comes back in one copy as well
    const size_t kc = (size_t)std::max(K, 1) * cap, sn = (size_t)np;
    Stage st;
    int rc;
    const float *d_T = nullptr, *d_world = nullptr;
    const uint8_t *d_bad = nullptr, *d_desc = nullptr, *d_flags;
    const orbhip_keypoint *d_keys = nullptr;
    const int *d_ref = nullptr, *d_start, *d_okf, *d_oidx;
    uint8_t *d_pd = nullptr, *d_status;
    float *d_nrm = nullptr, *d_mx = nullptr, *d_mn = nullptr;
    int *d_best;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            if (wn) {
                d_T = stg.put(Tcw, (size_t)K * 12);
                d_keys = stg.fill<orbhip_keypoint>(kc, [&](orbhip_keypoint *h_keys) {
                    for (int k = 0; k < K; ++k)
                        if (kfs[k]->n) memcpy(h_keys + (size_t)k * cap, kfs[k]->keys, (size_t)kfs[k]->n * sizeof(orbhip_keypoint));
                });
                d_ref = stg.put(ref_obs, sn);
                d_world = stg.put(world, sn * 3);
            }
            if (wd)
                d_desc = stg.fill<uint8_t>(kc * 32, [&](uint8_t *h_desc) {
                    for (int k = 0; k < K; ++k)
                        if (kfs[k]->n) memcpy(h_desc + (size_t)k * cap * 32, kfs[k]->desc, (size_t)kfs[k]->n * 32);
                });
            if (kf_bad) d_bad = stg.put(kf_bad, (size_t)K);
            d_start = stg.put(obs_start, sn + 1);
            d_okf = stg.put(obs_kf, nobs); d_oidx = stg.put(obs_idx, nobs);
            d_flags = stg.put(flags, sn);
            // outputs: point_desc | normal | max_dist | min_dist | best_obs | status
            if (wd) d_pd = stg.inout(point_desc, sn * 32);
            if (wn) { d_nrm = stg.inout(normal, sn * 3); d_mx = stg.inout(max_dist, sn); d_mn = stg.inout(min_dist, sn); }
            d_best = stg.fill<int>(sn, [&](int *h_best) { for (size_t i = 0; i < sn; ++i) h_best[i] = -1; });
            if (best_obs && wd) stg.back(best_obs, d_best, sn);
            d_status = stg.fill<uint8_t>(sn, [&](uint8_t *h_status) { memset(h_status, 0, sn); });
            stg.back(status, d_status, sn);
        }))) return rc;
    if ((rc = orbhip_update_map_points_device(m, cam, what, d_T, d_keys, d_desc, nullptr, cap, d_bad, np, np, d_start, d_okf, d_oidx,
                                              d_ref, d_world, d_flags, d_pd, d_nrm, d_mx, d_mn, d_best, d_status))) return rc;
    return stage_fetch(m, &st);
}

// ---- local map (kernels: orbhip_localmap.hip) -----------------------------------------------------------------------
static int local_map_args(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap, const orbhip_local_map_tables *t,
                          const orbhip_local_map_io *io)
{
    if (!m || !t || !io || frames < 0 || rows < 0 || np < 0 || pcap < 0 || np > pcap || cap < 1) return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("update_local_map: capacity %d exceeds %d", cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (rows > 65536) { set_error("update_local_map: %d bank rows exceed 65536", rows); return ORBHIP_E_CAPACITY; }
    if (!t->slot_point || !t->n || !t->covis || !t->child_start || !t->child || !t->parent || !t->obs_start || !t->obs_kf ||
        !t->flags || !t->world || !t->normal || !t->max_dist || !t->min_dist || !t->point_desc || !io->frame_point ||
        !io->frame_n || !io->local_kf || !io->n_local_kf || !io->votes || !io->local_point || !io->world_l || !io->normal_l ||
        !io->max_dist_l || !io->min_dist_l || !io->desc_l || !io->flags_l || !io->np_l || !io->taken || !io->report)
        return ORBHIP_E_ARG;
    return ORBHIP_OK;
}

int orbhip_update_local_map_device(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap,
                                   const orbhip_local_map_tables *t, const orbhip_local_map_io *io)
{
    if (int rc = local_map_args(m, frames, rows, cap, np, pcap, t, io)) return rc;
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *work;
    if (int rc = scratch(m, S_LMAP, local_map_workspace_bytes(frames, rows, pcap), &work)) return rc;
    LocalMapArgs A;
    memset(&A, 0, sizeof(A));
    A.slot_point = (const int *)t->slot_point; A.n = (const int *)t->n; A.kf_bad = (const uint8_t *)t->kf_bad;
    A.covis = (const int *)t->covis; A.child_start = (const int *)t->child_start; A.child = (const int *)t->child;
    A.parent = (const int *)t->parent; A.obs_start = (const int *)t->obs_start; A.obs_kf = (const int *)t->obs_kf;
    A.flags = (const uint8_t *)t->flags; A.world = (const float *)t->world; A.normal = (const float *)t->normal;
    A.max_dist = (const float *)t->max_dist; A.min_dist = (const float *)t->min_dist; A.point_desc = (const uint8_t *)t->point_desc;
    A.frame_point = (int *)io->frame_point; A.frame_n = (const int *)io->frame_n; A.local_kf = (int *)io->local_kf;
    A.n_local_kf = (int *)io->n_local_kf; A.votes = (int *)io->votes; A.local_point = (int *)io->local_point;
    A.world_l = (float *)io->world_l; A.normal_l = (float *)io->normal_l; A.max_dist_l = (float *)io->max_dist_l;
    A.min_dist_l = (float *)io->min_dist_l; A.desc_l = (uint8_t *)io->desc_l; A.flags_l = (uint8_t *)io->flags_l;
    A.np_l = (int *)io->np_l; A.taken = (uint8_t *)io->taken; A.report = (int *)io->report;
    A.frames = frames; A.rows = rows; A.cap = cap; A.pcap = pcap;
    return launch_local_map(m->stream, A, work);
}

int orbhip_track_local_map_device(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap,
                                  const orbhip_local_map_tables *t, const orbhip_local_map_io *io, const orbhip_camera *cam,
                                  const orbhip_local_map_track *tr, float viewing_cos_limit, float th, float nnratio)
{
    if (int rc = local_map_args(m, frames, rows, cap, np, pcap, t, io)) return rc;
    if (!cam || !tr || pcap < 1 || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS || !tr->Tcw || !tr->kps || !tr->desc ||
        !tr->q || !tr->assign || !tr->nmatches)
        return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    int rc;
    if ((rc = orbhip_update_local_map_device(m, frames, rows, cap, np, pcap, t, io))) return rc;
    if ((rc = orbhip_frustum_queries_device(m, frames, cam, tr->Tcw, pcap, io->np_l, io->world_l, io->normal_l, io->max_dist_l,
                                            io->min_dist_l, io->flags_l, viewing_cos_limit, th, tr->q, nullptr))) return rc;
    const GridInv inv = grid_inv(cam);
    if ((rc = orbhip_search_by_projection_points_device(m, frames, tr->kps, tr->desc, io->frame_n, cap, tr->u_right, io->taken,
                                                        cam->min_x, cam->min_y, inv.w, inv.h, tr->q, io->desc_l, io->np_l, pcap,
                                                        nnratio, tr->assign, tr->nmatches))) return rc;
    return launch_local_map_apply(m->stream, frames, cap, pcap, tr->q, (const int *)io->np_l, (const int *)io->frame_n,
                                  (const int *)tr->assign, (const int *)io->local_point, (int *)io->frame_point, (int *)io->report);
}

// a CSR offsets array: starts at or above 0 and does not decrease
static bool csr_ok(const int32_t *start, int count, const char *what)
{
    if (start[0] < 0) { set_error("update_local_map: %s starts below 0", what); return false; }
    for (int i = 0; i < count; ++i)
        if (start[i + 1] < start[i]) { set_error("update_local_map: %s must be non-decreasing (entry %d)", what, i); return false; }
    return true;
}

int orbhip_update_local_map(orbhip_matcher *m, int frames, int rows, int cap, int np, int pcap,
                            const orbhip_local_map_tables *t, const orbhip_local_map_io *io)
{
    if (int rc = local_map_args(m, frames, rows, cap, np, pcap, t, io)) return rc;
    if (frames == 0) return ORBHIP_OK;
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n, *covis = (const int32_t *)t->covis;
    const int32_t *child_start = (const int32_t *)t->child_start, *child = (const int32_t *)t->child, *parent = (const int32_t *)t->parent;
    const int32_t *obs_start = (const int32_t *)t->obs_start, *obs_kf = (const int32_t *)t->obs_kf;
    const int32_t *frame_point = (const int32_t *)io->frame_point, *frame_n = (const int32_t *)io->frame_n;
    const int32_t *local_kf = (const int32_t *)io->local_kf, *n_local_kf = (const int32_t *)io->n_local_kf;
    if (!csr_ok(child_start, rows, "child_start") || !csr_ok(obs_start, np, "obs_start")) return ORBHIP_E_ARG;
    const size_t nchild = (size_t)child_start[rows], nobs = (size_t)obs_start[np];
    auto row_ok = [rows](int r) { return r >= 0 && r < rows; };
    for (int r = 0; r < rows; ++r) {
        bool ok = n[r] >= 0 && n[r] <= cap && parent[r] >= -1 && parent[r] < rows;
        for (int j = 0; ok && j < 10; ++j) ok = covis[(size_t)r * 10 + j] >= -1 && covis[(size_t)r * 10 + j] < rows;
        for (int i = 0; ok && i < n[r]; ++i) ok = slot_point[(size_t)r * cap + i] >= -1 && slot_point[(size_t)r * cap + i] < np;
        if (!ok) { set_error("update_local_map: bank row %d holds a count, row or point index out of range", r); return ORBHIP_E_ARG; }
    }
    for (size_t o = 0; o < nchild; ++o)
        if (!row_ok(child[o])) { set_error("update_local_map: child %zu (row %d) is outside the bank", o, child[o]); return ORBHIP_E_ARG; }
    for (size_t o = 0; o < nobs; ++o)
        if (!row_ok(obs_kf[o])) { set_error("update_local_map: observation %zu (row %d) is outside the bank", o, obs_kf[o]); return ORBHIP_E_ARG; }
    for (int f = 0; f < frames; ++f) {
        bool ok = frame_n[f] >= 0 && frame_n[f] <= cap && n_local_kf[f] >= 0 && n_local_kf[f] <= rows;
        for (int i = 0; ok && i < frame_n[f]; ++i) ok = frame_point[(size_t)f * cap + i] >= -1 && frame_point[(size_t)f * cap + i] < np;
        for (int i = 0; ok && i < n_local_kf[f]; ++i) ok = row_ok(local_kf[(size_t)f * rows + i]);
        if (!ok) { set_error("update_local_map: frame %d holds a count, row or point index out of range", f); return ORBHIP_E_ARG; }
    }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t R = (size_t)rows, Cp = (size_t)cap, P = (size_t)pcap, Fr = (size_t)frames;
    Stage st;
    int rc;
    orbhip_local_map_tables dt;
    orbhip_local_map_io dio;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dt.slot_point = stg.put(slot_point, R * Cp);
            dt.n = stg.put(n, R);
            dt.kf_bad = t->kf_bad ? stg.put((const uint8_t *)t->kf_bad, R) : nullptr;
            dt.covis = stg.put(covis, R * 10);
            dt.child_start = stg.put(child_start, R + 1);
            dt.child = stg.put(child, nchild);
            dt.parent = stg.put(parent, R);
            dt.obs_start = stg.put(obs_start, (size_t)np + 1);
            dt.obs_kf = stg.put(obs_kf, nobs);
            dt.flags = stg.put((const uint8_t *)t->flags, P);
            dt.world = stg.put((const float *)t->world, P * 3);
            dt.normal = stg.put((const float *)t->normal, P * 3);
            dt.max_dist = stg.put((const float *)t->max_dist, P);
            dt.min_dist = stg.put((const float *)t->min_dist, P);
            dt.point_desc = stg.put((const uint8_t *)t->point_desc, P * 32);
            dio.frame_n = stg.put(frame_n, Fr);
            // in/out and output arrays next to each other, as the caller passed them: one copy brings all of them back
            auto out = [&](void *host, size_t bytes) { return stg.inout((uint8_t *)host, bytes); };
            dio.frame_point = out(io->frame_point, Fr * Cp * 4);
            dio.local_kf = out(io->local_kf, Fr * R * 4);
            dio.n_local_kf = out(io->n_local_kf, Fr * 4);
            dio.votes = out(io->votes, Fr * R * 4);
            dio.local_point = out(io->local_point, Fr * P * 4);
            dio.world_l = out(io->world_l, Fr * P * 12);
            dio.normal_l = out(io->normal_l, Fr * P * 12);
            dio.max_dist_l = out(io->max_dist_l, Fr * P * 4);
            dio.min_dist_l = out(io->min_dist_l, Fr * P * 4);
            dio.desc_l = out(io->desc_l, Fr * P * 32);
            dio.flags_l = out(io->flags_l, Fr * P);
            dio.np_l = out(io->np_l, Fr * 4);
            dio.taken = out(io->taken, Fr * Cp);
            dio.report = out(io->report, Fr * 32);
        }))) return rc;
    if ((rc = orbhip_update_local_map_device(m, frames, rows, cap, np, pcap, &dt, &dio))) return rc;
    return stage_fetch(m, &st);
}

// ---- covisibility graph (kernels: orbhip_covisibility.hip) ------------------------------------------------------------
static constexpr int kCovisMaxRows = 4096;

// what both forms of orbhip_update_connections check, the handle aside
static int update_connections_args(int rows, int cap, int np, int pcap, const orbhip_covis_tables *t, const orbhip_covis_state *s,
                                   int id0_row, int U, const void *update_rows, const void *report)
{
    if (!t || !s || rows < 0 || np < 0 || pcap < 0 || np > pcap || cap < 1 || U < 0 || id0_row < -1 || id0_row >= std::max(rows, 0))
        return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("update_connections: capacity %d exceeds %d", cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (rows > kCovisMaxRows) { set_error("update_connections: %d bank rows exceed %d", rows, kCovisMaxRows); return ORBHIP_E_CAPACITY; }
    if (U > 65536) { set_error("update_connections: %d list entries exceed 65536", U); return ORBHIP_E_CAPACITY; }
    if (!t->slot_point || !t->n || !t->obs_start || !t->obs_kf || !t->flags || !s->conn_w || !s->ord_kf || !s->ord_w || !s->n_ord ||
        !s->covis || !s->first_conn || !s->parent || !update_rows || !report)
        return ORBHIP_E_ARG;
    return ORBHIP_OK;
}

static int update_connections_launch(orbhip_matcher *m, int rows, int cap, int np, const orbhip_covis_tables *t,
                                     const orbhip_covis_state *s, const int *d_row_slot, int id0_row, int U, const void *d_update_rows,
                                     void *d_report)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *work;
    if (int rc = scratch(m, S_COVIS, covis_workspace_bytes(U, rows), &work)) return rc;
    CovisArgs A;
    memset(&A, 0, sizeof(A));
    A.slot_point = (const int *)t->slot_point; A.n = (const int *)t->n; A.obs_start = (const int *)t->obs_start;
    A.obs_kf = (const int *)t->obs_kf; A.flags = (const uint8_t *)t->flags;
    A.conn_w = (int *)s->conn_w; A.ord_kf = (int *)s->ord_kf; A.ord_w = (int *)s->ord_w; A.n_ord = (int *)s->n_ord;
    A.covis = (int *)s->covis; A.first_conn = (uint8_t *)s->first_conn; A.parent = (int *)s->parent;
    A.row_slot = d_row_slot; A.update_rows = (const int *)d_update_rows; A.report = (int *)d_report;
    A.rows = rows; A.cap = cap; A.np = np; A.id0_row = id0_row; A.U = U;
    return launch_update_connections(m->stream, A, work);
}

int orbhip_update_connections_device(orbhip_matcher *m, int rows, int cap, int np, int pcap, const orbhip_covis_tables *t,
                                     const orbhip_covis_state *s, int id0_row, int U, const void *d_update_rows, void *d_report)
{
    if (int rc = update_connections_args(rows, cap, np, pcap, t, s, id0_row, U, d_update_rows, d_report)) return rc;
    if (!m) return ORBHIP_E_ARG;
    if (U == 0 || rows == 0) return ORBHIP_OK;
    return update_connections_launch(m, rows, cap, np, t, s, nullptr, id0_row, U, d_update_rows, d_report);
}

int orbhip_update_connections(orbhip_matcher *m, int rows, int cap, int np, int pcap, const orbhip_covis_tables *t,
                              const orbhip_covis_state *s, int id0_row, int U, const int32_t *update_rows, int32_t *report)
{
    if (int rc = update_connections_args(rows, cap, np, pcap, t, s, id0_row, U, update_rows, report)) return rc;
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n;
    const int32_t *obs_start = (const int32_t *)t->obs_start, *obs_kf = (const int32_t *)t->obs_kf;
    const uint8_t *flags = (const uint8_t *)t->flags;
    int32_t *conn_w = (int32_t *)s->conn_w, *ord_kf = (int32_t *)s->ord_kf, *ord_w = (int32_t *)s->ord_w, *n_ord = (int32_t *)s->n_ord;
    int32_t *covis = (int32_t *)s->covis, *parent = (int32_t *)s->parent;
    uint8_t *first_conn = (uint8_t *)s->first_conn;
    if (obs_start[0] < 0) { set_error("update_connections: obs_start starts below 0"); return ORBHIP_E_ARG; }
    for (int p = 0; p < np; ++p)
        if (obs_start[p + 1] < obs_start[p]) { set_error("update_connections: obs_start must be non-decreasing (entry %d)", p); return ORBHIP_E_ARG; }
    const size_t nobs = (size_t)obs_start[np];
    for (size_t o = 0; o < nobs; ++o)
        if (obs_kf[o] < 0 || obs_kf[o] >= rows) { set_error("update_connections: observation %zu (row %d) is outside the bank", o, obs_kf[o]); return ORBHIP_E_ARG; }
    for (int r = 0; r < rows; ++r) {
        if (n[r] < 0 || n[r] > cap) { set_error("update_connections: bank row %d holds a count outside [0, cap]", r); return ORBHIP_E_ARG; }
        if (n_ord[r] < 0 || n_ord[r] > rows) { set_error("update_connections: n_ord of bank row %d is outside [0, rows]", r); return ORBHIP_E_ARG; }
    }
    // the rows the call can reach: the updated rows and the rows their points' observations name
    std::vector<int32_t> row_slot((size_t)rows, -1), resident;
    auto reach = [&](int r) { if (row_slot[r] < 0) { row_slot[r] = (int32_t)resident.size(); resident.push_back(r); } };
    for (int u = 0; u < U; ++u) {
        const int r = update_rows[u];
        if (r < 0 || r >= rows) { set_error("update_connections: list entry %d (row %d) is outside the bank", u, r); return ORBHIP_E_ARG; }
        if (row_slot[r] >= 0) continue;                           // a repeat, or a row a point of an earlier entry named
        reach(r);
    }
    const size_t n_updated = resident.size();                     // the updated rows come first
    for (size_t k = 0; k < n_updated; ++k) {
        const int r = resident[k];
        for (int i = 0; i < n[r]; ++i) {
            const int p = slot_point[(size_t)r * cap + i];
            if (p < -1 || p >= np) { set_error("update_connections: bank row %d holds a point index out of range", r); return ORBHIP_E_ARG; }
            if (p < 0 || !(flags[p] & ORBHIP_POINT_PRESENT)) continue;
            for (int o = obs_start[p]; o < obs_start[p + 1]; ++o) reach(obs_kf[o]);
        }
    }
    if (!m) return ORBHIP_E_ARG;
    if (U == 0 || rows == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t R = (size_t)rows, Cp = (size_t)cap, T = resident.size(), Un = (size_t)U;
    Stage st;
    int rc;
    orbhip_covis_tables dt;
    orbhip_covis_state ds;
    const int32_t *d_row_slot, *d_update;
    int32_t *d_cw, *d_okf, *d_ow, *d_no, *d_cv, *d_par, *d_rep;
    uint8_t *d_fc;
    // a state table's resident rows, `width` T each, gathered into a piece that travels back for the scatter below
    auto gather = [&](Stage &st, auto *table, size_t width) {
        using E = std::remove_pointer_t<decltype(table)>;
        E *d = st.fill<E>(T * width, [&](E *h) {
            for (size_t k = 0; k < T; ++k) memcpy(h + k * width, table + (size_t)resident[k] * width, width * sizeof(E));
        });
        st.back((E *)nullptr, d, T * width);
        return d;
    };
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_row_slot = stg.put(row_slot.data(), R);
            // slot rows of the updated rows only: they hold the first slots
            dt.slot_point = stg.fill<int32_t>(n_updated * Cp, [&](int32_t *h) {
                for (size_t k = 0; k < n_updated; ++k) memcpy(h + k * Cp, slot_point + (size_t)resident[k] * Cp, Cp * 4);
            });
            dt.n = stg.fill<int32_t>(T, [&](int32_t *h) { for (size_t k = 0; k < T; ++k) h[k] = n[resident[k]]; });
            dt.obs_start = stg.put(obs_start, (size_t)np + 1);
            dt.obs_kf = stg.put(obs_kf, nobs);
            dt.flags = stg.put(flags, (size_t)np);
            d_update = stg.put(update_rows, Un);
            // the state rows and the report next to each other: one copy brings all of them back
            ds.conn_w = d_cw = gather(stg, conn_w, R); ds.ord_kf = d_okf = gather(stg, ord_kf, R); ds.ord_w = d_ow = gather(stg, ord_w, R);
            ds.n_ord = d_no = gather(stg, n_ord, 1); ds.covis = d_cv = gather(stg, covis, 10);
            ds.first_conn = d_fc = gather(stg, first_conn, 1);
            ds.parent = d_par = gather(stg, parent, 1);
            d_rep = stg.out(report, Un * 8);
        }))) return rc;
    if ((rc = update_connections_launch(m, rows, cap, np, &dt, &ds, d_row_slot, id0_row, U, d_update, d_rep))) return rc;
    if ((rc = stage_fetch(m, &st))) return rc;
    auto scatter = [&](auto *table, const auto *d, size_t width) {
        for (size_t k = 0; k < T; ++k) memcpy(table + (size_t)resident[k] * width, st.image(d) + k * width, width * sizeof(*table));
    };
    scatter(conn_w, d_cw, R); scatter(ord_kf, d_okf, R); scatter(ord_w, d_ow, R); scatter(n_ord, d_no, 1); scatter(covis, d_cv, 10);
    scatter(first_conn, d_fc, 1); scatter(parent, d_par, 1);
    return ORBHIP_OK;
}

static int covisible_targets_args(int rows, const void *ord_kf, const void *n_ord, int Q, const void *cur, int nn, int nn2,
                                  const void *targets, const void *counts)
{
    if (rows < 0 || Q < 0 || nn < 1 || nn2 < 0 || nn > kCovisMaxRows || nn2 > kCovisMaxRows || !ord_kf || !n_ord || !cur || !targets ||
        !counts)
        return ORBHIP_E_ARG;
    if (rows > kCovisMaxRows) { set_error("covisible_targets: %d bank rows exceed %d", rows, kCovisMaxRows); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

int orbhip_covisible_targets_device(orbhip_matcher *m, int rows, const void *d_ord_kf, const void *d_n_ord, const void *d_kf_bad,
                                    int Q, const void *d_cur, int nn, int nn2, void *d_targets, void *d_counts)
{
    if (int rc = covisible_targets_args(rows, d_ord_kf, d_n_ord, Q, d_cur, nn, nn2, d_targets, d_counts)) return rc;
    if (!m) return ORBHIP_E_ARG;
    if (Q == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    CovisTargetArgs A;
    A.ord_kf = (const int *)d_ord_kf; A.n_ord = (const int *)d_n_ord; A.row_slot = nullptr; A.kf_bad = (const uint8_t *)d_kf_bad;
    A.cur = (const int *)d_cur; A.targets = (int *)d_targets; A.counts = (int *)d_counts;
    A.rows = rows; A.stride = rows; A.nn = nn; A.nn2 = nn2;
    return launch_covisible_targets(m->stream, A, Q);
}

int orbhip_covisible_targets(orbhip_matcher *m, int rows, const int32_t *ord_kf, const int32_t *n_ord, const uint8_t *kf_bad, int Q,
                             const int32_t *cur, int nn, int nn2, int32_t *targets, int32_t *counts)
{
    if (int rc = covisible_targets_args(rows, ord_kf, n_ord, Q, cur, nn, nn2, targets, counts)) return rc;
    // the lists it walks: those of the current rows and, for the fuse targets, of their first nn entries
    std::vector<int32_t> row_slot((size_t)rows, -1), resident;
    auto reach = [&](int r, const char *what) {
        if (r < 0 || r >= rows) { set_error("covisible_targets: %s (row %d) is outside the bank", what, r); return false; }
        if (n_ord[r] < 0 || n_ord[r] > rows) { set_error("covisible_targets: n_ord of bank row %d is outside [0, rows]", r); return false; }
        if (row_slot[r] < 0) { row_slot[r] = (int32_t)resident.size(); resident.push_back(r); }
        return true;
    };
    for (int q = 0; q < Q; ++q) {
        if (!reach(cur[q], "a current row")) return ORBHIP_E_ARG;
        const int c = cur[q];
        for (int v = 0; v < std::min(n_ord[c], nn); ++v) {
            const int a = ord_kf[(size_t)c * rows + v];
            if (!reach(a, "a first neighbour")) return ORBHIP_E_ARG;
            for (int v2 = 0; nn2 > 0 && v2 < std::min(n_ord[a], nn2); ++v2) {
                const int k2 = ord_kf[(size_t)a * rows + v2];
                if (k2 < 0 || k2 >= rows) { set_error("covisible_targets: a second neighbour (row %d) is outside the bank", k2); return ORBHIP_E_ARG; }
            }
        }
    }
    if (!m) return ORBHIP_E_ARG;
    if (Q == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t R = (size_t)rows, T = resident.size(), W = (size_t)std::min(std::max(nn, nn2), rows), Qn = (size_t)Q;
    const size_t out_cap = (size_t)nn * (1 + (size_t)nn2);
    Stage st;
    int rc;
    CovisTargetArgs A;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            A.row_slot = stg.put(row_slot.data(), R);
            A.ord_kf = stg.fill<int32_t>(T * W, [&](int32_t *h_head) {
                for (size_t k = 0; k < T; ++k) memcpy(h_head + k * W, ord_kf + (size_t)resident[k] * R, W * 4);
            });
            A.n_ord = stg.fill<int32_t>(T, [&](int32_t *h_no) { for (size_t k = 0; k < T; ++k) h_no[k] = n_ord[resident[k]]; });
            A.kf_bad = kf_bad ? stg.put(kf_bad, R) : nullptr;
            A.cur = stg.put(cur, Qn);
            A.targets = stg.out(targets, Qn * out_cap);
            A.counts = stg.out(counts, Qn);
        }))) return rc;
    A.rows = rows; A.stride = (int)W; A.nn = nn; A.nn2 = nn2;
    if ((rc = launch_covisible_targets(m->stream, A, Q))) return rc;
    return stage_fetch(m, &st);
}

int orbhip_children_from_parents_device(orbhip_matcher *m, int rows, const void *d_parent, const void *d_kf_bad, void *d_child_start,
                                        void *d_child)
{
    if (rows < 0 || !d_parent || !d_child_start || !d_child) return ORBHIP_E_ARG;
    if (rows > kCovisMaxRows) { set_error("children_from_parents: %d bank rows exceed %d", rows, kCovisMaxRows); return ORBHIP_E_CAPACITY; }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    return launch_children_from_parents(m->stream, rows, (const int *)d_parent, (const uint8_t *)d_kf_bad, (int *)d_child_start,
                                        (int *)d_child);
}

// ---- culling (kernels: orbhip_culling.hip) ----------------------------------------------------------------------------
// what every form of the two culling entries checks, the handle aside; kf: orbhip_cull_key_frames*
static int cull_args(const char *who, bool kf, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t,
                     const orbhip_cull_io *io)
{
    if (!t || !io || rows < 0 || np < 0 || pcap < 0 || np > pcap || cap < 1 || obs_cap < 0) return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("%s: capacity %d exceeds %d", who, cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (rows > kCovisMaxRows) { set_error("%s: %d bank rows exceed %d", who, rows, kCovisMaxRows); return ORBHIP_E_CAPACITY; }
    if (!t->obs_start || !t->obs_kf || !t->obs_idx || !t->ref_obs || !io->slot_point || !io->flags || !io->obs_start_out ||
        !io->obs_kf_out || !io->obs_idx_out || !io->ref_obs_out)
        return ORBHIP_E_ARG;
    if (io->obs_start_out == t->obs_start || io->obs_kf_out == t->obs_kf || io->obs_idx_out == t->obs_idx || io->ref_obs_out == t->ref_obs) {
        set_error("%s: the observation table out must not alias the table in", who);
        return ORBHIP_E_ARG;
    }
    if (kf && (!t->kps || !t->n || !io->kf_bad || !io->child_start || !io->child || (t->not_erase && !io->to_be_erased)))
        return ORBHIP_E_ARG;
    return ORBHIP_OK;
}

static void cull_common(CullArgs &A, int rows, int cap, int np, int obs_cap, const orbhip_cull_tables *t, const orbhip_cull_io *io)
{
    memset(&A, 0, sizeof(A));
    A.kps = (const orbhip_keypoint *)t->kps; A.u_right = (const float *)t->u_right; A.depth = (const float *)t->depth;
    A.n = (const int *)t->n; A.obs_start = (const int *)t->obs_start; A.obs_kf = (const int *)t->obs_kf;
    A.obs_idx = (const int *)t->obs_idx; A.ref_obs = (const int *)t->ref_obs; A.not_erase = (const uint8_t *)t->not_erase;
    A.slot_point = (int *)io->slot_point; A.flags = (uint8_t *)io->flags; A.kf_bad = (uint8_t *)io->kf_bad;
    A.to_be_erased = (uint8_t *)io->to_be_erased; A.child_start = (int *)io->child_start; A.child = (int *)io->child;
    A.obs_start_out = (int *)io->obs_start_out; A.obs_kf_out = (int *)io->obs_kf_out; A.obs_idx_out = (int *)io->obs_idx_out;
    A.ref_obs_out = (int *)io->ref_obs_out;
    A.rows = rows; A.cap = cap; A.np = np; A.obs_cap = obs_cap; A.id0_row = -1;
}

static int cull_map_points_args(int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t, const orbhip_cull_io *io,
                                int R, const void *recent, const void *found, const void *visible, const void *first_kf_id, int th_obs,
                                const void *recent_out, const void *n_recent_out, const void *status)
{
    if (int rc = cull_args("cull_map_points", false, rows, cap, np, pcap, obs_cap, t, io)) return rc;
    if (R < 0 || th_obs < 0 || !recent || !found || !visible || !first_kf_id || !recent_out || !n_recent_out || !status) return ORBHIP_E_ARG;
    return ORBHIP_OK;
}

static int cull_map_points_launch(orbhip_matcher *m, int rows, int cap, int np, int obs_cap, const orbhip_cull_tables *t,
                                  const orbhip_cull_io *io, int R, const void *d_recent, const void *d_found, const void *d_visible,
                                  const void *d_first_kf_id, int cur_kf_id, int th_obs, void *d_recent_out, void *d_n_recent_out,
                                  void *d_status)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *work;
    if (int rc = scratch(m, S_CULL, cull_workspace_bytes(np, obs_cap, 0), &work)) return rc;
    CullArgs A;
    cull_common(A, rows, cap, np, obs_cap, t, io);
    A.recent = (const int *)d_recent; A.found = (const int *)d_found; A.visible = (const int *)d_visible;
    A.first_kf_id = (const int *)d_first_kf_id; A.recent_out = (int *)d_recent_out; A.n_recent_out = (int *)d_n_recent_out;
    A.status = (uint8_t *)d_status; A.R = R; A.cur_kf_id = cur_kf_id; A.th_obs = th_obs;
    return launch_cull_map_points(m->stream, A, work);
}

int orbhip_cull_map_points_device(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t,
                                  const orbhip_cull_io *io, int R, const void *d_recent, const void *d_found, const void *d_visible,
                                  const void *d_first_kf_id, int cur_kf_id, int th_obs, void *d_recent_out, void *d_n_recent_out,
                                  void *d_status)
{
    if (int rc = cull_map_points_args(rows, cap, np, pcap, obs_cap, t, io, R, d_recent, d_found, d_visible, d_first_kf_id, th_obs,
                                      d_recent_out, d_n_recent_out, d_status))
        return rc;
    if (!m) return ORBHIP_E_ARG;
    return cull_map_points_launch(m, rows, cap, np, obs_cap, t, io, R, d_recent, d_found, d_visible, d_first_kf_id, cur_kf_id, th_obs,
                                  d_recent_out, d_n_recent_out, d_status);
}

static int cull_key_frames_args(int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t, const orbhip_cull_io *io,
                                const orbhip_covis_state *s, int id0_row, int U, const void *cand, int mono, const void *report)
{
    if (int rc = cull_args("cull_key_frames", true, rows, cap, np, pcap, obs_cap, t, io)) return rc;
    if (!s || U < 0 || id0_row < -1 || id0_row >= std::max(rows, 0) || !cand || !report || (!mono && !t->depth)) return ORBHIP_E_ARG;
    if (U > 65536) { set_error("cull_key_frames: %d candidates exceed 65536", U); return ORBHIP_E_CAPACITY; }
    if (!s->conn_w || !s->ord_kf || !s->ord_w || !s->n_ord || !s->covis || !s->parent) return ORBHIP_E_ARG;
    return ORBHIP_OK;
}

static int cull_key_frames_launch(orbhip_matcher *m, int rows, int cap, int np, int obs_cap, const orbhip_cull_tables *t,
                                  const orbhip_cull_io *io, const orbhip_covis_state *s, int id0_row, int U, const void *d_cand, int mono,
                                  float th_depth, void *d_report)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *work;
    if (int rc = scratch(m, S_CULL, cull_workspace_bytes(np, obs_cap, U), &work)) return rc;
    CullArgs A;
    cull_common(A, rows, cap, np, obs_cap, t, io);
    A.conn_w = (int *)s->conn_w; A.ord_kf = (int *)s->ord_kf; A.ord_w = (int *)s->ord_w; A.n_ord = (int *)s->n_ord;
    A.covis = (int *)s->covis; A.parent = (int *)s->parent;
    A.cand_in = (const int *)d_cand; A.report = (int *)d_report; A.id0_row = id0_row; A.U = U; A.mono = mono != 0; A.th_depth = th_depth;
    return launch_cull_key_frames(m->stream, A, work);
}

int orbhip_cull_key_frames_device(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t,
                                  const orbhip_cull_io *io, const orbhip_covis_state *s, int id0_row, int U, const void *d_cand, int mono,
                                  float th_depth, void *d_report)
{
    if (int rc = cull_key_frames_args(rows, cap, np, pcap, obs_cap, t, io, s, id0_row, U, d_cand, mono, d_report)) return rc;
    if (!m) return ORBHIP_E_ARG;
    return cull_key_frames_launch(m, rows, cap, np, obs_cap, t, io, s, id0_row, U, d_cand, mono, th_depth, d_report);
}

// what the host forms range-check in the tables both calls share; *total = obs_start[np]
static int cull_check_tables(const char *who, int rows, int cap, int np, int obs_cap, const orbhip_cull_tables *t, const orbhip_cull_io *io,
                             size_t *total)
{
    const int32_t *obs_start = (const int32_t *)t->obs_start, *obs_kf = (const int32_t *)t->obs_kf, *obs_idx = (const int32_t *)t->obs_idx;
    if (obs_start[0] != 0) { set_error("%s: obs_start must start at 0", who); return ORBHIP_E_ARG; }
    for (int p = 0; p < np; ++p)
        if (obs_start[p + 1] < obs_start[p]) { set_error("%s: obs_start must be non-decreasing (entry %d)", who, p); return ORBHIP_E_ARG; }
    if (obs_start[np] > obs_cap) { set_error("%s: the table holds %d entries, obs_cap is %d", who, obs_start[np], obs_cap); return ORBHIP_E_ARG; }
    *total = (size_t)obs_start[np];
    std::vector<int32_t> seen((size_t)rows, -1);
    for (int p = 0; p < np; ++p)
        for (int o = obs_start[p]; o < obs_start[p + 1]; ++o) {
            const int k = obs_kf[o];
            if (k < 0 || k >= rows || obs_idx[o] < 0 || obs_idx[o] >= cap) { set_error("%s: observation %d (row %d, key point %d) is outside the bank", who, o, k, obs_idx[o]); return ORBHIP_E_ARG; }
            if (seen[k] == p) { set_error("%s: the list of point %d names bank row %d twice", who, p, k); return ORBHIP_E_ARG; }
            seen[k] = p;
        }
    const int32_t *slot_point = (const int32_t *)io->slot_point;
    for (size_t i = 0; i < (size_t)rows * cap; ++i)
        if (slot_point[i] < -1 || slot_point[i] >= np) { set_error("%s: bank row %zu holds a point index out of range", who, i / cap); return ORBHIP_E_ARG; }
    return ORBHIP_OK;
}

// the tables both host forms stage
static void cull_stage_tables(Stage &st, int rows, int cap, int np, int pcap, int obs_cap, size_t total, const orbhip_cull_tables *t,
                              orbhip_cull_tables *dt)
{
    const size_t RC = (size_t)rows * cap;
    memset(dt, 0, sizeof(*dt));
    if (t->kps) dt->kps = st.put((const orbhip_keypoint *)t->kps, RC);
    if (t->u_right) dt->u_right = st.put((const float *)t->u_right, RC);
    if (t->depth) dt->depth = st.put((const float *)t->depth, RC);
    if (t->n) dt->n = st.put((const int32_t *)t->n, (size_t)rows);
    dt->obs_start = st.put((const int32_t *)t->obs_start, (size_t)np + 1);
    dt->obs_kf = st.put((const int32_t *)t->obs_kf, total);
    dt->obs_idx = st.put((const int32_t *)t->obs_idx, total);
    dt->ref_obs = st.put((const int32_t *)t->ref_obs, (size_t)np);
    if (t->not_erase) dt->not_erase = st.put((const uint8_t *)t->not_erase, (size_t)rows);
    (void)pcap; (void)obs_cap;
}

int orbhip_cull_map_points(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t,
                           const orbhip_cull_io *io, int R, const int32_t *recent, const int32_t *found, const int32_t *visible,
                           const int32_t *first_kf_id, int cur_kf_id, int th_obs, int32_t *recent_out, int32_t *n_recent_out,
                           uint8_t *status)
{
    if (int rc = cull_map_points_args(rows, cap, np, pcap, obs_cap, t, io, R, recent, found, visible, first_kf_id, th_obs, recent_out,
                                      n_recent_out, status))
        return rc;
    size_t total;
    if (int rc = cull_check_tables("cull_map_points", rows, cap, np, obs_cap, t, io, &total)) return rc;
    for (int e = 0; e < R; ++e)
        if (recent[e] < 0 || recent[e] >= np) { set_error("cull_map_points: list entry %d (point %d) is outside the map", e, recent[e]); return ORBHIP_E_ARG; }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t RC = (size_t)rows * cap, P = (size_t)np, Rn = (size_t)R;
    Stage st;
    int rc;
    orbhip_cull_tables dt;
    orbhip_cull_io dio;
    memset(&dio, 0, sizeof(dio));
    orbhip_cull_tables th = *t;
    th.kps = nullptr; th.depth = nullptr; th.n = nullptr; th.not_erase = nullptr;       // not read by this call
    const int32_t *d_recent, *d_found, *d_visible, *d_first;
    void *d_recent_out, *d_n_out, *d_status;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            auto inout = [&](void *host, size_t bytes) { return stg.inout((uint8_t *)host, bytes); };
            auto out = [&](void *host, size_t bytes) { return stg.out((uint8_t *)host, bytes); };
            cull_stage_tables(stg, rows, cap, np, pcap, obs_cap, total, &th, &dt);
            d_recent = stg.put(recent, Rn); d_found = stg.put(found, P); d_visible = stg.put(visible, P);
            d_first = stg.put(first_kf_id, P);
            dio.slot_point = inout(io->slot_point, RC * 4);
            dio.flags = inout(io->flags, P);
            dio.obs_start_out = out(io->obs_start_out, (P + 1) * 4);
            dio.obs_kf_out = inout(io->obs_kf_out, total * 4);
            dio.obs_idx_out = inout(io->obs_idx_out, total * 4);
            dio.ref_obs_out = out(io->ref_obs_out, P * 4);
            d_recent_out = inout(recent_out, Rn * 4); d_n_out = out(n_recent_out, 4); d_status = out(status, Rn);
        }))) return rc;
    if ((rc = cull_map_points_launch(m, rows, cap, np, obs_cap, &dt, &dio, R, d_recent, d_found, d_visible, d_first, cur_kf_id, th_obs,
                                     d_recent_out, d_n_out, d_status)))
        return rc;
    return stage_fetch(m, &st);
}

int orbhip_cull_key_frames(orbhip_matcher *m, int rows, int cap, int np, int pcap, int obs_cap, const orbhip_cull_tables *t,
                           const orbhip_cull_io *io, const orbhip_covis_state *s, int id0_row, int U, const int32_t *cand, int mono,
                           float th_depth, int32_t *report)
{
    if (int rc = cull_key_frames_args(rows, cap, np, pcap, obs_cap, t, io, s, id0_row, U, cand, mono, report)) return rc;
    size_t total;
    if (int rc = cull_check_tables("cull_key_frames", rows, cap, np, obs_cap, t, io, &total)) return rc;
    const int32_t *n = (const int32_t *)t->n, *n_ord = (const int32_t *)s->n_ord, *ord_kf = (const int32_t *)s->ord_kf;
    const int32_t *parent = (const int32_t *)s->parent;
    for (int r = 0; r < rows; ++r) {
        if (n[r] < 0 || n[r] > cap) { set_error("cull_key_frames: bank row %d holds a count outside [0, cap]", r); return ORBHIP_E_ARG; }
        if (n_ord[r] < 0 || n_ord[r] > rows) { set_error("cull_key_frames: n_ord of bank row %d is outside [0, rows]", r); return ORBHIP_E_ARG; }
        if (parent[r] < -1 || parent[r] >= rows) { set_error("cull_key_frames: the parent of bank row %d is outside the bank", r); return ORBHIP_E_ARG; }
        for (int i = 0; i < n_ord[r]; ++i)
            if (ord_kf[(size_t)r * rows + i] < 0 || ord_kf[(size_t)r * rows + i] >= rows) { set_error("cull_key_frames: the ordered list of bank row %d names a row outside the bank", r); return ORBHIP_E_ARG; }
    }
    {
        std::vector<uint8_t> seen((size_t)rows, 0);
        for (int u = 0; u < U; ++u) {
            const int r = cand[u];
            if (r < -1 || r >= rows) { set_error("cull_key_frames: candidate %d (row %d) is outside the bank", u, r); return ORBHIP_E_ARG; }
            if (r < 0) continue;
            if (seen[r]) { set_error("cull_key_frames: the candidate list names bank row %d twice", r); return ORBHIP_E_ARG; }
            seen[r] = 1;
        }
    }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t RC = (size_t)rows * cap, P = (size_t)np, Rw = (size_t)rows, Un = (size_t)U;
    Stage st;
    int rc;
    orbhip_cull_tables dt;
    orbhip_cull_io dio;
    orbhip_covis_state ds;
    memset(&dio, 0, sizeof(dio));
    memset(&ds, 0, sizeof(ds));
    const int32_t *d_cand;
    void *d_report;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            auto inout = [&](void *host, size_t bytes) { return stg.inout((uint8_t *)host, bytes); };
            auto out = [&](void *host, size_t bytes) { return stg.out((uint8_t *)host, bytes); };
            cull_stage_tables(stg, rows, cap, np, pcap, obs_cap, total, t, &dt);
            d_cand = stg.put(cand, Un);
            dio.slot_point = inout(io->slot_point, RC * 4);
            dio.flags = inout(io->flags, P);
            dio.kf_bad = inout(io->kf_bad, Rw);
            if (io->to_be_erased) dio.to_be_erased = inout(io->to_be_erased, Rw);
            dio.child_start = out(io->child_start, (Rw + 1) * 4);
            dio.child = inout(io->child, Rw * 4);
            dio.obs_start_out = out(io->obs_start_out, (P + 1) * 4);
            dio.obs_kf_out = inout(io->obs_kf_out, total * 4);
            dio.obs_idx_out = inout(io->obs_idx_out, total * 4);
            dio.ref_obs_out = out(io->ref_obs_out, P * 4);
            ds.conn_w = inout(s->conn_w, Rw * Rw * 4);
            ds.ord_kf = inout(s->ord_kf, Rw * Rw * 4);
            ds.ord_w = inout(s->ord_w, Rw * Rw * 4);
            ds.n_ord = inout(s->n_ord, Rw * 4);
            ds.covis = inout(s->covis, Rw * 40);
            ds.parent = inout(s->parent, Rw * 4);
            d_report = out(report, Un * 32);
        }))) return rc;
    if ((rc = cull_key_frames_launch(m, rows, cap, np, obs_cap, &dt, &dio, &ds, id0_row, U, d_cand, mono, th_depth, d_report))) return rc;
    return stage_fetch(m, &st);
}

// ---- Sim3 RANSAC (kernels: orbhip_sim3.hip) ---------------------------------------------------------------------------
// SetRansacParameters (src/Sim3Solver.cc:114-138) as a function of N.  epsilon is a float before pow, as in the text; the
// quotient is clamped while still a double (the text converts it to int first, which overflows for small epsilon).
static int sim3_limit_of(int N, double prob, int min_inliers, int max_its)
{
    if (N < min_inliers) return 0;          // iterate never runs (:146)
    if (N == min_inliers) return 1;
    const float epsilon = (float)min_inliers / N;
    const double d = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)epsilon, 3)));
    if (!(d >= 1.0)) return 1;
    return d > (double)max_its ? max_its : (int)d;
}

static int sim3_params(const char *who, int C, int cap, const orbhip_camera *cam, int min_inliers, int max_its)
{
    if (C < 0 || cap < 1 || !cam || min_inliers < 3 || max_its < 1) return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("%s: capacity %d exceeds %d", who, cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (max_its > 65536) { set_error("%s: %d iterations exceed 65536", who, max_its); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}
static bool sim3_solvers_ok(const orbhip_sim3_solvers *s)
{
    return s && s->x1 && s->x2 && s->p1 && s->p2 && s->max_err1 && s->max_err2 && s->slot1 && s->n_corr && s->n1 && s->limit && s->state;
}
static int sim3_setup_args(int C, int cur, const void *kf_index, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                           const orbhip_sim3_tables *t, const void *matched12, int match_form, const float *level_sigma2, double prob,
                           int min_inliers, int max_its)
{
    if (int rc = sim3_params("sim3_setup", C, cap, cam, min_inliers, max_its)) return rc;
    if (rows < 0 || np < 0 || pcap < 0 || np > pcap || cur < 0 || cur >= rows || !(prob > 0.0 && prob < 1.0) || !level_sigma2 ||
        cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS || !kf_index || !matched12 ||
        (match_form != ORBHIP_SIM3_MATCH_POINTS && match_form != ORBHIP_SIM3_MATCH_SLOTS))
        return ORBHIP_E_ARG;
    if (!t || !t->slot_point || !t->obs_start || !t->obs_kf || !t->obs_idx || !t->flags || !t->world || !t->Tcw || !t->kps || !t->n)
        return ORBHIP_E_ARG;
    return ORBHIP_OK;
}
static void sim3_solvers(Sim3Args &A, const orbhip_sim3_solvers *s)
{
    A.x1 = (float *)s->x1; A.x2 = (float *)s->x2; A.p1 = (float *)s->p1; A.p2 = (float *)s->p2;
    A.max_err1 = (uint32_t *)s->max_err1; A.max_err2 = (uint32_t *)s->max_err2; A.slot1 = (int *)s->slot1;
    A.n_corr = (int *)s->n_corr; A.n1 = (int *)s->n1; A.limit = (int *)s->limit; A.state = (int *)s->state;
}
static void sim3_camera(Sim3Args &A, const orbhip_camera *cam)
{
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.n_levels = cam->n_levels;
}
// mvnMaxError* is a vector<size_t> (include/Sim3Solver.h:78-79): the product is truncated
static uint32_t sim3_threshold(float sigma2)
{
    const double v = 9.210 * (double)sigma2;
    if (!(v >= 0.0)) return 0;
    return v >= 4294967295.0 ? 0xffffffffu : (uint32_t)v;
}

static int sim3_setup_launch(orbhip_matcher *m, int C, int cur, const void *d_kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                             const orbhip_sim3_tables *t, const void *d_matched12, int match_form, const float *level_sigma2, double prob,
                             int min_inliers, int max_its, const orbhip_sim3_solvers *s)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *d_tab;
    if (int rc = scratch(m, S_SIM3LIM, ((size_t)cap + 1) * sizeof(int), &d_tab)) return rc;
    if (m->sim3_cap != cap || m->sim3_prob != prob || m->sim3_min_inliers != min_inliers || m->sim3_max_its != max_its) {
        ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));   // the table a previous call may still read is about to change
        m->sim3_limit.resize((size_t)cap + 1);
        for (int N = 0; N <= cap; ++N) m->sim3_limit[N] = sim3_limit_of(N, prob, min_inliers, max_its);
        ORBHIP_HIP_CHECK(hipMemcpy(d_tab, m->sim3_limit.data(), ((size_t)cap + 1) * sizeof(int), hipMemcpyHostToDevice));
        m->sim3_cap = cap; m->sim3_prob = prob; m->sim3_min_inliers = min_inliers; m->sim3_max_its = max_its;
    }
    Sim3Args A;
    memset(&A, 0, sizeof(A));
    A.slot_point = (const int *)t->slot_point; A.n = (const int *)t->n; A.obs_start = (const int *)t->obs_start;
    A.obs_kf = (const int *)t->obs_kf; A.obs_idx = (const int *)t->obs_idx; A.flags = (const uint8_t *)t->flags;
    A.world = (const float *)t->world; A.Tcw = (const float *)t->Tcw; A.kps = (const orbhip_keypoint *)t->kps;
    A.kf_index = (const int *)d_kf_index; A.matched12 = (const int *)d_matched12; A.limit_tab = (const int *)d_tab;
    sim3_solvers(A, s);
    sim3_camera(A, cam);
    for (int l = 0; l < ORBHIP_MAX_LEVELS; ++l) A.thr[l] = l < cam->n_levels ? sim3_threshold(level_sigma2[l]) : 0;
    A.C = C; A.cur = cur; A.rows = rows; A.cap = cap; A.np = np; A.match_form = match_form; A.min_inliers = min_inliers; A.max_its = max_its;
    return launch_sim3_setup(m->stream, A);
}

int orbhip_sim3_setup_device(orbhip_matcher *m, int C, int cur, const void *d_kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                             int pcap, const orbhip_sim3_tables *t, const void *d_matched12, int match_form, const float *level_sigma2,
                             double prob, int min_inliers, int max_its, const orbhip_sim3_solvers *s)
{
    if (int rc = sim3_setup_args(C, cur, d_kf_index, cam, rows, cap, np, pcap, t, d_matched12, match_form, level_sigma2, prob, min_inliers,
                                 max_its))
        return rc;
    if (!sim3_solvers_ok(s) || !m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    return sim3_setup_launch(m, C, cur, d_kf_index, cam, rows, cap, np, t, d_matched12, match_form, level_sigma2, prob, min_inliers, max_its, s);
}

static int sim3_iterate_launch(orbhip_matcher *m, int C, int cap, const orbhip_camera *cam, const orbhip_sim3_solvers *s, const void *d_draws,
                               int max_its, int n_iterations, int min_inliers, int fix_scale, void *d_sim3, void *d_inliers, void *d_report)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const int n_iter = std::min(n_iterations, max_its);
    void *work;
    if (int rc = scratch(m, S_SIM3, sim3_workspace_bytes(C, n_iter, cap), &work)) return rc;
    Sim3Args A;
    memset(&A, 0, sizeof(A));
    sim3_solvers(A, s);
    sim3_camera(A, cam);
    A.draws = (const int *)d_draws; A.sim3 = (float *)d_sim3; A.inliers = (uint8_t *)d_inliers; A.report = (int *)d_report;
    A.C = C; A.cap = cap; A.max_its = max_its; A.n_iter = n_iter; A.min_inliers = min_inliers; A.fix_scale = fix_scale != 0;
    return launch_sim3_iterate(m->stream, A, work);
}

int orbhip_sim3_iterate_device(orbhip_matcher *m, int C, int cap, const orbhip_camera *cam, const orbhip_sim3_solvers *s, const void *d_draws,
                               int max_its, int n_iterations, int min_inliers, int fix_scale, void *d_sim3, void *d_inliers, void *d_report)
{
    if (int rc = sim3_params("sim3_iterate", C, cap, cam, min_inliers, max_its)) return rc;
    if (!sim3_solvers_ok(s) || n_iterations < 0 || !d_draws || !d_sim3 || !d_inliers || !d_report || !m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    return sim3_iterate_launch(m, C, cap, cam, s, d_draws, max_its, n_iterations, min_inliers, fix_scale, d_sim3, d_inliers, d_report);
}

// N of candidate row kf as k_sim3_setup counts it, for the draw check of the host form
static int sim3_host_count(int cur, int kf, int cap, const orbhip_sim3_tables *t, const int32_t *matched, int match_form)
{
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n, *obs_start = (const int32_t *)t->obs_start;
    const int32_t *obs_kf = (const int32_t *)t->obs_kf;
    const uint8_t *flags = (const uint8_t *)t->flags;
    auto observed = [&](int p, int row) {
        for (int o = obs_start[p]; o < obs_start[p + 1]; ++o)
            if (obs_kf[o] == row) return true;
        return false;
    };
    int N = 0;
    for (int i1 = 0; i1 < n[cur]; ++i1) {
        const int mt = matched[i1];
        if (mt < 0) continue;
        const int p2 = match_form == ORBHIP_SIM3_MATCH_SLOTS ? slot_point[(size_t)kf * cap + mt] : mt;
        const int p1 = slot_point[(size_t)cur * cap + i1];
        if (p1 < 0 || p2 < 0 || !(flags[p1] & ORBHIP_POINT_PRESENT) || !(flags[p2] & ORBHIP_POINT_PRESENT)) continue;
        if (observed(p1, cur) && observed(p2, kf)) ++N;
    }
    return N;
}

// what the host forms over orbhip_sim3_tables check of the tables' contents
static int sim3_check_tables(const char *who, const orbhip_camera *cam, int rows, int cap, int np, const orbhip_sim3_tables *t)
{
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n, *obs_start = (const int32_t *)t->obs_start;
    const int32_t *obs_kf = (const int32_t *)t->obs_kf, *obs_idx = (const int32_t *)t->obs_idx;
    const orbhip_keypoint *kps = (const orbhip_keypoint *)t->kps;
    const size_t RC = (size_t)rows * cap;
    for (int r = 0; r < rows; ++r)
        if (n[r] < 0 || n[r] > cap) { set_error("%s: bank row %d holds a count outside [0, cap]", who, r); return ORBHIP_E_ARG; }
    for (size_t i = 0; i < RC; ++i)
        if (slot_point[i] < -1 || slot_point[i] >= np) { set_error("%s: bank row %zu holds a point index out of range", who, i / cap); return ORBHIP_E_ARG; }
    if (obs_start[0] != 0) { set_error("%s: obs_start must start at 0", who); return ORBHIP_E_ARG; }
    for (int p = 0; p < np; ++p)
        if (obs_start[p + 1] < obs_start[p]) { set_error("%s: obs_start must be non-decreasing (entry %d)", who, p); return ORBHIP_E_ARG; }
    const size_t total = (size_t)obs_start[np];
    for (size_t o = 0; o < total; ++o) {
        if (obs_kf[o] < 0 || obs_kf[o] >= rows || obs_idx[o] < 0 || obs_idx[o] >= cap) { set_error("%s: observation %zu is outside the bank", who, o); return ORBHIP_E_ARG; }
        const int oct = kps[(size_t)obs_kf[o] * cap + obs_idx[o]].octave;
        if (oct < 0 || oct >= cam->n_levels) { set_error("%s: observation %zu names a key point of octave %d", who, o, oct); return ORBHIP_E_ARG; }
    }
    return ORBHIP_OK;
}

int orbhip_sim3_ransac(orbhip_matcher *m, int C, int cur, const int32_t *kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                       int pcap, const orbhip_sim3_tables *t, const int32_t *matched12, int match_form, const float *level_sigma2,
                       double prob, int min_inliers, int max_its, int fix_scale, const int32_t *draws, int n_iterations, int32_t *state,
                       float *sim3, uint8_t *inliers, int32_t *report)
{
    if (int rc = sim3_setup_args(C, cur, kf_index, cam, rows, cap, np, pcap, t, matched12, match_form, level_sigma2, prob, min_inliers,
                                 max_its))
        return rc;
    if (n_iterations < 0 || !draws || !sim3 || !inliers || !report) return ORBHIP_E_ARG;
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n, *obs_start = (const int32_t *)t->obs_start;
    const int32_t *obs_kf = (const int32_t *)t->obs_kf, *obs_idx = (const int32_t *)t->obs_idx;
    const orbhip_keypoint *kps = (const orbhip_keypoint *)t->kps;
    const size_t RC = (size_t)rows * cap, P = (size_t)np, Cn = (size_t)C;
    if (int rc = sim3_check_tables("sim3_ransac", cam, rows, cap, np, t)) return rc;
    const size_t total = (size_t)obs_start[np];
    const int n_iter = std::min(n_iterations, max_its);
    for (int c = 0; c < C; ++c) {
        const int kf = kf_index[c];
        if (kf < 0 || kf >= rows) { set_error("sim3_ransac: candidate %d (row %d) is outside the bank", c, kf); return ORBHIP_E_ARG; }
        const int32_t *mt = matched12 + (size_t)c * cap;
        for (int i1 = 0; i1 < n[cur]; ++i1)
            if (mt[i1] >= (match_form == ORBHIP_SIM3_MATCH_SLOTS ? cap : np)) { set_error("sim3_ransac: match %d of candidate %d is out of range", i1, c); return ORBHIP_E_ARG; }
        const int it0 = state ? state[2 * c] : 0;
        if (it0 < 0 || it0 > max_its || (state && state[2 * c + 1] < 0)) { set_error("sim3_ransac: the state of candidate %d is out of range", c); return ORBHIP_E_ARG; }
        const int N = sim3_host_count(cur, kf, cap, t, mt, match_form);
        const int last = std::min(sim3_limit_of(N, prob, min_inliers, max_its), it0 + n_iter);
        for (int it = it0; it < last; ++it)
            for (int k = 0; k < 3; ++k) {
                const int d = draws[((size_t)c * max_its + it) * 3 + k];
                if (d < 0 || d > N - 1 - k) { set_error("sim3_ransac: draw %d of iteration %d of candidate %d is %d, outside [0, %d]", k, it, c, d, N - 1 - k); return ORBHIP_E_ARG; }
            }
    }
    if (!m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t CC = Cn * cap;
    Stage st;
    int rc;
    orbhip_sim3_tables dt;
    const int32_t *d_kf, *d_matched, *d_draws;
    float *d_sim3;
    uint8_t *d_inl;
    int32_t *d_rep, *d_state;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dt.slot_point = stg.put(slot_point, RC); dt.obs_start = stg.put(obs_start, P + 1); dt.obs_kf = stg.put(obs_kf, total);
            dt.obs_idx = stg.put(obs_idx, total); dt.flags = stg.put((const uint8_t *)t->flags, P);
            dt.world = stg.put((const float *)t->world, P * 3);
            dt.Tcw = stg.put((const float *)t->Tcw, (size_t)rows * 12); dt.kps = stg.put(kps, RC); dt.n = stg.put(n, (size_t)rows);
            d_kf = stg.put(kf_index, Cn); d_matched = stg.put(matched12, CC); d_draws = stg.put(draws, Cn * max_its * 3);
            d_sim3 = stg.inout(sim3, Cn * 16);
            d_inl = stg.inout(inliers, CC);
            d_rep = stg.inout(report, Cn * 8);
            d_state = state ? stg.inout(state, Cn * 2) : stg.fill<int32_t>(Cn * 2, [&](int32_t *h_state) { memset(h_state, 0, Cn * 8); });
        }))) return rc;
    // the solvers live in the handle for the length of the call
    void *sv;
    if ((rc = scratch(m, S_SIM3SOLV, 11 * al256(CC * 12), &sv))) return rc;
    uint8_t *w = (uint8_t *)sv;
    auto carve = [&](size_t bytes) { void *p = w; w += al256(bytes); return p; };
    orbhip_sim3_solvers ds;
    ds.x1 = carve(CC * 12); ds.x2 = carve(CC * 12); ds.p1 = carve(CC * 8); ds.p2 = carve(CC * 8); ds.max_err1 = carve(CC * 4);
    ds.max_err2 = carve(CC * 4); ds.slot1 = carve(CC * 4); ds.n_corr = carve(Cn * 4); ds.n1 = carve(Cn * 4); ds.limit = carve(Cn * 4);
    ds.state = carve(Cn * 8);
    if ((rc = sim3_setup_launch(m, C, cur, d_kf, cam, rows, cap, np, &dt, d_matched, match_form, level_sigma2, prob, min_inliers, max_its, &ds)))
        return rc;
    ORBHIP_HIP_CHECK(hipMemcpyAsync(ds.state, d_state, Cn * 8, hipMemcpyDeviceToDevice, m->stream));
    if ((rc = sim3_iterate_launch(m, C, cap, cam, &ds, d_draws, max_its, n_iterations, min_inliers, fix_scale, d_sim3, d_inl, d_rep)))
        return rc;
    ORBHIP_HIP_CHECK(hipMemcpyAsync(d_state, ds.state, Cn * 8, hipMemcpyDeviceToDevice, m->stream));
    return stage_fetch(m, &st);
}

// ---- PnP RANSAC (kernels: orbhip_pnp.hip) ------------------------------------------------------------------------------
// SetRansacParameters (src/PnPsolver.cc:134-152) as a function of N: the adjusted mRansacMinInliers and mRansacMaxIts, with
// the reference's types.  The quotient is clamped while still a double (the text converts it to int first).
static void pnp_parameters_of(int N, const orbhip_pnp_params *p, int *n_min_out, int *limit_out)
{
    float eps = p->epsilon;
    int n_min = (int)((float)N * eps);                   // :134, a float product
    if (n_min < p->min_inliers) n_min = p->min_inliers;
    if (n_min < p->min_set) n_min = p->min_set;
    *n_min_out = n_min;
    if (N < n_min) { *limit_out = 0; return; }          // iterate never runs (:173)
    const float q = (float)n_min / (float)N;
    if (eps < q) eps = q;
    if (n_min == N) { *limit_out = 1; return; }
    const double d = std::ceil(std::log(1 - p->prob) / std::log(1 - std::pow((double)eps, 3)));
    *limit_out = !(d >= 1.0) ? 1 : (d > (double)p->max_its ? p->max_its : (int)d);
}

static bool pnp_params_equal(const orbhip_pnp_params &a, const orbhip_pnp_params &b)
{
    return a.prob == b.prob && a.min_inliers == b.min_inliers && a.max_its == b.max_its && a.min_set == b.min_set &&
           a.epsilon == b.epsilon && a.th2 == b.th2;
}
static int pnp_common_args(const char *who, int C, int n, int cap, const orbhip_camera *cam, const orbhip_pnp_params *p)
{
    if (C < 0 || n < 0 || cap < 1 || n > cap || !cam || !p) return ORBHIP_E_ARG;
    if (p->min_set != 4) { set_error("%s: min_set must be 4", who); return ORBHIP_E_ARG; }
    if (p->min_inliers < 1 || p->max_its < 1 || !(p->prob > 0.0 && p->prob < 1.0) || !(p->epsilon >= 0.f) || !(p->th2 >= 0.f) ||
        !std::isfinite(p->epsilon) || !std::isfinite(p->th2))
        return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("%s: capacity %d exceeds %d", who, cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if (p->max_its > 65536) { set_error("%s: %d iterations exceed 65536", who, p->max_its); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}
static bool pnp_solvers_ok(const orbhip_pnp_solvers *s)
{
    return s && s->p2d && s->p3d && s->max_err && s->kp_index && s->n_corr && s->min_inliers && s->limit && s->state &&
           s->best_inliers && s->best_Tcw;
}
static int pnp_setup_args(int C, const void *kps, int n, int cap, const void *matches, int match_form, const void *kf_index, int rows,
                          int np, int pcap, const orbhip_pnp_map *map, const orbhip_camera *cam, const float *level_sigma2,
                          const orbhip_pnp_params *p)
{
    if (int rc = pnp_common_args("pnp_setup", C, n, cap, cam, p)) return rc;
    if (rows < 0 || np < 0 || pcap < 0 || np > pcap || !kps || !matches || !level_sigma2 || cam->n_levels < 1 ||
        cam->n_levels > ORBHIP_MAX_LEVELS || !map || !map->flags || !map->world ||
        (match_form != ORBHIP_PNP_MATCH_POINTS && match_form != ORBHIP_PNP_MATCH_SLOTS))
        return ORBHIP_E_ARG;
    if (match_form == ORBHIP_PNP_MATCH_SLOTS && (!kf_index || !map->slot_point)) return ORBHIP_E_ARG;
    return ORBHIP_OK;
}
static void pnp_solvers(PnpArgs &A, const orbhip_pnp_solvers *s)
{
    A.p2d = (float *)s->p2d; A.p3d = (float *)s->p3d; A.max_err = (float *)s->max_err; A.kp_index = (int *)s->kp_index;
    A.n_corr = (int *)s->n_corr; A.min_inliers = (int *)s->min_inliers; A.limit = (int *)s->limit; A.state = (int *)s->state;
    A.best_inliers = (uint8_t *)s->best_inliers; A.best_Tcw = (float *)s->best_Tcw;
}
static void pnp_camera(PnpArgs &A, const orbhip_camera *cam)
{
    A.fu = (double)cam->fx; A.fv = (double)cam->fy; A.uc = (double)cam->cx; A.vc = (double)cam->cy; A.n_levels = cam->n_levels;
}

static int pnp_setup_launch(orbhip_matcher *m, int C, const void *d_kps, int n, int cap, const void *d_matches, int match_form,
                            const void *d_kf_index, int rows, int np, const orbhip_pnp_map *map, const orbhip_camera *cam,
                            const float *level_sigma2, const orbhip_pnp_params *p, const orbhip_pnp_solvers *s)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *d_tab;
    const size_t tab_bytes = ((size_t)cap + 1) * 2 * sizeof(int);
    if (int rc = scratch(m, S_PNPTAB, tab_bytes, &d_tab)) return rc;
    if (m->pnp_cap != cap || !pnp_params_equal(m->pnp_params, *p)) {
        ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));   // the table a previous call may still read is about to change
        m->pnp_tab.resize(((size_t)cap + 1) * 2);
        for (int N = 0; N <= cap; ++N) pnp_parameters_of(N, p, &m->pnp_tab[2 * (size_t)N], &m->pnp_tab[2 * (size_t)N + 1]);
        ORBHIP_HIP_CHECK(hipMemcpy(d_tab, m->pnp_tab.data(), tab_bytes, hipMemcpyHostToDevice));
        m->pnp_cap = cap; m->pnp_params = *p;
    }
    PnpArgs A;
    memset(&A, 0, sizeof(A));
    A.kps = (const orbhip_keypoint *)d_kps; A.matches = (const int *)d_matches; A.kf_index = (const int *)d_kf_index;
    A.slot_point = (const int *)map->slot_point; A.flags = (const uint8_t *)map->flags; A.world = (const float *)map->world;
    A.tab = (const int *)d_tab;
    pnp_solvers(A, s);
    pnp_camera(A, cam);
    for (int l = 0; l < ORBHIP_MAX_LEVELS; ++l) A.max_err_lv[l] = l < cam->n_levels ? level_sigma2[l] * p->th2 : 0.f;   // :156
    A.C = C; A.n = n; A.cap = cap; A.rows = rows; A.np = np; A.match_form = match_form;
    return launch_pnp_setup(m->stream, A);
}

int orbhip_pnp_setup_device(orbhip_matcher *m, int C, const void *d_kps, int n, int cap, const void *d_matches, int match_form,
                            const void *d_kf_index, int rows, int np, int pcap, const orbhip_pnp_map *map, const orbhip_camera *cam,
                            const float *level_sigma2, const orbhip_pnp_params *params, const orbhip_pnp_solvers *s)
{
    if (int rc = pnp_setup_args(C, d_kps, n, cap, d_matches, match_form, d_kf_index, rows, np, pcap, map, cam, level_sigma2, params))
        return rc;
    if (!pnp_solvers_ok(s) || !m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    return pnp_setup_launch(m, C, d_kps, n, cap, d_matches, match_form, d_kf_index, rows, np, map, cam, level_sigma2, params, s);
}

static int pnp_iterate_launch(orbhip_matcher *m, int C, int n, int cap, const orbhip_camera *cam, const orbhip_pnp_params *p,
                              const orbhip_pnp_solvers *s, const void *d_draws, int draw_rows, int n_iterations, void *d_Tcw,
                              void *d_inliers, void *d_report)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const int W = std::min(std::max(p->max_its, n_iterations), draw_rows);   // no call runs more iterations than this
    void *work;
    if (int rc = scratch(m, S_PNP, pnp_workspace_bytes(C, W, cap), &work)) return rc;
    PnpArgs A;
    memset(&A, 0, sizeof(A));
    pnp_solvers(A, s);
    pnp_camera(A, cam);
    A.draws = (const int *)d_draws; A.Tcw = (float *)d_Tcw; A.inliers = (uint8_t *)d_inliers; A.report = (int *)d_report;
    A.C = C; A.n = n; A.cap = cap; A.n_iter = n_iterations; A.draw_rows = draw_rows; A.W = W;
    return launch_pnp_iterate(m->stream, A, work);
}

int orbhip_pnp_iterate_device(orbhip_matcher *m, int C, int n, int cap, const orbhip_camera *cam, const orbhip_pnp_params *params,
                              const orbhip_pnp_solvers *s, const void *d_draws, int draw_rows, int n_iterations, void *d_Tcw,
                              void *d_inliers, void *d_report)
{
    if (int rc = pnp_common_args("pnp_iterate", C, n, cap, cam, params)) return rc;
    if (!pnp_solvers_ok(s) || n_iterations < 0 || n_iterations > 65536 || !d_draws || !d_Tcw || !d_inliers || !d_report || !m)
        return ORBHIP_E_ARG;
    if (draw_rows < std::max(params->max_its, n_iterations)) {
        set_error("pnp_iterate: %d draw rows, a fresh solver can reach %d", draw_rows, std::max(params->max_its, n_iterations));
        return ORBHIP_E_ARG;
    }
    if (C == 0) return ORBHIP_OK;
    return pnp_iterate_launch(m, C, n, cap, cam, params, s, d_draws, draw_rows, n_iterations, d_Tcw, d_inliers, d_report);
}

int orbhip_pnp_ransac(orbhip_matcher *m, int C, const orbhip_keypoint *kps, int n, int cap, const int32_t *matches, int match_form,
                      const int32_t *kf_index, int rows, int np, int pcap, const orbhip_pnp_map *map, const orbhip_camera *cam,
                      const float *level_sigma2, const orbhip_pnp_params *params, const int32_t *draws, int draw_rows, int n_iterations,
                      int32_t *state, uint8_t *best_inliers, float *best_Tcw, float *Tcw, uint8_t *inliers, int32_t *report)
{
    if (int rc = pnp_setup_args(C, kps, n, cap, matches, match_form, kf_index, rows, np, pcap, map, cam, level_sigma2, params)) return rc;
    if (n_iterations < 0 || n_iterations > 65536 || draw_rows < 0 || !draws || !Tcw || !inliers || !report) return ORBHIP_E_ARG;
    if ((state != nullptr) != (best_inliers != nullptr) || (state != nullptr) != (best_Tcw != nullptr)) {
        set_error("pnp_ransac: state, best_inliers and best_Tcw go together");
        return ORBHIP_E_ARG;
    }
    const bool slots = match_form == ORBHIP_PNP_MATCH_SLOTS;
    const int32_t *slot_point = (const int32_t *)map->slot_point;
    const uint8_t *flags = (const uint8_t *)map->flags;
    const size_t RC = slots ? (size_t)rows * cap : 0, P = (size_t)np, Cn = (size_t)C, CC = Cn * cap;
    for (size_t i = 0; i < RC; ++i)
        if (slot_point[i] < -1 || slot_point[i] >= np) { set_error("pnp_ransac: bank row %zu holds a point index out of range", i / cap); return ORBHIP_E_ARG; }
    for (int i = 0; i < n; ++i)
        if (kps[i].octave < 0 || kps[i].octave >= cam->n_levels) { set_error("pnp_ransac: key point %d has octave %d", i, kps[i].octave); return ORBHIP_E_ARG; }
    for (int c = 0; c < C; ++c) {
        const int kf = slots ? kf_index[c] : 0;
        if (slots && (kf < 0 || kf >= rows)) { set_error("pnp_ransac: candidate %d (row %d) is outside the bank", c, kf); return ORBHIP_E_ARG; }
        const int32_t *mt = matches + (size_t)c * cap;
        int N = 0;
        for (int i = 0; i < n; ++i) {
            if (mt[i] >= (slots ? cap : np)) { set_error("pnp_ransac: match %d of candidate %d is out of range", i, c); return ORBHIP_E_ARG; }
            if (mt[i] < 0) continue;
            const int p = slots ? slot_point[(size_t)kf * cap + mt[i]] : mt[i];
            if (p >= 0 && (flags[p] & ORBHIP_POINT_PRESENT)) ++N;
        }
        int n_min, limit;
        pnp_parameters_of(N, params, &n_min, &limit);
        const int it0 = state ? state[2 * c] : 0, best = state ? state[2 * c + 1] : 0;
        if (it0 < 0 || it0 > 65536 || (best != 0 && (best < n_min || best > N))) { set_error("pnp_ransac: the state of candidate %d is out of range", c); return ORBHIP_E_ARG; }
        if (best > 0) {
            int set = 0;
            for (int i = 0; i < N; ++i) set += best_inliers[(size_t)c * cap + i] ? 1 : 0;
            if (set != best) { set_error("pnp_ransac: best_inliers of candidate %d holds %d entries, the state says %d", c, set, best); return ORBHIP_E_ARG; }
        }
        if (N < n_min) continue;
        const int last = std::max(limit, it0 + n_iterations);
        if (last > draw_rows) { set_error("pnp_ransac: candidate %d runs to iteration %d, draws has %d rows", c, last, draw_rows); return ORBHIP_E_ARG; }
        for (int it = it0; it < last; ++it)
            for (int k = 0; k < 4; ++k) {
                const int d = draws[((size_t)c * draw_rows + it) * 4 + k];
                if (d < 0 || d > N - 1 - k) { set_error("pnp_ransac: draw %d of iteration %d of candidate %d is %d, outside [0, %d]", k, it, c, d, N - 1 - k); return ORBHIP_E_ARG; }
            }
    }
    if (!m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    int rc;
    const orbhip_keypoint *d_kps;
    const int32_t *d_matches, *d_kf, *d_draws;
    orbhip_pnp_map dm;
    float *d_Tcw, *d_bt;
    uint8_t *d_inl, *d_bi;
    int32_t *d_rep, *d_state;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_kps = stg.put(kps, (size_t)n);
            d_matches = stg.put(matches, CC); d_kf = slots ? stg.put(kf_index, Cn) : nullptr;
            dm.slot_point = slots ? stg.put(slot_point, RC) : nullptr;
            dm.flags = stg.put(flags, P); dm.world = stg.put((const float *)map->world, P * 3);
            d_draws = stg.put(draws, Cn * draw_rows * 4);
            d_Tcw = stg.inout(Tcw, Cn * 12);
            d_inl = stg.inout(inliers, CC);
            d_rep = stg.inout(report, Cn * 8);
            // state, best_inliers and best_Tcw go together: the caller's, or zeros that do not travel back
            d_state = state ? stg.inout(state, Cn * 2) : stg.fill<int32_t>(Cn * 2, [&](int32_t *h) { memset(h, 0, Cn * 8); });
            d_bi = state ? stg.inout(best_inliers, CC) : stg.fill<uint8_t>(CC, [&](uint8_t *h) { memset(h, 0, CC); });
            d_bt = state ? stg.inout(best_Tcw, Cn * 12) : stg.fill<float>(Cn * 12, [&](float *h) { memset(h, 0, Cn * 48); });
        }))) return rc;
    // the rest of the solver record lives in the handle for the length of the call
    void *sv;
    if ((rc = scratch(m, S_PNPSOLV, al256(CC * 8) + al256(CC * 12) + 2 * al256(CC * 4) + 4 * al256(Cn * 8), &sv))) return rc;
    uint8_t *w = (uint8_t *)sv;
    auto carve = [&](size_t bytes) { void *p = w; w += al256(bytes); return p; };
    orbhip_pnp_solvers ds;
    ds.p2d = carve(CC * 8); ds.p3d = carve(CC * 12); ds.max_err = carve(CC * 4); ds.kp_index = carve(CC * 4); ds.n_corr = carve(Cn * 4);
    ds.min_inliers = carve(Cn * 4); ds.limit = carve(Cn * 4); ds.state = carve(Cn * 8);
    ds.best_inliers = d_bi; ds.best_Tcw = d_bt;
    if ((rc = pnp_setup_launch(m, C, d_kps, n, cap, d_matches, match_form, d_kf, rows, np, &dm, cam, level_sigma2, params, &ds))) return rc;
    ORBHIP_HIP_CHECK(hipMemcpyAsync(ds.state, d_state, Cn * 8, hipMemcpyDeviceToDevice, m->stream));
    if ((rc = pnp_iterate_launch(m, C, n, cap, cam, params, &ds, d_draws, draw_rows, n_iterations, d_Tcw, d_inl, d_rep))) return rc;
    ORBHIP_HIP_CHECK(hipMemcpyAsync(d_state, ds.state, Cn * 8, hipMemcpyDeviceToDevice, m->stream));
    return stage_fetch(m, &st);
}

// ---- pose optimisation (kernel: orbhip_poseopt.hip) ----------------------------------------------------------------------
static int poseopt_args(int frames, const void *kps, const void *n, int cap, const void *world, const void *point_flags, int wrows,
                        int pcap, const orbhip_camera *cam, const float *inv_level_sigma2, int mode, int flags, const void *Tcw,
                        const void *frame_point, const void *outlier, const void *report)
{
    if (frames < 0 || cap < 1 || wrows < 0 || pcap < 0 || !cam || !inv_level_sigma2 || !kps || !n || !world || !Tcw || !frame_point ||
        !outlier || !report)
        return ORBHIP_E_ARG;
    if (mode != ORBHIP_POSEOPT_PLAIN && mode != ORBHIP_POSEOPT_DISCARD && mode != ORBHIP_POSEOPT_LOCAL_MAP) {
        set_error("pose_optimization: mode %d", mode);
        return ORBHIP_E_ARG;
    }
    if ((flags & ~(ORBHIP_POSEOPT_ONLY_TRACKING | ORBHIP_POSEOPT_STEREO)) || (mode != ORBHIP_POSEOPT_PLAIN && !point_flags) ||
        cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS || (frames > 0 && (wrows < 1 || pcap < 1)))
        return ORBHIP_E_ARG;
    if (cap > kPoCapMax) { set_error("pose_optimization: capacity %d exceeds %d", cap, kPoCapMax); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

static int poseopt_launch(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap, const void *d_u_right,
                          const void *d_world, const void *d_point_flags, int wrows, int pcap, const void *d_world_row,
                          const orbhip_camera *cam, const float *inv_level_sigma2, int mode, int flags, void *d_Tcw,
                          void *d_frame_point, void *d_outlier, void *d_discarded, void *d_report)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    PoArgs A;
    memset(&A, 0, sizeof(A));
    A.kps = (const orbhip_keypoint *)d_kps; A.n = (const int *)d_n; A.u_right = (const float *)d_u_right;
    A.world = (const float *)d_world; A.point_flags = (const uint8_t *)d_point_flags; A.world_row = (const int *)d_world_row;
    A.Tcw = (float *)d_Tcw; A.frame_point = (int *)d_frame_point; A.outlier = (uint8_t *)d_outlier; A.discarded = (int *)d_discarded;
    A.report = (int *)d_report;
    fill_inv_sigma2(A.inv, cam, inv_level_sigma2);
    A.cam = po_cam(cam, 5.991, 7.815);                                        // src/Optimizer.cc:273-274
    A.frames = frames; A.cap = cap; A.wrows = wrows; A.pcap = pcap; A.n_levels = cam->n_levels; A.mode = mode; A.flags = flags;
    return launch_pose_optimization(m->stream, A);
}

int orbhip_pose_optimization_device(orbhip_matcher *m, int frames, const void *d_kps, const void *d_n, int cap, const void *d_u_right,
                                    const void *d_world, const void *d_point_flags, int wrows, int pcap, const void *d_world_row,
                                    const orbhip_camera *cam, const float *inv_level_sigma2, int mode, int flags, void *d_Tcw,
                                    void *d_frame_point, void *d_outlier, void *d_discarded, void *d_report)
{
    if (int rc = poseopt_args(frames, d_kps, d_n, cap, d_world, d_point_flags, wrows, pcap, cam, inv_level_sigma2, mode, flags, d_Tcw,
                              d_frame_point, d_outlier, d_report))
        return rc;
    if (!m) return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    return poseopt_launch(m, frames, d_kps, d_n, cap, d_u_right, d_world, d_point_flags, wrows, pcap, d_world_row, cam,
                          inv_level_sigma2, mode, flags, d_Tcw, d_frame_point, d_outlier, d_discarded, d_report);
}

int orbhip_pose_optimization(orbhip_matcher *m, int frames, const orbhip_keypoint *kps, const int32_t *n, int cap, const float *u_right,
                             const float *world, const uint8_t *point_flags, int wrows, int pcap, const int32_t *world_row,
                             const orbhip_camera *cam, const float *inv_level_sigma2, int mode, int flags, float *Tcw,
                             int32_t *frame_point, uint8_t *outlier, int32_t *discarded, int32_t *report)
{
    if (int rc = poseopt_args(frames, kps, n, cap, world, point_flags, wrows, pcap, cam, inv_level_sigma2, mode, flags, Tcw, frame_point,
                              outlier, report))
        return rc;
    for (int f = 0; f < frames; ++f) {
        if (n[f] < 0 || n[f] > cap) { set_error("pose_optimization: frame %d has n = %d, cap = %d", f, n[f], cap); return ORBHIP_E_ARG; }
        if (world_row && (world_row[f] < 0 || world_row[f] >= wrows)) {
            set_error("pose_optimization: frame %d refers to world row %d of %d", f, world_row[f], wrows);
            return ORBHIP_E_ARG;
        }
        for (int i = 0; i < n[f]; ++i) {
            const size_t k = (size_t)f * cap + i;
            if (frame_point[k] < -1 || frame_point[k] >= pcap) {
                set_error("pose_optimization: slot %d of frame %d holds point %d, outside [-1, %d)", i, f, frame_point[k], pcap);
                return ORBHIP_E_ARG;
            }
            if (frame_point[k] >= 0 && (kps[k].octave < 0 || kps[k].octave >= cam->n_levels)) {
                set_error("pose_optimization: key point %d of frame %d has octave %d", i, f, kps[k].octave);
                return ORBHIP_E_ARG;
            }
        }
    }
    if (!m) return ORBHIP_E_ARG;
    if (frames == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    int rc;
    const size_t Fn = (size_t)frames, FC = Fn * cap, WP = (size_t)wrows * pcap;
    const orbhip_keypoint *d_kps;
    const int32_t *d_n, *d_row;
    const float *d_ur, *d_world;
    const uint8_t *d_pf;
    float *d_Tcw;
    int32_t *d_fp, *d_dis, *d_rep;
    uint8_t *d_out;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_kps = stg.put(kps, FC);
            d_n = stg.put(n, Fn);
            d_ur = u_right ? stg.put(u_right, FC) : nullptr;
            d_world = stg.put(world, WP * 3);
            d_pf = point_flags ? stg.put(point_flags, WP) : nullptr;
            d_row = world_row ? stg.put(world_row, Fn) : nullptr;
            d_Tcw = stg.inout(Tcw, Fn * 12);
            d_fp = stg.inout(frame_point, FC);
            d_out = stg.inout(outlier, FC);
            d_dis = discarded ? stg.inout(discarded, FC) : nullptr;
            d_rep = stg.inout(report, Fn * 8);
        }))) return rc;
    if ((rc = poseopt_launch(m, frames, d_kps, d_n, cap, d_ur, d_world, d_pf, wrows, pcap, d_row, cam, inv_level_sigma2, mode, flags,
                             d_Tcw, d_fp, d_out, d_dis, d_rep)))
        return rc;
    return stage_fetch(m, &st);
}

// ---- Sim3 optimisation (kernel: orbhip_sim3opt.hip) ----------------------------------------------------------------------
static int sim3opt_args(int C, int cur, const void *kf_index, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                        const orbhip_sim3_tables *t, int match_form, const float *inv_level_sigma2, float th2, const void *matched12,
                        const void *sim3, const void *S12, const void *report)
{
    if (C < 0 || cap < 1 || !cam || rows < 0 || np < 0 || pcap < 0 || np > pcap || cur < 0 || cur >= rows || !inv_level_sigma2 ||
        cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS || !(th2 > 0.f) || !kf_index || !matched12 || !sim3 || !S12 || !report ||
        (match_form != ORBHIP_SIM3_MATCH_POINTS && match_form != ORBHIP_SIM3_MATCH_SLOTS))
        return ORBHIP_E_ARG;
    if (!t || !t->slot_point || !t->obs_start || !t->obs_kf || !t->obs_idx || !t->flags || !t->world || !t->Tcw || !t->kps || !t->n)
        return ORBHIP_E_ARG;
    if (cap > kS3oCapMax) { set_error("optimize_sim3: capacity %d exceeds %d", cap, kS3oCapMax); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

static int sim3opt_launch(orbhip_matcher *m, int C, int cur, const void *d_kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                          const orbhip_sim3_tables *t, int match_form, const float *inv_level_sigma2, float th2, int fix_scale,
                          const void *d_select, void *d_matched12, const void *d_sim3, void *d_S12, void *d_Scw, void *d_report)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    S3oArgs A;
    memset(&A, 0, sizeof(A));
    A.T.slot_point = (const int *)t->slot_point; A.T.n = (const int *)t->n; A.T.obs_start = (const int *)t->obs_start;
    A.T.obs_kf = (const int *)t->obs_kf; A.T.obs_idx = (const int *)t->obs_idx; A.T.flags = (const uint8_t *)t->flags;
    A.T.rows = rows; A.T.cap = cap; A.T.np = np; A.T.cur = cur; A.T.match_form = match_form;
    A.kps = (const orbhip_keypoint *)t->kps; A.world = (const float *)t->world; A.Tcw = (const float *)t->Tcw;
    A.kf_index = (const int *)d_kf_index; A.select = (const uint8_t *)d_select; A.sim3 = (const float *)d_sim3;
    A.matched12 = (int *)d_matched12; A.S12 = (double *)d_S12; A.Scw = (float *)d_Scw; A.report = (int *)d_report;
    fill_inv_sigma2(A.inv, cam, inv_level_sigma2);
    A.cam.fx = (double)cam->fx; A.cam.fy = (double)cam->fy; A.cam.cx = (double)cam->cx; A.cam.cy = (double)cam->cy;
    A.delta = (double)std::sqrt(th2);                                          // src/Optimizer.cc:1095: a float
    A.th2 = (double)th2;
    A.C = C; A.n_levels = cam->n_levels; A.fix_scale = fix_scale != 0;
    return launch_optimize_sim3(m->stream, A);
}

int orbhip_optimize_sim3_device(orbhip_matcher *m, int C, int cur, const void *d_kf_index, const orbhip_camera *cam, int rows, int cap,
                                int np, int pcap, const orbhip_sim3_tables *t, int match_form, const float *inv_level_sigma2, float th2,
                                int fix_scale, const void *d_select, void *d_matched12, const void *d_sim3, void *d_S12, void *d_Scw,
                                void *d_report)
{
    if (int rc = sim3opt_args(C, cur, d_kf_index, cam, rows, cap, np, pcap, t, match_form, inv_level_sigma2, th2, d_matched12, d_sim3,
                              d_S12, d_report))
        return rc;
    if (!m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    return sim3opt_launch(m, C, cur, d_kf_index, cam, rows, cap, np, t, match_form, inv_level_sigma2, th2, fix_scale, d_select,
                          d_matched12, d_sim3, d_S12, d_Scw, d_report);
}

int orbhip_optimize_sim3(orbhip_matcher *m, int C, int cur, const int32_t *kf_index, const orbhip_camera *cam, int rows, int cap, int np,
                         int pcap, const orbhip_sim3_tables *t, int match_form, const float *inv_level_sigma2, float th2, int fix_scale,
                         const uint8_t *select, int32_t *matched12, const float *sim3, double *S12, float *Scw, int32_t *report)
{
    if (int rc = sim3opt_args(C, cur, kf_index, cam, rows, cap, np, pcap, t, match_form, inv_level_sigma2, th2, matched12, sim3, S12,
                              report))
        return rc;
    if (int rc = sim3_check_tables("optimize_sim3", cam, rows, cap, np, t)) return rc;
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n, *obs_start = (const int32_t *)t->obs_start;
    const orbhip_keypoint *kps = (const orbhip_keypoint *)t->kps;
    for (int i = 0; i < n[cur]; ++i) {
        const size_t k = (size_t)cur * cap + i;
        if (slot_point[k] >= 0 && (kps[k].octave < 0 || kps[k].octave >= cam->n_levels)) {
            set_error("optimize_sim3: key point %d of the current key frame has octave %d", i, kps[k].octave);
            return ORBHIP_E_ARG;
        }
    }
    for (int c = 0; c < C; ++c) {
        const int kf = kf_index[c];
        if (kf < 0 || kf >= rows) { set_error("optimize_sim3: candidate %d (row %d) is outside the bank", c, kf); return ORBHIP_E_ARG; }
        const int32_t *mt = matched12 + (size_t)c * cap;
        for (int i1 = 0; i1 < n[cur]; ++i1)
            if (mt[i1] >= (match_form == ORBHIP_SIM3_MATCH_SLOTS ? cap : np)) { set_error("optimize_sim3: match %d of candidate %d is out of range", i1, c); return ORBHIP_E_ARG; }
    }
    if (!m) return ORBHIP_E_ARG;
    if (C == 0) return ORBHIP_OK;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t RC = (size_t)rows * cap, P = (size_t)np, Cn = (size_t)C, CC = Cn * cap, total = (size_t)obs_start[np];
    Stage st;
    int rc;
    orbhip_sim3_tables dt;
    const int32_t *d_kf;
    const uint8_t *d_sel;
    const float *d_sim3;
    int32_t *d_matched, *d_rep;
    double *d_S12;
    float *d_Scw;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dt.slot_point = stg.put(slot_point, RC); dt.obs_start = stg.put(obs_start, P + 1);
            dt.obs_kf = stg.put((const int32_t *)t->obs_kf, total); dt.obs_idx = stg.put((const int32_t *)t->obs_idx, total);
            dt.flags = stg.put((const uint8_t *)t->flags, P); dt.world = stg.put((const float *)t->world, P * 3);
            dt.Tcw = stg.put((const float *)t->Tcw, (size_t)rows * 12); dt.kps = stg.put(kps, RC); dt.n = stg.put(n, (size_t)rows);
            d_kf = stg.put(kf_index, Cn);
            d_sel = select ? stg.put(select, Cn) : nullptr;
            d_sim3 = stg.put(sim3, Cn * 16);
            d_matched = stg.inout(matched12, CC);
            d_S12 = stg.inout(S12, Cn * 8);
            d_Scw = Scw ? stg.inout(Scw, Cn * 12) : nullptr;
            d_rep = stg.inout(report, Cn * 8);
        }))) return rc;
    if ((rc = sim3opt_launch(m, C, cur, d_kf, cam, rows, cap, np, &dt, match_form, inv_level_sigma2, th2, fix_scale, d_sel, d_matched,
                             d_sim3, d_S12, d_Scw, d_rep)))
        return rc;
    return stage_fetch(m, &st);
}

// ---- local bundle adjustment (kernels: orbhip_lba.hip) ---------------------------------------------------------------------
static int lba_args(int cur, int id0_row, const orbhip_camera *cam, int rows, int cap, int np, int pcap, const orbhip_lba_tables *t,
                    const float *inv_level_sigma2, int max_points, int max_edges, const orbhip_lba_out *out)
{
    if (!cam || rows < 0 || cap < 1 || np < 0 || pcap < 0 || np > pcap || cur < 0 || cur >= rows || id0_row < -1 || id0_row >= rows ||
        max_points < 1 || max_edges < 1 || !inv_level_sigma2 || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS)
        return ORBHIP_E_ARG;
    if (!t || !t->slot_point || !t->n || !t->obs_start || !t->obs_kf || !t->obs_idx || !t->flags || !t->kps || !t->ord_kf || !t->n_ord ||
        !t->Tcw || !t->world || !out || !out->local_kf || !out->fixed_kf || !out->local_point || !out->erase || !out->report)
        return ORBHIP_E_ARG;
    if (cap > 4096 || rows > 4096) { set_error("local_bundle_adjustment: rows %d or capacity %d exceeds 4096", rows, cap); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

static int lba_launch(orbhip_matcher *m, int cur, int id0_row, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                      const orbhip_lba_tables *t, const float *inv_level_sigma2, int max_points, int max_edges, const void *d_stop,
                      const orbhip_lba_out *out)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    LbaWs W;
    memset(&W, 0, sizeof(W));
    W.slot_point = (const int *)t->slot_point; W.n = (const int *)t->n; W.kf_bad = (const uint8_t *)t->kf_bad;
    W.obs_start = (const int *)t->obs_start; W.obs_kf = (const int *)t->obs_kf; W.obs_idx = (const int *)t->obs_idx;
    W.flags = (const uint8_t *)t->flags; W.kps = (const orbhip_keypoint *)t->kps; W.u_right = (const float *)t->u_right;
    W.ord_kf = (const int *)t->ord_kf; W.n_ord = (const int *)t->n_ord; W.Tcw = (float *)t->Tcw; W.world = (float *)t->world;
    W.o_local_kf = (int *)out->local_kf; W.o_fixed_kf = (int *)out->fixed_kf; W.o_local_point = (int *)out->local_point;
    W.o_erase = (int *)out->erase; W.o_report = (int *)out->report;
    W.stop = (const uint8_t *)d_stop;
    fill_inv_sigma2(W.inv, cam, inv_level_sigma2);
    W.cam = po_cam(cam, 5.991, 7.815);                                        // src/Optimizer.cc:569-570
    W.cur = cur; W.id0_row = id0_row; W.rows = rows; W.cap = cap; W.np = np; W.pcap = pcap; W.n_levels = cam->n_levels;
    W.max_points = max_points; W.max_edges = max_edges;
    void *ws;
    if (int rc = scratch(m, S_LBA, lba_workspace_bytes(W), &ws)) return rc;
    return launch_local_bundle_adjustment(m->stream, W, ws);
}

int orbhip_local_bundle_adjustment_device(orbhip_matcher *m, int cur, int id0_row, const orbhip_camera *cam, int rows, int cap, int np,
                                          int pcap, const orbhip_lba_tables *tables, const float *inv_level_sigma2, int max_points,
                                          int max_edges, const void *d_stop, const orbhip_lba_out *out)
{
    if (int rc = lba_args(cur, id0_row, cam, rows, cap, np, pcap, tables, inv_level_sigma2, max_points, max_edges, out)) return rc;
    if (!m) return ORBHIP_E_ARG;
    return lba_launch(m, cur, id0_row, cam, rows, cap, np, pcap, tables, inv_level_sigma2, max_points, max_edges, d_stop, out);
}

int orbhip_local_bundle_adjustment(orbhip_matcher *m, int cur, int id0_row, const orbhip_camera *cam, int rows, int cap, int np,
                                   int pcap, const orbhip_lba_tables *t, const float *inv_level_sigma2, int max_points, int max_edges,
                                   const uint8_t *stop, const orbhip_lba_out *out)
{
    if (int rc = lba_args(cur, id0_row, cam, rows, cap, np, pcap, t, inv_level_sigma2, max_points, max_edges, out)) return rc;
    const int32_t *slot_point = (const int32_t *)t->slot_point, *n = (const int32_t *)t->n, *obs_start = (const int32_t *)t->obs_start;
    const int32_t *obs_kf = (const int32_t *)t->obs_kf, *obs_idx = (const int32_t *)t->obs_idx;
    const int32_t *ord_kf = (const int32_t *)t->ord_kf, *n_ord = (const int32_t *)t->n_ord;
    const orbhip_keypoint *kps = (const orbhip_keypoint *)t->kps;
    const size_t R = (size_t)rows, RC = R * cap, P = (size_t)pcap;
    for (int r = 0; r < rows; ++r) {
        if (n[r] < 0 || n[r] > cap) { set_error("local_bundle_adjustment: bank row %d holds a count outside [0, cap]", r); return ORBHIP_E_ARG; }
        if (n_ord[r] < 0 || n_ord[r] > rows) { set_error("local_bundle_adjustment: n_ord[%d] is outside [0, rows]", r); return ORBHIP_E_ARG; }
    }
    for (size_t i = 0; i < RC; ++i)
        if (slot_point[i] < -1 || slot_point[i] >= np) { set_error("local_bundle_adjustment: bank row %zu holds a point index out of range", i / cap); return ORBHIP_E_ARG; }
    for (int i = 0; i < n_ord[cur]; ++i)
        if (ord_kf[(size_t)cur * rows + i] < 0 || ord_kf[(size_t)cur * rows + i] >= rows) { set_error("local_bundle_adjustment: covisible entry %d is outside the bank", i); return ORBHIP_E_ARG; }
    if (obs_start[0] < 0) { set_error("local_bundle_adjustment: obs_start must start at 0 or above"); return ORBHIP_E_ARG; }
    for (int p = 0; p < np; ++p)
        if (obs_start[p + 1] < obs_start[p]) { set_error("local_bundle_adjustment: obs_start must be non-decreasing (entry %d)", p); return ORBHIP_E_ARG; }
    const size_t total = (size_t)obs_start[np];
    for (size_t o = (size_t)obs_start[0]; o < total; ++o) {
        if (obs_kf[o] < 0 || obs_kf[o] >= rows || obs_idx[o] < 0 || obs_idx[o] >= cap) { set_error("local_bundle_adjustment: observation %zu is outside the bank", o); return ORBHIP_E_ARG; }
        const int oct = kps[(size_t)obs_kf[o] * cap + obs_idx[o]].octave;
        if (oct < 0 || oct >= cam->n_levels) { set_error("local_bundle_adjustment: observation %zu names a key point of octave %d", o, oct); return ORBHIP_E_ARG; }
    }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t MP = (size_t)max_points, ME = (size_t)max_edges;
    Stage st;
    int rc;
    orbhip_lba_tables dt;
    orbhip_lba_out dout;
    const uint8_t *d_stop;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dt.slot_point = stg.put(slot_point, RC); dt.n = stg.put(n, R);
            dt.kf_bad = t->kf_bad ? stg.put((const uint8_t *)t->kf_bad, R) : nullptr;
            dt.obs_start = stg.put(obs_start, (size_t)np + 1); dt.obs_kf = stg.put(obs_kf, total); dt.obs_idx = stg.put(obs_idx, total);
            dt.flags = stg.put((const uint8_t *)t->flags, P); dt.kps = stg.put(kps, RC);
            dt.u_right = t->u_right ? stg.put((const float *)t->u_right, RC) : nullptr;
            dt.ord_kf = stg.put(ord_kf, R * R); dt.n_ord = stg.put(n_ord, R);
            d_stop = stop ? stg.put(stop, 1) : nullptr;
            dt.Tcw = stg.inout((float *)t->Tcw, R * 12);
            dt.world = stg.inout((float *)t->world, P * 3);
            dout.local_kf = stg.inout((int32_t *)out->local_kf, R); dout.fixed_kf = stg.inout((int32_t *)out->fixed_kf, R);
            dout.local_point = stg.inout((int32_t *)out->local_point, MP); dout.erase = stg.inout((int32_t *)out->erase, ME * 3);
            dout.report = stg.inout((int32_t *)out->report, 16);
        }))) return rc;
    if ((rc = lba_launch(m, cur, id0_row, cam, rows, cap, np, pcap, &dt, inv_level_sigma2, max_points, max_edges, d_stop, &dout))) return rc;
    return stage_fetch(m, &st);
}

// ---- essential-graph optimisation (kernels: orbhip_essgraph.hip) -------------------------------------------------------------
static int eg_args(int cur, int loop_row, int rows, int pcap, const orbhip_eg_tables *t, int max_edges, const orbhip_eg_out *out)
{
    if (rows < 1 || pcap < 0 || cur < 0 || cur >= rows || loop_row < 0 || loop_row >= rows || max_edges < 1) return ORBHIP_E_ARG;
    if (!t || !t->kf_id || !t->parent || !t->conn_w || !t->ord_kf || !t->ord_w || !t->n_ord || !t->loop_start || !t->loop_kf ||
        !t->lc_start || !t->lc_kf || !t->corrected || !t->non_corrected || !t->in_corrected || !t->in_non_corrected || !t->Tcw ||
        (pcap > 0 && (!t->flags || !t->ref_kf || !t->corrected_by_kf || !t->corrected_ref || !t->world)) || !out ||
        (pcap > 0 && !out->point_list) || !out->Scw || !out->Swc || !out->report)
        return ORBHIP_E_ARG;
    if (rows > 4096) { set_error("optimize_essential_graph: rows %d exceeds 4096", rows); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

static int eg_launch(orbhip_matcher *m, int cur, int loop_row, int rows, int pcap, const orbhip_eg_tables *t, int fix_scale, int max_edges,
                     const orbhip_eg_out *out)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    EgWs W;
    memset(&W, 0, sizeof(W));
    W.kf_bad = (const uint8_t *)t->kf_bad; W.kf_id = (const int *)t->kf_id; W.parent = (const int *)t->parent;
    W.conn_w = (const int *)t->conn_w; W.ord_kf = (const int *)t->ord_kf; W.ord_w = (const int *)t->ord_w; W.n_ord = (const int *)t->n_ord;
    W.loop_start = (const int *)t->loop_start; W.loop_kf = (const int *)t->loop_kf; W.lc_start = (const int *)t->lc_start;
    W.lc_kf = (const int *)t->lc_kf; W.corrected = (const double *)t->corrected; W.non_corrected = (const double *)t->non_corrected;
    W.in_c = (const uint8_t *)t->in_corrected; W.in_nc = (const uint8_t *)t->in_non_corrected; W.flags = (const uint8_t *)t->flags;
    W.ref_kf = (const int *)t->ref_kf; W.cby = (const int *)t->corrected_by_kf; W.cref = (const int *)t->corrected_ref;
    W.Tcw = (float *)t->Tcw; W.world = (float *)t->world;
    W.o_point_list = (int *)out->point_list; W.o_Scw = (double *)out->Scw; W.o_Swc = (double *)out->Swc; W.o_report = (int *)out->report;
    W.rows = rows; W.pcap = pcap; W.cur = cur; W.loop_row = loop_row; W.fix_scale = fix_scale ? 1 : 0; W.max_edges = max_edges;
    void *ws;
    if (int rc = scratch(m, S_EG, eg_workspace_bytes(W), &ws)) return rc;
    if (!m->h_eg) ORBHIP_HIP_CHECK(hipHostMalloc(&m->h_eg, sizeof(EgState), hipHostMallocDefault));
    return launch_optimize_essential_graph(m->stream, W, ws, (EgState *)m->h_eg, m->eg_counters);
}

int orbhip_optimize_essential_graph_device(orbhip_matcher *m, int cur, int loop_row, int rows, int pcap, const orbhip_eg_tables *tables,
                                           int fix_scale, int max_edges, const orbhip_eg_out *out)
{
    if (int rc = eg_args(cur, loop_row, rows, pcap, tables, max_edges, out)) return rc;
    if (!m) return ORBHIP_E_ARG;
    return eg_launch(m, cur, loop_row, rows, pcap, tables, fix_scale, max_edges, out);
}

int orbhip_optimize_essential_graph(orbhip_matcher *m, int cur, int loop_row, int rows, int pcap, const orbhip_eg_tables *t,
                                    int fix_scale, int max_edges, const orbhip_eg_out *out)
{
    if (int rc = eg_args(cur, loop_row, rows, pcap, t, max_edges, out)) return rc;
    const uint8_t *kf_bad = (const uint8_t *)t->kf_bad;
    const int32_t *parent = (const int32_t *)t->parent, *ord_kf = (const int32_t *)t->ord_kf, *n_ord = (const int32_t *)t->n_ord;
    const int32_t *starts[2] = {(const int32_t *)t->loop_start, (const int32_t *)t->lc_start};
    const int32_t *lists[2] = {(const int32_t *)t->loop_kf, (const int32_t *)t->lc_kf};
    const int32_t *ref_kf = (const int32_t *)t->ref_kf, *cref = (const int32_t *)t->corrected_ref;
    const char *names[2] = {"loop_kf", "lc_kf"};
    auto bad = [&](int r) { return kf_bad && kf_bad[r]; };
    for (int r = 0; r < rows; ++r) {
        if (parent[r] < -1 || parent[r] >= rows) { set_error("optimize_essential_graph: parent[%d] is outside [-1, rows)", r); return ORBHIP_E_ARG; }
        if (n_ord[r] < 0 || n_ord[r] > rows) { set_error("optimize_essential_graph: n_ord[%d] is outside [0, rows]", r); return ORBHIP_E_ARG; }
        for (int i = 0; i < n_ord[r]; ++i)
            if (ord_kf[(size_t)r * rows + i] < 0 || ord_kf[(size_t)r * rows + i] >= rows) { set_error("optimize_essential_graph: covisible entry %d of row %d is outside the bank", i, r); return ORBHIP_E_ARG; }
        if (!bad(r) && parent[r] >= 0 && bad(parent[r])) { set_error("optimize_essential_graph: the parent of row %d is a bad row", r); return ORBHIP_E_ARG; }
    }
    for (int k = 0; k < 2; ++k) {
        if (starts[k][0] != 0) { set_error("optimize_essential_graph: %s's start table must begin at 0", names[k]); return ORBHIP_E_ARG; }
        for (int r = 0; r < rows; ++r) {
            if (starts[k][r + 1] < starts[k][r]) { set_error("optimize_essential_graph: %s's start table must be non-decreasing (row %d)", names[k], r); return ORBHIP_E_ARG; }
            for (int o = starts[k][r]; o < starts[k][r + 1]; ++o) {
                const int j = lists[k][o];
                if (j < 0 || j >= rows || (o > starts[k][r] && j <= lists[k][o - 1])) { set_error("optimize_essential_graph: %s of row %d must hold ascending rows of the bank", names[k], r); return ORBHIP_E_ARG; }
                if ((k == 1 || !bad(r)) && (bad(j) || bad(r))) { set_error("optimize_essential_graph: %s of row %d joins a bad row (a null vertex)", names[k], r); return ORBHIP_E_ARG; }
            }
        }
    }
    for (int p = 0; p < pcap; ++p)
        if (ref_kf[p] < -1 || ref_kf[p] >= rows || cref[p] < -1 || cref[p] >= rows) { set_error("optimize_essential_graph: point %d names a reference row outside [-1, rows)", p); return ORBHIP_E_ARG; }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t R = (size_t)rows, P = (size_t)pcap, NL = (size_t)starts[0][rows], NC = (size_t)starts[1][rows];
    Stage st;
    int rc;
    const int32_t zero = 0;
    const uint8_t zb = 0;
    orbhip_eg_tables dt;
    orbhip_eg_out dout;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dt.kf_bad = kf_bad ? stg.put(kf_bad, R) : nullptr;
            dt.kf_id = stg.put((const int32_t *)t->kf_id, R); dt.parent = stg.put(parent, R);
            dt.conn_w = stg.put((const int32_t *)t->conn_w, R * R); dt.ord_kf = stg.put(ord_kf, R * R);
            dt.ord_w = stg.put((const int32_t *)t->ord_w, R * R);
            dt.n_ord = stg.put(n_ord, R);
            dt.loop_start = stg.put(starts[0], R + 1); dt.loop_kf = NL ? stg.put(lists[0], NL) : stg.put(&zero, 1);
            dt.lc_start = stg.put(starts[1], R + 1); dt.lc_kf = NC ? stg.put(lists[1], NC) : stg.put(&zero, 1);
            dt.corrected = stg.put((const double *)t->corrected, R * 8); dt.non_corrected = stg.put((const double *)t->non_corrected, R * 8);
            dt.in_corrected = stg.put((const uint8_t *)t->in_corrected, R);
            dt.in_non_corrected = stg.put((const uint8_t *)t->in_non_corrected, R);
            dt.flags = P ? stg.put((const uint8_t *)t->flags, P) : stg.put(&zb, 1);
            dt.ref_kf = P ? stg.put(ref_kf, P) : stg.put(&zero, 1);
            dt.corrected_by_kf = P ? stg.put((const int32_t *)t->corrected_by_kf, P) : stg.put(&zero, 1);
            dt.corrected_ref = P ? stg.put(cref, P) : stg.put(&zero, 1);
            dt.Tcw = stg.inout((float *)t->Tcw, R * 12);
            dt.world = P ? stg.inout((float *)t->world, P * 3) : stage_zeros<float>(stg, 3);
            dout.point_list = P ? stg.inout((int32_t *)out->point_list, P) : stage_zeros<int32_t>(stg, 1);
            dout.Scw = stg.inout((double *)out->Scw, R * 8); dout.Swc = stg.inout((double *)out->Swc, R * 8);
            dout.report = stg.inout((int32_t *)out->report, 16);
        }))) return rc;
    if ((rc = eg_launch(m, cur, loop_row, rows, pcap, &dt, fix_scale, max_edges, &dout))) return rc;
    return stage_fetch(m, &st);
}

int orbhip_optimize_essential_graph_counters(orbhip_matcher *m, int32_t counters[2])
{
    if (!m || !counters) return ORBHIP_E_ARG;
    counters[0] = m->eg_counters[0]; counters[1] = m->eg_counters[1];
    return ORBHIP_OK;
}

// ---- global bundle adjustment (kernels: orbhip_gba.hip) ----------------------------------------------------------------------
static int gba_args(const orbhip_camera *cam, int rows, int cap, int np, int pcap, const orbhip_gba_tables *t, const float *inv_level_sigma2,
                    const void *kf_list, int nkf, const void *pt_list, int npt, int iterations, int mode, int max_points, int max_edges,
                    const orbhip_gba_out *out)
{
    if (!cam || rows < 0 || cap < 1 || np < 0 || pcap < 0 || np > pcap || max_points < 1 || max_edges < 1 || !inv_level_sigma2 ||
        cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS || iterations < 1 || (mode != ORBHIP_GBA_IN_PLACE && mode != ORBHIP_GBA_STAGED) ||
        (kf_list && (nkf < 0 || nkf > rows)) || (pt_list && (npt < 0 || npt > pcap)))
        return ORBHIP_E_ARG;
    if (!t || !t->kf_id || !t->obs_start || !t->obs_kf || !t->obs_idx || !t->flags || !t->kps || !t->Tcw || !t->world || !out || !out->report)
        return ORBHIP_E_ARG;
    if (mode == ORBHIP_GBA_IN_PLACE ? !out->point_list : (!out->TcwGBA || !out->posGBA || !out->kf_mark || !out->pt_mark)) return ORBHIP_E_ARG;
    if (cap > 4096 || rows > 4096) { set_error("global_bundle_adjustment: rows %d or capacity %d exceeds 4096", rows, cap); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

static int gba_launch(orbhip_matcher *m, const orbhip_camera *cam, int rows, int cap, int np, int pcap, const orbhip_gba_tables *t,
                      const float *inv_level_sigma2, const void *d_kf_list, int nkf, const void *d_pt_list, int npt, int iterations,
                      int robust, int mode, int max_points, int max_edges, const void *d_stop, const orbhip_gba_out *out)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    GbaWs G;
    memset(&G, 0, sizeof(G));
    LbaWs &W = G.L;
    W.kf_bad = (const uint8_t *)t->kf_bad; W.obs_start = (const int *)t->obs_start; W.obs_kf = (const int *)t->obs_kf;
    W.obs_idx = (const int *)t->obs_idx; W.flags = (const uint8_t *)t->flags; W.kps = (const orbhip_keypoint *)t->kps;
    W.u_right = (const float *)t->u_right; W.Tcw = (float *)t->Tcw; W.world = (float *)t->world;
    W.stop = (const uint8_t *)d_stop;
    fill_inv_sigma2(W.inv, cam, inv_level_sigma2);
    W.cam = po_cam(cam, 5.99, 7.815);                                         // src/Optimizer.cc:85-86: 5.99, not 5.991
    W.cur = 0; W.id0_row = -1; W.rows = rows; W.cap = cap; W.np = np; W.pcap = pcap; W.n_levels = cam->n_levels;
    W.max_points = max_points; W.max_edges = max_edges;
    W.single_its = iterations; W.robust = robust ? 1 : 0;
    G.kf_id = (const int *)t->kf_id; G.kf_list = (const int *)d_kf_list; G.pt_list = (const int *)d_pt_list; G.nkf = nkf; G.npt = npt;
    G.mode = mode;
    G.TcwGBA = (float *)out->TcwGBA; G.posGBA = (float *)out->posGBA; G.kf_mark = (uint8_t *)out->kf_mark; G.pt_mark = (uint8_t *)out->pt_mark;
    G.o_point_list = (int *)out->point_list; G.o_report = (int *)out->report;
    void *ws;
    if (int rc = scratch(m, S_GBA, gba_workspace_bytes(G), &ws)) return rc;
    if (!m->h_gba) ORBHIP_HIP_CHECK(hipHostMalloc(&m->h_gba, sizeof(LbaState), hipHostMallocDefault));
    return launch_global_bundle_adjustment(m->stream, G, ws, (LbaState *)m->h_gba, m->gba_counters);
}

int orbhip_global_bundle_adjustment_device(orbhip_matcher *m, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                                           const orbhip_gba_tables *tables, const float *inv_level_sigma2, const void *d_kf_list,
                                           int nkf, const void *d_pt_list, int npt, int iterations, int robust, int mode,
                                           int max_points, int max_edges, const void *d_stop, const orbhip_gba_out *out)
{
    if (int rc = gba_args(cam, rows, cap, np, pcap, tables, inv_level_sigma2, d_kf_list, nkf, d_pt_list, npt, iterations, mode, max_points,
                          max_edges, out))
        return rc;
    if (!m) return ORBHIP_E_ARG;
    return gba_launch(m, cam, rows, cap, np, pcap, tables, inv_level_sigma2, d_kf_list, nkf, d_pt_list, npt, iterations, robust, mode,
                      max_points, max_edges, d_stop, out);
}

int orbhip_global_bundle_adjustment(orbhip_matcher *m, const orbhip_camera *cam, int rows, int cap, int np, int pcap,
                                    const orbhip_gba_tables *t, const float *inv_level_sigma2, const int32_t *kf_list, int nkf,
                                    const int32_t *pt_list, int npt, int iterations, int robust, int mode, int max_points,
                                    int max_edges, const uint8_t *stop, const orbhip_gba_out *out)
{
    if (int rc = gba_args(cam, rows, cap, np, pcap, t, inv_level_sigma2, kf_list, nkf, pt_list, npt, iterations, mode, max_points, max_edges, out))
        return rc;
    const uint8_t *kf_bad = (const uint8_t *)t->kf_bad;
    const int32_t *kf_id = (const int32_t *)t->kf_id, *obs_start = (const int32_t *)t->obs_start;
    const int32_t *obs_kf = (const int32_t *)t->obs_kf, *obs_idx = (const int32_t *)t->obs_idx;
    const orbhip_keypoint *kps = (const orbhip_keypoint *)t->kps;
    const uint8_t *flags = (const uint8_t *)t->flags;
    const size_t R = (size_t)rows, RC = R * cap, P = (size_t)pcap;
    auto bad = [&](int r) { return kf_bad && kf_bad[r]; };
    std::vector<uint8_t> listed(R, kf_list ? 0 : 1);
    int max_kfid = 0;
    if (kf_list)
        for (int i = 0; i < nkf; ++i) {
            const int r = kf_list[i];
            if (r < 0 || r >= rows || listed[r]) { set_error("global_bundle_adjustment: kf_list[%d] is outside the bank or repeats a row", i); return ORBHIP_E_ARG; }
            listed[r] = 1;
        }
    for (int r = 0; r < rows; ++r)
        if (listed[r] && !bad(r) && kf_id[r] > max_kfid) max_kfid = kf_id[r];
    if (pt_list)
        for (int i = 0; i < npt; ++i)
            if (pt_list[i] < 0 || pt_list[i] >= np) { set_error("global_bundle_adjustment: pt_list[%d] is outside [0, np)", i); return ORBHIP_E_ARG; }
    if (obs_start[0] < 0) { set_error("global_bundle_adjustment: obs_start must start at 0 or above"); return ORBHIP_E_ARG; }
    for (int p = 0; p < np; ++p)
        if (obs_start[p + 1] < obs_start[p]) { set_error("global_bundle_adjustment: obs_start must be non-decreasing (entry %d)", p); return ORBHIP_E_ARG; }
    const size_t total = (size_t)obs_start[np];
    for (size_t o = (size_t)obs_start[0]; o < total; ++o) {
        if (obs_kf[o] < 0 || obs_kf[o] >= rows || obs_idx[o] < 0 || obs_idx[o] >= cap) { set_error("global_bundle_adjustment: observation %zu is outside the bank", o); return ORBHIP_E_ARG; }
        const int oct = kps[(size_t)obs_kf[o] * cap + obs_idx[o]].octave;
        if (oct < 0 || oct >= cam->n_levels) { set_error("global_bundle_adjustment: observation %zu names a key point of octave %d", o, oct); return ORBHIP_E_ARG; }
    }
    for (int i = 0; i < (pt_list ? npt : np); ++i) {                         // a null vertex: optimizer.vertex(pKF->mnId) of a row not listed
        const int p = pt_list ? pt_list[i] : i;
        if (!(flags[p] & ORBHIP_POINT_PRESENT)) continue;
        for (int o = obs_start[p]; o < obs_start[p + 1]; ++o) {
            const int r = obs_kf[o];
            if (!bad(r) && kf_id[r] <= max_kfid && !listed[r]) { set_error("global_bundle_adjustment: point %d is observed by row %d, which is not listed (a null vertex)", p, r); return ORBHIP_E_ARG; }
        }
    }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t MP = (size_t)max_points, NK = kf_list ? (size_t)nkf : 0, NP = pt_list ? (size_t)npt : 0;
    const bool staged = mode == ORBHIP_GBA_STAGED;
    Stage st;
    int rc;
    const int32_t zero = 0;
    const uint8_t zb = 0;
    const float fz[3] = {0.f, 0.f, 0.f};
    orbhip_gba_tables dt;
    orbhip_gba_out dout;
    memset(&dout, 0, sizeof(dout));
    const int32_t *d_kfl, *d_ptl;
    const uint8_t *d_stop;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            dt.kf_bad = kf_bad ? stg.put(kf_bad, R) : nullptr; dt.kf_id = stg.put(kf_id, R);
            dt.obs_start = stg.put(obs_start, (size_t)np + 1);
            dt.obs_kf = total ? stg.put(obs_kf, total) : stg.put(&zero, 1); dt.obs_idx = total ? stg.put(obs_idx, total) : stg.put(&zero, 1);
            dt.flags = P ? stg.put(flags, P) : stg.put(&zb, 1); dt.kps = stg.put(kps, RC);
            dt.u_right = t->u_right ? stg.put((const float *)t->u_right, RC) : nullptr;
            d_kfl = kf_list ? (NK ? stg.put(kf_list, NK) : stg.put(&zero, 1)) : nullptr;
            d_ptl = pt_list ? (NP ? stg.put(pt_list, NP) : stg.put(&zero, 1)) : nullptr;
            d_stop = stop ? stg.put(stop, 1) : nullptr;
            // in place: the poses, the points and the list travel back; staged: the GBA copies and the marks do
            if (staged) {
                dt.Tcw = const_cast<float *>(stg.put((const float *)t->Tcw, R * 12));   // read only in this mode
                dt.world = const_cast<float *>(P ? stg.put((const float *)t->world, P * 3) : stg.put(fz, 3));
                dout.TcwGBA = stg.inout((float *)out->TcwGBA, R * 12);
                dout.posGBA = P ? stg.inout((float *)out->posGBA, P * 3) : stage_zeros<float>(stg, 3);
                dout.kf_mark = stg.inout((uint8_t *)out->kf_mark, R);
                dout.pt_mark = P ? stg.inout((uint8_t *)out->pt_mark, P) : stage_zeros<uint8_t>(stg, 1);
            } else {
                dt.Tcw = stg.inout((float *)t->Tcw, R * 12);
                dt.world = P ? stg.inout((float *)t->world, P * 3) : stage_zeros<float>(stg, 3);
                dout.point_list = stg.inout((int32_t *)out->point_list, MP);
            }
            dout.report = stg.inout((int32_t *)out->report, 16);
        }))) return rc;
    if ((rc = gba_launch(m, cam, rows, cap, np, pcap, &dt, inv_level_sigma2, d_kfl, nkf, d_ptl, npt, iterations, robust, mode, max_points,
                         max_edges, d_stop, &dout)))
        return rc;
    return stage_fetch(m, &st);
}

int orbhip_global_bundle_adjustment_counters(orbhip_matcher *m, int32_t counters[2])
{
    if (!m || !counters) return ORBHIP_E_ARG;
    counters[0] = m->gba_counters[0]; counters[1] = m->gba_counters[1];
    return ORBHIP_OK;
}

static int gba_apply_args(int n_origins, int rows, int pcap, const orbhip_gba_apply *a)
{
    if (rows < 1 || pcap < 0 || n_origins < 0) return ORBHIP_E_ARG;
    if (!a || (n_origins > 0 && !a->origins) || !a->parent || !a->kf_mark || !a->TcwGBA || !a->Tcw || !a->TcwBefGBA || !a->report ||
        (pcap > 0 && (!a->pt_mark || !a->posGBA || !a->flags || !a->ref_kf || !a->world)))
        return ORBHIP_E_ARG;
    if (rows > 4096) { set_error("apply_global_ba: rows %d exceeds 4096", rows); return ORBHIP_E_CAPACITY; }
    return ORBHIP_OK;
}

static int gba_apply_launch(orbhip_matcher *m, int n_origins, int rows, int pcap, const orbhip_gba_apply *a)
{
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    GbaApply A;
    memset(&A, 0, sizeof(A));
    A.origins = (const int *)a->origins; A.parent = (const int *)a->parent; A.kf_bad = (const uint8_t *)a->kf_bad;
    A.kf_mark = (uint8_t *)a->kf_mark; A.TcwGBA = (float *)a->TcwGBA; A.Tcw = (float *)a->Tcw; A.TcwBef = (float *)a->TcwBefGBA;
    A.pt_mark = (const uint8_t *)a->pt_mark; A.flags = (const uint8_t *)a->flags; A.posGBA = (const float *)a->posGBA;
    A.ref_kf = (const int *)a->ref_kf; A.world = (float *)a->world; A.o_report = (int *)a->report;
    A.n_origins = n_origins; A.rows = rows; A.pcap = pcap;
    void *ws;
    if (int rc = scratch(m, S_GBAAPPLY, gba_apply_workspace_bytes(A), &ws)) return rc;
    return launch_apply_global_ba(m->stream, A, ws);
}

int orbhip_apply_global_ba_device(orbhip_matcher *m, int n_origins, int rows, int pcap, const orbhip_gba_apply *a)
{
    if (int rc = gba_apply_args(n_origins, rows, pcap, a)) return rc;
    if (!m) return ORBHIP_E_ARG;
    return gba_apply_launch(m, n_origins, rows, pcap, a);
}

int orbhip_apply_global_ba(orbhip_matcher *m, int n_origins, int rows, int pcap, const orbhip_gba_apply *a)
{
    if (int rc = gba_apply_args(n_origins, rows, pcap, a)) return rc;
    const int32_t *origins = (const int32_t *)a->origins, *parent = (const int32_t *)a->parent, *ref_kf = (const int32_t *)a->ref_kf;
    const uint8_t *kf_bad = (const uint8_t *)a->kf_bad, *kf_mark = (const uint8_t *)a->kf_mark;
    for (int i = 0; i < n_origins; ++i) {
        const int r = origins[i];
        if (r < 0 || r >= rows || (kf_bad && kf_bad[r]) || !kf_mark[r]) { set_error("apply_global_ba: origin %d must be a marked row of the map", i); return ORBHIP_E_ARG; }
    }
    for (int r = 0; r < rows; ++r)
        if (parent[r] < -1 || parent[r] >= rows) { set_error("apply_global_ba: parent[%d] is outside [-1, rows)", r); return ORBHIP_E_ARG; }
    for (int p = 0; p < pcap; ++p)
        if (ref_kf[p] < -1 || ref_kf[p] >= rows) { set_error("apply_global_ba: point %d names a reference row outside [-1, rows)", p); return ORBHIP_E_ARG; }
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    const size_t R = (size_t)rows, P = (size_t)pcap, NO = (size_t)n_origins;
    Stage st;
    int rc;
    const int32_t zero = 0;
    const uint8_t zb = 0;
    const float fz[3] = {0.f, 0.f, 0.f};
    orbhip_gba_apply d;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d.origins = NO ? stg.put(origins, NO) : stg.put(&zero, 1); d.parent = stg.put(parent, R);
            d.kf_bad = kf_bad ? stg.put(kf_bad, R) : nullptr;
            d.pt_mark = P ? stg.put((const uint8_t *)a->pt_mark, P) : stg.put(&zb, 1);
            d.posGBA = P ? stg.put((const float *)a->posGBA, P * 3) : stg.put(fz, 3);
            d.flags = P ? stg.put((const uint8_t *)a->flags, P) : stg.put(&zb, 1);
            d.ref_kf = P ? stg.put(ref_kf, P) : stg.put(&zero, 1);
            d.kf_mark = stg.inout((uint8_t *)a->kf_mark, R);
            d.TcwGBA = stg.inout((float *)a->TcwGBA, R * 12); d.Tcw = stg.inout((float *)a->Tcw, R * 12);
            d.TcwBefGBA = stg.inout((float *)a->TcwBefGBA, R * 12);
            d.world = P ? stg.inout((float *)a->world, P * 3) : stage_zeros<float>(stg, 3);
            d.report = stg.inout((int32_t *)a->report, 8);
        }))) return rc;
    if ((rc = gba_apply_launch(m, n_origins, rows, pcap, &d))) return rc;
    return stage_fetch(m, &st);
}

#ifdef ORBHIP_DEVTOOLS
// development builds: {workgroups, sum of rounds, max rounds} of the parallel resolve since the last call
int orbhip_dev_resolve_stats(unsigned int out[4])
{
    unsigned int z[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(orbhip::g_resolve_stats), sizeof(z)) != hipSuccess) return ORBHIP_E_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(orbhip::g_resolve_stats), z, sizeof(z)) != hipSuccess) return ORBHIP_E_HIP;
    return ORBHIP_OK;
}
// development builds: what the window search of this handle's last windowed search left for the resolve -- cnt[nlists] and
// the compact rows ccand[nlists * 64] (nlists = pairs x query capacity of that call); synchronises the stream
int orbhip_dev_window_lists(orbhip_matcher *m, int nlists, int *cnt, unsigned long long *ccand)
{
    if (!m || nlists < 1 || !cnt || !ccand) return ORBHIP_E_ARG;
    const size_t n = (size_t)nlists;
    if (m->cap[S_CNT] < n * sizeof(int) || m->cap[S_CCAND] < n * kCompact * sizeof(unsigned long long)) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
    ORBHIP_HIP_CHECK(hipMemcpy(cnt, m->buf[S_CNT], n * sizeof(int), hipMemcpyDeviceToHost));
    ORBHIP_HIP_CHECK(hipMemcpy(ccand, m->buf[S_CCAND], n * kCompact * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ORBHIP_OK;
}
// development builds: the LDS-state parallel resolve of this handle runs its stamped instantiation (on != 0) ...
int orbhip_dev_set_resolve_stamps(orbhip_matcher *m, int on)
{
    if (!m) return ORBHIP_E_ARG;
    m->resolve_stamps = on != 0;
    return ORBHIP_OK;
}
// ... and its per-phase clock sums since the last call: {state init + head loads, first full step, event-driven rounds,
// unobserved pass, assign + histogram, cull, output, workgroups}.  The caller synchronises the stream first.
int orbhip_dev_resolve_stamps(unsigned long long out[8])
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(orbhip::g_resolve_stamps), sizeof(z)) != hipSuccess) return ORBHIP_E_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(orbhip::g_resolve_stamps), z, sizeof(z)) != hipSuccess) return ORBHIP_E_HIP;
    return ORBHIP_OK;
}
#endif

int orbhip_keyframe_queries(orbhip_matcher *m, const orbhip_camera *cam, int mode, int double_invz, const float *T1,
                            const float *T2, int n, const float *world, const float *normal, const float *max_dist,
                            const float *min_dist, const uint8_t *flags, float th, orbhip_query *q)
{
    if (!m || !cam || n < 0 || !T1 || !q || (mode != 0 && mode != 1) || (mode == 1 && !T2) || cam->n_levels < 1 ||
        cam->n_levels > ORBHIP_MAX_LEVELS)
        return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    if (!world || !max_dist || !min_dist || !flags || (mode == 0 && !normal)) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    Stage st;
    KfQueryArgs A;
    int rc = stage_send(m, &st, [&](Stage &stg) {
        A.T1 = stg.put(T1, 12);
        A.T2 = T2 ? stg.put(T2, 12) : nullptr;
        A.world = stg.put(world, (size_t)n * 3);
        A.normal = normal ? stg.put(normal, (size_t)n * 3) : nullptr;
        A.max_dist = stg.put(max_dist, (size_t)n);
        A.min_dist = stg.put(min_dist, (size_t)n);
        A.flags = stg.put(flags, (size_t)n);
    });
    if (rc) return rc;
    A.n = n; A.mode = mode; A.double_invz = double_invz;
    void *p;
    if ((rc = scratch(m, S_Q, (size_t)n * sizeof(orbhip_query), &p))) return rc;
    A.q = (orbhip_query *)p;
    hipLaunchKernelGGL(k_keyframe_queries, dim3((n + 255) / 256), dim3(256), 0, m->stream, A, *cam, th);
    const uint8_t *h;
    if ((rc = read_back(m, p, (size_t)n * sizeof(orbhip_query), &h))) return rc;
    memcpy(q, h, (size_t)n * sizeof(orbhip_query));
    return ORBHIP_OK;
}

int orbhip_fuse(orbhip_matcher *m, const orbhip_frame_view *kf, const orbhip_camera *cam, const float *Tcw, int sim3_form,
                int n, const float *world, const float *normal, const float *max_dist, const float *min_dist,
                const uint8_t *flags, const uint8_t *point_desc, float th, const float *inv_level_sigma2, int32_t *best_idx,
                int32_t *best_dist)
{
    if (!m || !kf || n < 0 || (n > 0 && (!best_idx || !best_dist || !point_desc))) return ORBHIP_E_ARG;
    if (n == 0) return ORBHIP_OK;
    static thread_local std::vector<orbhip_query> q;
    q.resize((size_t)n);
    int rc = orbhip_keyframe_queries(m, cam, 0, sim3_form ? 1 : 0, Tcw, nullptr, n, world, normal, max_dist, min_dist, flags, th, q.data());
    if (rc) return rc;
    // the Scw overload (src/ORBmatcher.cc:1062-1079) has no chi-square gate
    return orbhip_search_best_in_window(m, kf, q.data(), point_desc, n, sim3_form ? 0 : 1, inv_level_sigma2, best_idx, best_dist);
}

// lanes per query of k_fuse_batch: 8 is the mapping kept; development builds can select the
// one-wavefront-per-query mapping for tools/bench_fuse.py
static int g_fuse_lanes = 8;
#ifdef ORBHIP_DEVTOOLS
// lanes per query of k_window_search for every windowed search of this handle: 16 / 64, 0 = the product rule
int orbhip_dev_set_window_lanes(orbhip_matcher *m, int lanes)
{
    if (!m || (lanes != 0 && lanes != 16 && lanes != 64)) return ORBHIP_E_ARG;
    m->window_lanes = lanes;
    return ORBHIP_OK;
}
int orbhip_dev_fuse_lanes(int lanes)
{
    if (lanes != 8 && lanes != 64) return ORBHIP_E_ARG;
    g_fuse_lanes = lanes;
    return ORBHIP_OK;
}
#endif

int orbhip_fuse_device(orbhip_matcher *m, int K, const void *d_kf_index, const orbhip_camera *cam, const void *d_Tcw,
                       int sim3_form, const void *d_kps, const void *d_desc, const void *d_n, int cap, const void *d_u_right,
                       const void *d_cell_start, const void *d_cell_items, int np, int pcap, const void *d_world,
                       const void *d_normal, const void *d_max_dist, const void *d_min_dist, const void *d_point_desc,
                       const void *d_flags, float th, const float *inv_level_sigma2, void *d_best_idx, void *d_best_dist,
                       void *d_q)
{
    if (!m || K < 0 || np < 0 || np > pcap || cap < 1 || !cam || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS)
        return ORBHIP_E_ARG;
    if (cap > kGridMax) { set_error("fuse_device: capacity %d exceeds %d", cap, kGridMax); return ORBHIP_E_CAPACITY; }
    if ((d_cell_start == nullptr) != (d_cell_items == nullptr)) return ORBHIP_E_ARG;
    if (K == 0 || np == 0) return ORBHIP_OK;
    if (!d_kf_index || !d_Tcw || !d_kps || !d_desc || !d_n || !d_world || !d_normal || !d_max_dist || !d_min_dist ||
        !d_point_desc || !d_flags || !inv_level_sigma2 || !d_best_idx || !d_best_dist)
        return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    FuseBatchArgs A;
    A.kf_index = (const int *)d_kf_index; A.Tcw = (const float *)d_Tcw;
    A.keys = (const orbhip_keypoint *)d_kps; A.desc = (const uint8_t *)d_desc; A.n_dev = (const int *)d_n;
    A.u_right = (const float *)d_u_right;
    A.cell_start = (const int *)d_cell_start; A.cell_items = (const int *)d_cell_items;
    A.world = (const float *)d_world; A.normal = (const float *)d_normal;
    A.max_dist = (const float *)d_max_dist; A.min_dist = (const float *)d_min_dist;
    A.point_desc = (const uint8_t *)d_point_desc; A.flags = (const uint8_t *)d_flags;
    A.best_idx = (int *)d_best_idx; A.best_dist = (int *)d_best_dist; A.q = (orbhip_query *)d_q;
    A.cap = cap; A.np = np; A.pcap = pcap; A.sim3_form = sim3_form ? 1 : 0; A.csr_by_target = 0;
    const GridInv inv = grid_inv(cam);
    A.min_x = cam->min_x; A.min_y = cam->min_y; A.inv_w = inv.w; A.inv_h = inv.h;
    if (!d_cell_start) {   // mGrid of the K targets into the handle's scratch: cell_of | cell_items | cell_start
        void *p;
        const size_t rows = al256((size_t)K * cap * sizeof(int));
        if (int rc = scratch(m, S_CSR, 2 * rows + (size_t)K * (kGridCells + 1) * sizeof(int), &p)) return rc;
        int *cell_of = (int *)p, *cell_items = (int *)((uint8_t *)p + rows), *cell_start = (int *)((uint8_t *)p + 2 * rows);
        const DevFrame D = dev_frame(0, A.keys, nullptr, nullptr, A.min_x, A.min_y, A.inv_w, A.inv_h);
        hipLaunchKernelGGL(k_grid_csr_indexed, dim3(K), dim3(1024), 0, m->stream, D, A.kf_index, A.n_dev, cap, cell_of,
                           cell_start, cell_items);
        A.cell_start = cell_start; A.cell_items = cell_items; A.csr_by_target = 1;
    }
    const SigmaTab sig = sigma_tab(inv_level_sigma2, cam->n_levels);
    const dim3 grid((np + 255) / 256, K);
    if (g_fuse_lanes == 64) hipLaunchKernelGGL(k_fuse_batch<64>, grid, dim3(256), 0, m->stream, A, *cam, th, sig);
    else hipLaunchKernelGGL(k_fuse_batch<8>, grid, dim3(256), 0, m->stream, A, *cam, th, sig);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_fuse_batch(orbhip_matcher *m, int K, const orbhip_frame_view *const *kfs, const orbhip_camera *cam,
                      const float *Tcw, int sim3_form, int n, const float *world, const float *normal,
                      const float *max_dist, const float *min_dist, const uint8_t *flags, const uint8_t *point_desc,
                      float th, const float *inv_level_sigma2, int32_t *best_idx, int32_t *best_dist)
{
    if (!m || K < 0 || n < 0 || !cam || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS) return ORBHIP_E_ARG;
    if (K == 0 || n == 0) return ORBHIP_OK;
    if (!kfs || !Tcw || !world || !normal || !max_dist || !min_dist || !flags || !point_desc || !inv_level_sigma2 ||
        !best_idx || !best_dist)
        return ORBHIP_E_ARG;
    for (int k = 0; k < K; ++k)
        if (!kfs[k] || kfs[k]->n < 0 || (kfs[k]->n > 0 && (!kfs[k]->keys || !kfs[k]->desc))) return ORBHIP_E_ARG;
    for (size_t i = 0; i < (size_t)K * n; ++i) { best_idx[i] = -1; best_dist[i] = 256; }
    // A key frame goes with the batch when the one launch computes what orbhip_fuse would for it: at most 4096 key
    // points and the grid / level count of the shared camera.  Any other takes the single-frame path for its row.
    const GridInv inv = grid_inv(cam);
    std::vector<int> rows, single;
    int cap = 1;
    bool any_ur = false;
    for (int k = 0; k < K; ++k) {
        const orbhip_frame_view *f = kfs[k];
        if (f->n <= kGridMax && f->min_x == cam->min_x && f->min_y == cam->min_y && f->grid_inv_w == inv.w &&
            f->grid_inv_h == inv.h && f->n_levels == cam->n_levels) {
            rows.push_back(k);
            cap = std::max(cap, f->n);
            any_ur = any_ur || (f->u_right && f->n > 0);
        } else single.push_back(k);
    }
    const int Kb = (int)rows.size();
    if (Kb > 0) {
        ORBHIP_HIP_CHECK(hipSetDevice(m->device));
        const size_t kc = (size_t)Kb * cap, sn = (size_t)n;
        Stage st;
        int rc;
        const int *d_index, *d_n;
        const float *d_T, *d_ur, *d_world, *d_normal, *d_max, *d_min;
        const orbhip_keypoint *d_keys;
        const uint8_t *d_desc, *d_flags, *d_pdesc;
        if ((rc = stage_send(m, &st, [&](Stage &stg) {
                d_index = stg.room<int>((size_t)Kb); d_n = stg.room<int>((size_t)Kb);
                d_T = stg.room<float>((size_t)Kb * 12);
                d_keys = stg.room<orbhip_keypoint>(kc);
                d_desc = stg.room<uint8_t>(kc * 32);
                d_ur = any_ur ? stg.room<float>(kc) : nullptr;
                d_flags = stg.room<uint8_t>((size_t)Kb * sn);
                stg.sweep([&] {   // row b of these seven pieces: key frame rows[b]
                    for (int b = 0; b < Kb; ++b) {
                        const int k = rows[b];
                        const orbhip_frame_view *f = kfs[k];
                        const size_t fn = (size_t)f->n;
                        stg.host(d_index)[b] = b; stg.host(d_n)[b] = f->n;
                        memcpy(stg.host(d_T) + (size_t)b * 12, Tcw + (size_t)k * 12, 12 * sizeof(float));
                        if (fn) {
                            memcpy(stg.host(d_keys) + (size_t)b * cap, f->keys, fn * sizeof(orbhip_keypoint));
                            memcpy(stg.host(d_desc) + (size_t)b * cap * 32, f->desc, fn * 32);
                        }
                        if (any_ur)
                            for (size_t j = 0; j < fn; ++j) stg.host(d_ur)[(size_t)b * cap + j] = f->u_right ? f->u_right[j] : -1.0f;
                        memcpy(stg.host(d_flags) + (size_t)b * sn, flags + (size_t)k * sn, sn);
                    }
                });
                d_world = stg.put(world, sn * 3); d_normal = stg.put(normal, sn * 3);
                d_max = stg.put(max_dist, sn); d_min = stg.put(min_dist, sn);
                d_pdesc = stg.put(point_desc, sn * 32);
            }))) return rc;
        void *p;
        const size_t ob = (size_t)Kb * sn * sizeof(int);
        if ((rc = scratch(m, S_OUT, 2 * ob, &p))) return rc;
        int *d_out = (int *)p;
        if ((rc = orbhip_fuse_device(m, Kb, d_index, cam, d_T, sim3_form, d_keys, d_desc, d_n, cap, d_ur, nullptr, nullptr, n, n,
                                     d_world, d_normal, d_max, d_min, d_pdesc, d_flags, th, inv_level_sigma2, d_out,
                                     d_out + (size_t)Kb * sn, nullptr))) return rc;
        const uint8_t *h;
        if ((rc = read_back(m, d_out, 2 * ob, &h))) return rc;
        for (int b = 0; b < Kb; ++b) {
            memcpy(best_idx + (size_t)rows[b] * sn, h + (size_t)b * sn * sizeof(int), sn * sizeof(int));
            memcpy(best_dist + (size_t)rows[b] * sn, h + ob + (size_t)b * sn * sizeof(int), sn * sizeof(int));
        }
    }
    for (int k : single)
        if (int rc = orbhip_fuse(m, kfs[k], cam, Tcw + (size_t)k * 12, sim3_form, n, world, normal, max_dist, min_dist,
                                 flags + (size_t)k * n, point_desc, th, inv_level_sigma2, best_idx + (size_t)k * n,
                                 best_dist + (size_t)k * n)) return rc;
    return ORBHIP_OK;
}

// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452) up to :433, for K neighbours in one device-resident call
int orbhip_create_new_map_points_device(orbhip_matcher *m, int cur, int K, const void *d_kf_index, const orbhip_camera *cam,
                                        const void *d_Tcw, const void *d_kps, const void *d_desc, const void *d_n, int cap,
                                        const void *d_u_right, const void *d_depth, const void *d_node, const void *d_has_point,
                                        const void *d_median_depth, int only_stereo, int check_ori, const float *level_sigma2,
                                        void *d_matches12, void *d_nmatches, void *d_x3d, void *d_status, void *d_skipped,
                                        void *d_f12, void *d_epipole)
{
    if (!m || cur < 0 || K < 0 || cap < 1 || !cam || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS ||
        cam->fx == 0.f || cam->fy == 0.f)
        return ORBHIP_E_ARG;
    if (cap > kResolveMax) {
        set_error("create_new_map_points_device: capacity %d exceeds %d", cap, kResolveMax);
        return ORBHIP_E_CAPACITY;
    }
    if ((d_u_right == nullptr) != (d_depth == nullptr)) return ORBHIP_E_ARG;
    // monocular (no right coordinates) needs the scene median depths, stereo / RGB-D must not pass them (:249-261)
    if ((d_u_right == nullptr) != (d_median_depth != nullptr)) return ORBHIP_E_ARG;
    if (!d_Tcw || !d_kps || !d_desc || !d_n || !d_node || !level_sigma2) return ORBHIP_E_ARG;
    if (K == 0) return ORBHIP_OK;
    if (!d_kf_index || !d_matches12 || !d_nmatches || !d_x3d || !d_status || !d_skipped) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    void *p;
    if (int rc = scratch(m, S_TRI, (size_t)K * sizeof(CnmpRow), &p)) return rc;
    CnmpArgs A;
    A.kf_index = (const int *)d_kf_index; A.Tcw = (const float *)d_Tcw;
    A.keys = (const orbhip_keypoint *)d_kps; A.desc = (const uint8_t *)d_desc; A.n_dev = (const int *)d_n;
    A.u_right = (const float *)d_u_right; A.depth = (const float *)d_depth;
    A.node = (const uint32_t *)d_node; A.has_point = (const uint8_t *)d_has_point;
    A.median_depth = (const float *)d_median_depth;
    A.matches12 = (int *)d_matches12; A.nmatches = (int *)d_nmatches; A.x3d = (float *)d_x3d;
    A.status = (uint8_t *)d_status; A.skipped = (uint8_t *)d_skipped;
    A.f12_out = (float *)d_f12; A.ep_out = (float *)d_epipole;
    A.table = (CnmpRow *)p;
    A.cur = cur; A.K = K; A.cap = cap; A.only_stereo = only_stereo ? 1 : 0;
    CnmpLevels L;
    memset(&L, 0, sizeof(L));
    for (int l = 0; l < cam->n_levels; ++l) { L.sigma2[l] = level_sigma2[l]; L.sf[l] = cam->scale_factors[l]; }
    hipLaunchKernelGGL(k_cnmp_rows, dim3((K + 63) / 64), dim3(64), 0, m->stream, A, *cam);
    hipLaunchKernelGGL(k_cnmp_search, dim3((cap + 3) / 4, K), dim3(256), 0, m->stream, A, L);
    if (check_ori) hipLaunchKernelGGL(k_cnmp_cull, dim3(K), dim3(1024), 0, m->stream, A);
    hipLaunchKernelGGL(k_cnmp_triangulate, dim3((cap + 255) / 256, K), dim3(256), 0, m->stream, A, *cam, L);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int orbhip_create_new_map_points(orbhip_matcher *m, const orbhip_frame_view *cur, const uint32_t *node_cur,
                                 const uint8_t *has_point_cur, const float *depth_cur, const float *Tcw_cur, int K,
                                 const orbhip_frame_view *const *kfs, const uint32_t *const *node, const uint8_t *const *has_point,
                                 const float *const *depth, const float *Tcw, const float *median_depth,
                                 const orbhip_camera *cam, int only_stereo, int check_ori, const float *level_sigma2,
                                 int32_t *matches12, int32_t *nmatches, float *x3d, uint8_t *status, uint8_t *skipped,
                                 float *f12, float *epipole)
{
    if (!m || !cur || K < 0 || cur->n < 0 || !cam || cam->n_levels < 1 || cam->n_levels > ORBHIP_MAX_LEVELS ||
        cam->fx == 0.f || cam->fy == 0.f || !level_sigma2 || !Tcw_cur)
        return ORBHIP_E_ARG;
    const bool stereo = cur->u_right != nullptr;
    if (stereo != (depth_cur != nullptr) || stereo == (median_depth != nullptr)) return ORBHIP_E_ARG;
    if (cur->n > 0 && (!cur->keys || !cur->desc || !node_cur)) return ORBHIP_E_ARG;
    if (K > 0 && (!kfs || !node || !Tcw || (stereo && !depth))) return ORBHIP_E_ARG;
    for (int k = 0; k < K; ++k) {
        const orbhip_frame_view *f = kfs[k];
        if (!f || f->n < 0 || (f->n > 0 && (!f->keys || !f->desc || !node[k] || (f->u_right != nullptr) != stereo)) ||
            (stereo && f->n > 0 && !depth[k]))
            return ORBHIP_E_ARG;
    }
    int cap = std::max(cur->n, 1);
    for (int k = 0; k < K; ++k) cap = std::max(cap, kfs[k]->n);
    if (cap > kResolveMax) {
        set_error("create_new_map_points: %d keypoints exceed the LDS-resident limit %d", cap, kResolveMax);
        return ORBHIP_E_CAPACITY;
    }
    if (K == 0 || cur->n == 0) return ORBHIP_OK;
    if (!matches12 || !nmatches || !x3d || !status || !skipped) return ORBHIP_E_ARG;
    for (int k = -1; k < K; ++k) {
        const orbhip_frame_view *f = k < 0 ? cur : kfs[k];
        for (int j = 0; j < f->n; ++j)
            if (f->keys[j].octave < 0 || f->keys[j].octave >= cam->n_levels) {
                set_error("create_new_map_points: keypoint %d has octave %d outside [0,%d)", j, f->keys[j].octave,
                          cam->n_levels);
                return ORBHIP_E_ARG;
            }
    }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    // rows of the staged batch: 0 = the current key frame, 1 + k = neighbour k
    const int rows = K + 1;
    const size_t rc_ = (size_t)rows * cap, kc = (size_t)K * cap;
    const bool any_hp = has_point_cur || has_point;
    Stage st;
    int rc;
    const int *d_index, *d_n;
    const float *d_T, *d_ur = nullptr, *d_z = nullptr, *d_med = nullptr;
    const orbhip_keypoint *d_keys;
    const uint8_t *d_desc, *d_hp = nullptr;
    const uint32_t *d_node;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_index = stg.room<int>((size_t)K); d_n = stg.room<int>((size_t)rows);
            d_T = stg.room<float>((size_t)rows * 12);
            d_keys = stg.room<orbhip_keypoint>(rc_);
            d_desc = stg.room<uint8_t>(rc_ * 32);
            d_node = stg.room<uint32_t>(rc_);
            if (stereo) { d_ur = stg.room<float>(rc_); d_z = stg.room<float>(rc_); }
            if (any_hp) d_hp = stg.room<uint8_t>(rc_);
            if (median_depth) d_med = stg.put(median_depth, (size_t)K);
            stg.sweep([&] {   // row r of these pieces: the current key frame, then neighbour k = r - 1
                for (int r = 0; r < rows; ++r) {
                    const int k = r - 1;
                    const orbhip_frame_view *f = r == 0 ? cur : kfs[k];
                    const size_t fn = (size_t)f->n, o = (size_t)r * cap;
                    const uint8_t *hp = r == 0 ? has_point_cur : (has_point ? has_point[k] : nullptr);
                    if (r > 0) stg.host(d_index)[k] = r;
                    stg.host(d_n)[r] = f->n;
                    memcpy(stg.host(d_T) + (size_t)r * 12, r == 0 ? Tcw_cur : Tcw + (size_t)k * 12, 12 * sizeof(float));
                    if (!fn) continue;
                    memcpy(stg.host(d_keys) + o, f->keys, fn * sizeof(orbhip_keypoint));
                    memcpy(stg.host(d_desc) + o * 32, f->desc, fn * 32);
                    memcpy(stg.host(d_node) + o, r == 0 ? node_cur : node[k], fn * 4);
                    if (stereo) {
                        memcpy(stg.host(d_ur) + o, f->u_right, fn * 4);
                        memcpy(stg.host(d_z) + o, r == 0 ? depth_cur : depth[k], fn * 4);
                    }
                    if (any_hp) { if (hp) memcpy(stg.host(d_hp) + o, hp, fn); else memset(stg.host(d_hp) + o, 0, fn); }
                }
            });
        }))) return rc;
    // outputs in one block: matches12 | nmatches | x3d | f12 | epipole | status | skipped
    const size_t o_n = kc * 4, o_x = o_n + al256((size_t)K * 4), o_f = o_x + kc * 12, o_e = o_f + al256((size_t)K * 36),
                 o_s = o_e + al256((size_t)K * 8), o_k = o_s + al256(kc), total = o_k + al256((size_t)K);
    void *p;
    if ((rc = scratch(m, S_OUT, total, &p))) return rc;
    uint8_t *d_out = (uint8_t *)p;
    ORBHIP_HIP_CHECK(hipMemsetAsync(d_out, 0, total, m->stream));
    if ((rc = orbhip_create_new_map_points_device(m, 0, K, d_index, cam, d_T, d_keys, d_desc, d_n, cap, d_ur, d_z, d_node, d_hp,
                                                  d_med, only_stereo, check_ori, level_sigma2, d_out, d_out + o_n, d_out + o_x,
                                                  d_out + o_s, d_out + o_k, d_out + o_f, d_out + o_e))) return rc;
    const uint8_t *h;
    if ((rc = read_back(m, d_out, total, &h))) return rc;
    const size_t n1 = (size_t)cur->n;
    for (int k = 0; k < K; ++k) {
        memcpy(matches12 + (size_t)k * n1, h + (size_t)k * cap * 4, n1 * 4);
        memcpy(x3d + (size_t)k * n1 * 3, h + o_x + (size_t)k * cap * 12, n1 * 12);
        memcpy(status + (size_t)k * n1, h + o_s + (size_t)k * cap, n1);
    }
    memcpy(nmatches, h + o_n, (size_t)K * 4);
    memcpy(skipped, h + o_k, (size_t)K);
    if (f12) memcpy(f12, h + o_f, (size_t)K * 36);
    if (epipole) memcpy(epipole, h + o_e, (size_t)K * 8);
    return ORBHIP_OK;
}

int orbhip_search_by_sim3(orbhip_matcher *m, const orbhip_frame_view *kf1, const orbhip_frame_view *kf2,
                          const orbhip_camera *cam, const float *T1w, const float *T2w, const float *S21, const float *S12,
                          const float *world1, const float *max_dist1, const float *min_dist1, const uint8_t *flags1,
                          const uint8_t *desc1, const float *world2, const float *max_dist2, const float *min_dist2,
                          const uint8_t *flags2, const uint8_t *desc2, float th, int32_t *matches12, int *nfound)
{
    if (!m || !kf1 || !kf2 || !cam || !T1w || !T2w || !S21 || !S12 || !matches12 || !nfound) return ORBHIP_E_ARG;
    const int n1 = kf1->n, n2 = kf2->n;
    for (int i = 0; i < n1; ++i) matches12[i] = -1;
    *nfound = 0;
    if (n1 == 0 || n2 == 0) return ORBHIP_OK;
    static thread_local std::vector<orbhip_query> q1, q2;
    static thread_local std::vector<int32_t> m1, d1, m2, d2;
    q1.resize(n1); q2.resize(n2); m1.resize(n1); d1.resize(n1); m2.resize(n2); d2.resize(n2);
    int rc;
    // KF1's map points into KF2 (:1146-1226) and KF2's into KF1 (:1228-1303)
    if ((rc = orbhip_keyframe_queries(m, cam, 1, 1, T1w, S21, n1, world1, nullptr, max_dist1, min_dist1, flags1, th, q1.data()))) return rc;
    if ((rc = orbhip_keyframe_queries(m, cam, 1, 1, T2w, S12, n2, world2, nullptr, max_dist2, min_dist2, flags2, th, q2.data()))) return rc;
    if ((rc = orbhip_search_best_in_window(m, kf2, q1.data(), desc1, n1, 0, nullptr, m1.data(), d1.data()))) return rc;
    if ((rc = orbhip_search_best_in_window(m, kf1, q2.data(), desc2, n2, 0, nullptr, m2.data(), d2.data()))) return rc;
    int found = 0;
    for (int i1 = 0; i1 < n1; ++i1) {   // agreement, :1306-1323
        const int idx2 = (m1[i1] >= 0 && d1[i1] <= TH_HIGH) ? m1[i1] : -1;
        if (idx2 < 0) continue;
        const int idx1 = (m2[idx2] >= 0 && d2[idx2] <= TH_HIGH) ? m2[idx2] : -1;
        if (idx1 == i1) { matches12[i1] = idx2; ++found; }
    }
    *nfound = found;
    return ORBHIP_OK;
}

int orbhip_matcher_set_stream(orbhip_matcher *m, void *stream)
{
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
    m->stream = stream ? (hipStream_t)stream : m->own_stream;
    return ORBHIP_OK;
}

int orbhip_matcher_sync(orbhip_matcher *m)
{
    if (!m) return ORBHIP_E_ARG;
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    ORBHIP_HIP_CHECK(hipStreamSynchronize(m->stream));
    return ORBHIP_OK;
}

int orbhip_compute_stereo_matches(orbhip_matcher *m, orbhip_extractor *left, int frame_l, orbhip_extractor *right,
                                  int frame_r, const orbhip_keypoint *keys_l, const uint8_t *desc_l, int nl,
                                  const orbhip_keypoint *keys_r, const uint8_t *desc_r, int nr, float mbf, float mb,
                                  float *u_right, float *depth, int *nmatches)
{
    if (!m || !left || !right || !u_right || !depth || !nmatches || nl < 0 || nr < 0) return ORBHIP_E_ARG;
    if (!left->bound || !right->bound || frame_l < 0 || frame_l >= left->last_batch || frame_r < 0 ||
        frame_r >= right->last_batch || left->device != m->device || right->device != m->device ||
        left->nlevels != right->nlevels) {
        set_error("stereo: extractor handles do not hold matching pyramids on device %d", m->device);
        return ORBHIP_E_ARG;
    }
    for (int i = 0; i < nl; ++i) { u_right[i] = -1.0f; depth[i] = -1.0f; }
    *nmatches = 0;
    if (nl == 0 || nr == 0) return ORBHIP_OK;
    if (nr > (1 << 20)) { set_error("stereo: %d right keypoints exceed the 2^20 the match key holds", nr); return ORBHIP_E_CAPACITY; }
    ORBHIP_HIP_CHECK(hipSetDevice(m->device));
    if (int rc = ensure_level0(left, nullptr)) return rc;     // mvImagePyramid[0] of handles that produce it on demand
    if (int rc = ensure_level0(right, nullptr)) return rc;
    // (the frames of the levels >= 1 are not needed: orbhip_compute_stereo_matches_device)
    // the pyramids were produced on the extractors' streams
    ORBHIP_HIP_CHECK(hipStreamSynchronize(left->stream));
    ORBHIP_HIP_CHECK(hipStreamSynchronize(right->stream));
    Stage st;
    int rc;
    const orbhip_keypoint *d_kl, *d_kr;
    const uint8_t *d_dl, *d_dr;
    const int counts[2] = {nl, nr};
    const int *d_counts;
    if ((rc = stage_send(m, &st, [&](Stage &stg) {
            d_kl = stg.put(keys_l, (size_t)nl);
            d_dl = stg.put(desc_l, (size_t)nl * 32);
            d_kr = stg.put(keys_r, (size_t)nr);
            d_dr = stg.put(desc_r, (size_t)nr * 32);
            d_counts = stg.put(counts, 2);
        }))) return rc;
    // outputs contiguous: u_right[nl] | depth[nl] | n
    void *p;
    if ((rc = scratch(m, S_OUT, (size_t)(2 * nl + 1) * sizeof(float), &p))) return rc;
    float *d_ur = (float *)p, *d_depth = d_ur + nl;
    const StereoBatch B = {d_counts, d_counts + 1, 0, 0, 0, 0, std::max(nl, nr), 0, 0};
    if ((rc = launch_stereo(m, left, frame_l, right, frame_r, 1, B, d_kl, d_dl, d_kr, d_dr, mbf, mb, d_ur, d_depth,
                            (int *)(d_depth + nl))))
        return rc;
    const uint8_t *h;
    if ((rc = read_back(m, d_ur, (size_t)(2 * nl + 1) * sizeof(float), &h))) return rc;
    memcpy(u_right, h, (size_t)nl * sizeof(float));
    memcpy(depth, h + (size_t)nl * sizeof(float), (size_t)nl * sizeof(float));
    *nmatches = reinterpret_cast<const int *>(h)[2 * nl];
    return ORBHIP_OK;
}

}  // extern "C"
