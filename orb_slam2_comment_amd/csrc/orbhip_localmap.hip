// Local map on the device: Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1231-1339), UpdateLocalPoints (:1205-1228) and
// the bookkeeping in front of SearchLocalPoints' search (:1146-1180) over tables (include/orbhip.h,
// orbhip_update_local_map_device).  gfx950 only, wave64.  Integer and bitwise work throughout: votes are sums, the owner
// of a point is a minimum, so nothing depends on the order in which atomics arrive.
//
// Launches of one orbhip_update_local_map_device call, all on the caller's stream: two memsets (d_votes to 0; the
// `first` keys and the "frame does not hold it" bytes of the workspace to 0xff) and six kernels:
//   k_lm_votes        16 lanes per frame slot: nulls bad frame points, adds the votes, marks the points the frame holds, taken
//   k_lm_keyframes    one workgroup per frame: first pass (ordered compaction, first maximum), then the walk in one wavefront
//   k_lm_first        key = list position * cap + slot, atomicMin into first[p]
//   k_lm_points<0>    winners per list position
//   k_lm_scan         exclusive scan of those counts, d_np_l
//   k_lm_points<1>    the same winners, written in order together with the gathered arrays
// orbhip_track_local_map_device adds the existing frustum and search launches and k_lm_apply.
#include "orbhip_internal.h"

#include <algorithm>

namespace orbhip {
namespace {

constexpr int kLmGroup = 16;        // lanes per frame slot in k_lm_votes
constexpr int kLmMaxKf = 80;        // mvpLocalKeyFrames.size() > 80 ends the walk (:1285)
constexpr int kLmCovis = 10;        // GetBestCovisibilityKeyFrames(10)
constexpr int kLmPosBlocks = 1024;  // grid.x of the kernels that loop over list positions
constexpr int kLmStampWords = 65536 / 32;

__device__ __forceinline__ int lm_list_len(const LocalMapArgs &A, int f) { return min(max(A.n_local_kf[f], 0), A.rows); }

// :1235-1251 and :1146-1162.  A group of 16 lanes owns one slot of the current frame.
__global__ __launch_bounds__(256) void k_lm_votes(LocalMapArgs A)
{
    const int f = blockIdx.y, gl = threadIdx.x & (kLmGroup - 1);
    const int i = blockIdx.x * (256 / kLmGroup) + (threadIdx.x / kLmGroup);
    const int nf = min(max(A.frame_n[f], 0), A.cap);
    if (i >= nf) return;
    int *fp = A.frame_point + (size_t)f * A.cap + i;
    const int p = *fp;
    uint8_t tk = 0;
    if (p >= 0) {
        const uint8_t fl = A.flags[p];
        if (fl & ORBHIP_POINT_PRESENT) {
            int *votes = A.votes + (size_t)f * A.rows;
            const int o1 = A.obs_start[p + 1];
            for (int o = A.obs_start[p] + gl; o < o1; o += kLmGroup) atomicAdd(votes + A.obs_kf[o], 1);
            if (gl == 0) A.free_pt[(size_t)f * A.pcap + p] = 0;          // mnLastFrameSeen = mnId (:1158)
            tk = (fl & ORBHIP_POINT_OBSERVED) ? 1 : 0;
        } else if (gl == 0) *fp = -1;                                     // :1248, :1153
    }
    if (gl == 0) A.taken[(size_t)f * A.cap + i] = tk;                     // src/ORBmatcher.cc:84-86
}

// :1253-1338.  One workgroup per frame.  The first pass walks the rows 256 at a time, ascending, and appends the voted rows
// that are not bad in that order; the walk over its entries is serial and runs in wavefront 0 with the stamps
// (mnTrackReferenceForFrame == mnId) as a bitset in LDS.
__global__ __launch_bounds__(256) void k_lm_keyframes(LocalMapArgs A)
{
    __shared__ uint32_t s_stamp[kLmStampWords];
    __shared__ int s_head[kLmMaxKf];       // the entries the walk can visit: a visit needs size() <= 80
    __shared__ int s_wcnt[4], s_wvoted[4], s_bv[4], s_br[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int rows = A.rows;
    const int *votes = A.votes + (size_t)f * rows;
    int *list = A.local_kf + (size_t)f * rows;
    for (int w = tid; w < kLmStampWords; w += 256) s_stamp[w] = 0;
    __syncthreads();
    int running = 0, nvoted = 0, bv = 0, br = -1;
    for (int base = 0; base < rows; base += 256) {
        const int r = base + tid;
        const int v = r < rows ? votes[r] : 0;
        const bool voted = v > 0;
        const bool good = voted && !(A.kf_bad && A.kf_bad[r]);            // :1267
        const unsigned long long mg = __ballot(good);
        nvoted += voted ? 1 : 0;
        if (lane == 0) s_wcnt[wv] = __popcll(mg);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_wcnt[w];
        const int total = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        if (good) {
            const int pos = off + lane_prefix(mg);
            list[pos] = r;                                                 // :1276
            if (pos < kLmMaxKf) s_head[pos] = r;
            atomicOr(&s_stamp[r >> 5], 1u << (r & 31));                    // :1277
            if (v > bv) { bv = v; br = r; }                                // this thread's rows ascend: strictly larger only
        }
        running += total;
        __syncthreads();
    }
    // first maximum: the larger count, the lower row among equal counts (:1270 is a strict comparison in ascending order)
    for (int s = 32; s >= 1; s >>= 1) {
        const int ov = __shfl_xor(bv, s), orow = __shfl_xor(br, s);
        if (orow >= 0 && (br < 0 || ov > bv || (ov == bv && orow < br))) { bv = ov; br = orow; }
    }
    nvoted = wave_sum(nvoted);
    if (lane == 0) { s_bv[wv] = bv; s_br[wv] = br; s_wvoted[wv] = nvoted; }
    __syncthreads();
    if (wv != 0) return;
    bv = s_bv[0]; br = s_br[0];
    for (int w = 1; w < 4; ++w) {
        const int ov = s_bv[w], orow = s_br[w];
        if (orow >= 0 && (br < 0 || ov > bv || (ov == bv && orow < br))) { bv = ov; br = orow; }
    }
    nvoted = s_wvoted[0] + s_wvoted[1] + s_wvoted[2] + s_wvoted[3];

    const int n_first = running;           // itEndKF, taken before the loop
    int size = running, walk_end = 0;
#define LM_BAD(x) (A.kf_bad && A.kf_bad[(x)])
#define LM_STAMPED(x) ((s_stamp[(x) >> 5] >> ((x) & 31)) & 1u)
#define LM_APPEND(x)                                                         \
    do {                                                                     \
        if (lane == 0) { list[size] = (x); s_stamp[(x) >> 5] |= 1u << ((x) & 31); } \
        ++size;                                                              \
        wave_lds_handoff();                                                  \
    } while (0)
    for (int v = 0; v < n_first; ++v) {
        if (size > kLmMaxKf) { walk_end = 1; break; }                      // :1285
        const int r = s_head[v];
        {   // a. the first of the ten best covisibles that is neither bad nor stamped (:1292-1304)
            int c = -1;
            if (lane < kLmCovis) c = A.covis[(size_t)r * kLmCovis + lane];
            const bool ok = c >= 0 && !LM_BAD(c) && !LM_STAMPED(c);
            const unsigned long long mk = __ballot(ok);
            if (mk) { const int cc = __shfl(c, __ffsll((long long)mk) - 1); LM_APPEND(cc); }
        }
        {   // b. the first such child (:1306-1319), 64 at a time
            const int c1 = A.child_start[r + 1];
            for (int b = A.child_start[r]; b < c1; b += 64) {
                int c = -1;
                if (b + lane < c1) c = A.child[b + lane];
                const bool ok = c >= 0 && !LM_BAD(c) && !LM_STAMPED(c);
                const unsigned long long mk = __ballot(ok);
                if (mk) { const int cc = __shfl(c, __ffsll((long long)mk) - 1); LM_APPEND(cc); break; }
            }
        }
        // c. the parent, not tested for isBad; its break leaves the walk (:1321-1330)
        const int pr = A.parent[r];
        if (pr >= 0 && !LM_STAMPED(pr)) { LM_APPEND(pr); walk_end = 2; break; }
    }
#undef LM_BAD
#undef LM_STAMPED
#undef LM_APPEND
    if (lane == 0) {
        int *rep = A.report + (size_t)f * 8;
        const int status = nvoted == 0 ? ORBHIP_LOCALMAP_NO_VOTES : (br < 0 ? ORBHIP_LOCALMAP_ALL_BAD : ORBHIP_LOCALMAP_OK);
        int nl = size;
        if (nvoted == 0) nl = A.n_local_kf[f];                             // :1253: the list stays
        else A.n_local_kf[f] = size;
        rep[0] = status; rep[1] = nvoted; rep[2] = nl; rep[3] = br; rep[4] = br < 0 ? 0 : bv; rep[5] = walk_end;
        rep[7] = 0;
    }
}

// The owner of a point is the first (list position, slot) that holds it (:1219): the smallest key.
__global__ __launch_bounds__(256) void k_lm_first(LocalMapArgs A)
{
    const int f = blockIdx.y, nl = lm_list_len(A, f);
    uint32_t *first = A.first + (size_t)f * A.pcap;
    for (int pos = blockIdx.x; pos < nl; pos += gridDim.x) {
        const int row = A.local_kf[(size_t)f * A.rows + pos];
        const int n = min(max(A.n[row], 0), A.cap);
        const int *sp = A.slot_point + (size_t)row * A.cap;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int p = sp[i];
            if (p >= 0 && (A.flags[p] & ORBHIP_POINT_PRESENT)) atomicMin(first + p, (uint32_t)(pos * A.cap + i));
        }
    }
}

// EMIT false: base[pos] = the number of points list position pos owns.  EMIT true: base[pos] is the exclusive scan of
// those counts, and the owners are written in slot order behind it together with the gathered arrays.
template <bool EMIT> __global__ __launch_bounds__(256) void k_lm_points(LocalMapArgs A)
{
    __shared__ int s_w[4];
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nl = lm_list_len(A, f);
    const uint32_t *first = A.first + (size_t)f * A.pcap;
    for (int pos = blockIdx.x; pos < nl; pos += gridDim.x) {
        const int row = A.local_kf[(size_t)f * A.rows + pos];
        const int n = min(max(A.n[row], 0), A.cap);
        const int *sp = A.slot_point + (size_t)row * A.cap;
        int run = EMIT ? A.base[(size_t)f * A.rows + pos] : 0;
        for (int b = 0; b < n; b += 256) {     // n is the same for the whole workgroup
            const int i = b + tid;
            int p = -1;
            bool win = false;
            uint8_t fl = 0;
            if (i < n) {
                p = sp[i];
                if (p >= 0) {
                    fl = A.flags[p];
                    win = (fl & ORBHIP_POINT_PRESENT) && first[p] == (uint32_t)(pos * A.cap + i);
                }
            }
            const unsigned long long mk = __ballot(win);
            if (lane == 0) s_w[wv] = __popcll(mk);
            __syncthreads();
            int off = run;
            for (int w = 0; w < wv; ++w) off += s_w[w];
            run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
            if (EMIT && win) {
                const size_t e = (size_t)f * A.pcap + (size_t)(off + lane_prefix(mk));
                A.local_point[e] = p;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    A.world_l[e * 3 + c] = A.world[(size_t)p * 3 + c];
                    A.normal_l[e * 3 + c] = A.normal[(size_t)p * 3 + c];
                }
                A.max_dist_l[e] = A.max_dist[p];
                A.min_dist_l[e] = A.min_dist[p];
                const uint4 *src = reinterpret_cast<const uint4 *>(A.point_desc + (size_t)p * 32);
                uint4 *dst = reinterpret_cast<uint4 *>(A.desc_l + e * 32);
                dst[0] = src[0];
                dst[1] = src[1];
                // a point the frame holds is not projected (:1170); the others carry Observations() > 0 for the search
                A.flags_l[e] = A.free_pt[(size_t)f * A.pcap + p] ? (uint8_t)(ORBHIP_POINT_PRESENT | (fl & ORBHIP_POINT_OBSERVED)) : (uint8_t)0;
            }
            __syncthreads();
        }
        if (!EMIT && tid == 0) A.base[(size_t)f * A.rows + pos] = run;
    }
}

__global__ __launch_bounds__(256) void k_lm_scan(LocalMapArgs A)
{
    __shared__ int s_w[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nl = lm_list_len(A, f);
    int *base = A.base + (size_t)f * A.rows;
    int running = 0;
    for (int b = 0; b < nl; b += 256) {
        const int i = b + tid;
        const int v = i < nl ? base[i] : 0;
        const int incl = wave_incl_scan_add(v);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_w[w];
        if (i < nl) base[i] = off + incl - v;
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) { A.np_l[f] = running; A.report[(size_t)f * 8 + 6] = running; }
}

// after the points search: nToMatch (:1164-1180) and F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:122)
__global__ __launch_bounds__(256) void k_lm_apply(int cap, int pcap, const orbhip_query *__restrict__ q, const int *__restrict__ np_l,
                                                  const int *__restrict__ frame_n, const int *__restrict__ assign,
                                                  const int *__restrict__ local_point, int *__restrict__ frame_point,
                                                  int *__restrict__ report)
{
    __shared__ int s_cnt;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int np = min(max(np_l[f], 0), pcap), nf = min(max(frame_n[f], 0), cap);
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int c = 0;
    for (int i = tid; i < np; i += 256) c += q[(size_t)f * pcap + i].valid != 0;
    c = wave_sum(c);
    if ((tid & 63) == 0 && c) atomicAdd(&s_cnt, c);
    for (int i = tid; i < nf; i += 256) {
        const int a = assign[(size_t)f * cap + i];
        if (a >= 0 && a < np) frame_point[(size_t)f * cap + i] = local_point[(size_t)f * pcap + a];
    }
    __syncthreads();
    if (tid == 0) report[(size_t)f * 8 + 7] = s_cnt;
}

}  // namespace

size_t local_map_workspace_bytes(int frames, int rows, int pcap)
{
    return al256((size_t)frames * pcap * 5) + al256((size_t)frames * rows * sizeof(int));
}

int launch_local_map(hipStream_t stream, LocalMapArgs A, void *workspace)
{
    const size_t fp = (size_t)A.frames * A.pcap;
    A.first = (uint32_t *)workspace;
    A.free_pt = (uint8_t *)workspace + fp * 4;
    A.base = (int *)((uint8_t *)workspace + al256(fp * 5));
    if (A.rows > 0) ORBHIP_HIP_CHECK(hipMemsetAsync(A.votes, 0, (size_t)A.frames * A.rows * sizeof(int), stream));
    if (fp > 0) ORBHIP_HIP_CHECK(hipMemsetAsync(workspace, 0xff, fp * 5, stream));
    const int pos_blocks = std::max(1, std::min(A.rows, kLmPosBlocks));
    hipLaunchKernelGGL(k_lm_votes, dim3((A.cap + 256 / kLmGroup - 1) / (256 / kLmGroup), A.frames), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_lm_keyframes, dim3(A.frames), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_lm_first, dim3(pos_blocks, A.frames), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_lm_points<false>, dim3(pos_blocks, A.frames), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_lm_scan, dim3(A.frames), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_lm_points<true>, dim3(pos_blocks, A.frames), dim3(256), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int launch_local_map_apply(hipStream_t stream, int frames, int cap, int pcap, const void *q, const int *np_l, const int *frame_n,
                           const int *assign, const int *local_point, int *frame_point, int *report)
{
    hipLaunchKernelGGL(k_lm_apply, dim3(frames), dim3(256), 0, stream, cap, pcap, (const orbhip_query *)q, np_l, frame_n, assign,
                       local_point, frame_point, report);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
