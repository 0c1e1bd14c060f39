// Covisibility graph on the device: KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379) with AddConnection (:123-136) and
// UpdateBestCovisibles (:138-157), GetBestCovisibilityKeyFrames (:174-182), the target list of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:457-479) and the child lists, over tables (include/orbhip.h,
// orbhip_update_connections_device).  gfx950 only, wave64.  Integer work throughout: counters and the re-sort count are sums,
// the lists come from a sort of distinct keys, so nothing depends on the order in which atomics arrive.
//
// Launches of one orbhip_update_connections_device call, all on the caller's stream: one memset (the counters) and
//   k_cv_counters     16 lanes per slot of an updated row, histogram in LDS, flushed once; all U entries in one launch
//   k_cv_summary      per entry: voted rows, the first maximum, rows at or above the threshold
//   k_cv_apply        one launch per list entry, in list order: workgroup c leaves at once unless c is the updated row or
//                     qualifies; it reads and writes row c of the state only, so a launch has no cross-row hazards
#include "orbhip_internal.h"

#include <algorithm>

namespace orbhip {
namespace {

constexpr int kCvGroup = 16;        // lanes per slot in k_cv_counters
constexpr int kCvMaxRows = 4096;    // the dense state, the LDS histogram and the LDS sort
constexpr int kCvTh = 15;           // src/KeyFrame.cc:330
constexpr int kCvCovis = 10;        // the head orbhip_local_map_tables.covis holds

__device__ __forceinline__ int cv_slot(const int *row_slot, int c) { return row_slot ? row_slot[c] : c; }

// :302-320.  A group of 16 lanes owns one slot of the updated row; a workgroup keeps its counts in LDS.
__global__ __launch_bounds__(256) void k_cv_counters(CovisArgs A)
{
    __shared__ int s_hist[kCvMaxRows];
    const int u = blockIdx.y, tid = threadIdx.x, gl = tid & (kCvGroup - 1);
    const int r = A.update_rows[u];
    if ((unsigned)r >= (unsigned)A.rows) return;
    const int sr = cv_slot(A.row_slot, r);
    if (sr < 0) return;
    for (int j = tid; j < A.rows; j += 256) s_hist[j] = 0;
    __syncthreads();
    const int n = min(max(A.n[sr], 0), A.cap);
    const int *sp = A.slot_point + (size_t)sr * A.cap;
    for (int i = blockIdx.x * (256 / kCvGroup) + tid / kCvGroup; i < n; i += gridDim.x * (256 / kCvGroup)) {
        const int p = sp[i];
        if ((unsigned)p >= (unsigned)A.np || !(A.flags[p] & ORBHIP_POINT_PRESENT)) continue;      // :306-310
        const int o1 = A.obs_start[p + 1];
        for (int o = A.obs_start[p] + gl; o < o1; o += kCvGroup) {
            const int k = A.obs_kf[o];
            if (k != r && (unsigned)k < (unsigned)A.rows) atomicAdd(&s_hist[k], 1);                // :316-318
        }
    }
    __syncthreads();
    int *counter = A.counter + (size_t)u * A.rows;
    for (int j = tid; j < A.rows; j += 256) {
        const int v = s_hist[j];
        if (v) atomicAdd(counter + j, v);
    }
}

// :323-341 without the writes: how many rows were voted, the first strictly largest count in ascending row order, how many
// rows reach the threshold.
__global__ __launch_bounds__(256) void k_cv_summary(CovisArgs A)
{
    __shared__ int s_nv[4], s_nq[4], s_bv[4], s_br[4];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int *counter = A.counter + (size_t)u * A.rows;
    int nv = 0, nq = 0, bv = 0, br = -1;
    for (int j = tid; j < A.rows; j += 256) {
        const int v = counter[j];
        nv += v > 0;
        nq += v >= kCvTh;
        if (v > bv) { bv = v; br = j; }                                    // this thread's rows ascend: strictly larger only
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const int ov = __shfl_xor(bv, s), orow = __shfl_xor(br, s);
        if (orow >= 0 && (br < 0 || ov > bv || (ov == bv && orow < br))) { bv = ov; br = orow; }
    }
    nv = wave_sum(nv);
    nq = wave_sum(nq);
    if (lane == 0) { s_nv[wv] = nv; s_nq[wv] = nq; s_bv[wv] = bv; s_br[wv] = br; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < 4; ++w) {
        const int ov = s_bv[w], orow = s_br[w];
        if (orow >= 0 && (br < 0 || ov > bv || (ov == bv && orow < br))) { bv = ov; br = orow; }
    }
    int *S = A.summary + (size_t)u * 4;
    S[0] = s_nv[0] + s_nv[1] + s_nv[2] + s_nv[3];
    S[1] = br < 0 ? 0 : bv;
    S[2] = br;
    S[3] = s_nq[0] + s_nq[1] + s_nq[2] + s_nq[3];
    A.report[(size_t)u * 8 + 6] = 0;                                       // k_cv_apply counts the re-sorted rows into it
}

// Entry u of the list.  Workgroup c: AddConnection(r, counter[c]) on a qualifying row c (:123-136, :344, :351) with the
// re-sort of all its entries (:138-157, cv_resort_row), or the own row (:354-376).
__global__ __launch_bounds__(256) void k_cv_apply(CovisArgs A, int u)
{
    __shared__ unsigned long long s_key[kCvMaxRows];
    __shared__ int s_cnt[4];
    const int c = blockIdx.x, tid = threadIdx.x, rows = A.rows;
    const int r = A.update_rows[u];
    if ((unsigned)r >= (unsigned)rows) return;
    const int *S = A.summary + (size_t)u * 4;
    const int nvoted = S[0], bv = S[1], br = S[2];
    const bool fallback = S[3] == 0, own = c == r;
    const int *counter = A.counter + (size_t)u * rows;
    const int sc = cv_slot(A.row_slot, c);
    int *rep = A.report + (size_t)u * 8;
    if (nvoted == 0) {                                                     // :323: nothing is written
        if (own && tid == 0) {
            rep[0] = ORBHIP_CONNECTIONS_EMPTY; rep[1] = 0; rep[2] = sc < 0 ? 0 : A.n_ord[sc]; rep[3] = -1; rep[4] = 0; rep[5] = -1;
            rep[7] = 0;
        }
        return;
    }
    int w = 0;
    if (!own) {
        w = counter[c];
        if (!(fallback ? c == br : w >= kCvTh)) return;                    // :341, :348
    }
    if (sc < 0) return;
    int *cw = A.conn_w + (size_t)sc * rows;
    if (!own) {
        const int old = cw[r];
        __syncthreads();                                                   // every read of the old weight is before its write
        if (old == w) return;                                              // :131-132
    }
    int N = 2;
    while (N < rows) N <<= 1;
    int mine = 0;
    for (int i = tid; i < N; i += 256) {
        unsigned long long key = 0;
        if (i < rows) {
            int v;
            bool in;
            if (own) {
                v = counter[i];
                cw[i] = v;                                                 // :367: the whole counter, old entries dropped
                in = fallback ? i == br : v >= kCvTh;                      // :368-369: the qualifying rows only
            } else {
                v = i == r ? w : cw[i];
                if (i == r) cw[i] = w;                                     // :128-130
                in = v > 0;
            }
            if (in) { key = (unsigned long long)(unsigned)v << 32 | (unsigned)i; ++mine; }
        }
        s_key[i] = key;
    }
    const int n_out = cv_resort_row(s_key, s_cnt, mine, N, A.ord_kf + (size_t)sc * rows, A.ord_w + (size_t)sc * rows,
                                    A.covis + (size_t)sc * kCvCovis, A.n_ord + sc);
    if (tid != 0) return;
    if (!own) { atomicAdd(rep + 6, 1); return; }
    int parent_set = -1;
    if (A.first_conn[sc] && r != A.id0_row) {                              // :371-376
        parent_set = (int)(unsigned)s_key[0];
        A.parent[sc] = parent_set;
        A.first_conn[sc] = 0;
    }
    rep[0] = ORBHIP_CONNECTIONS_OK; rep[1] = nvoted; rep[2] = n_out; rep[3] = br; rep[4] = bv; rep[5] = parent_set;
    rep[7] = fallback ? 1 : 0;
}

// GetBestCovisibilityKeyFrames(nn) (nn2 == 0) or vpTargetKFs of SearchInNeighbors (src/LocalMapping.cc:457-479).  One
// wavefront per query; the walk over the first neighbours is serial, with mnFuseTargetForKF == mnId as a bitset in LDS.
__global__ __launch_bounds__(64) void k_cv_targets(CovisTargetArgs A)
{
    __shared__ uint32_t s_stamp[kCvMaxRows / 32];
    const int q = blockIdx.x, lane = threadIdx.x, rows = A.rows;
    const int out_cap = A.nn * (1 + A.nn2);
    int *out = A.targets + (size_t)q * out_cap;
    const int cur = A.cur[q];
    for (int w = lane; w < kCvMaxRows / 32; w += 64) s_stamp[w] = 0;
    wave_lds_handoff();
    int size = 0;
    const int sc = (unsigned)cur < (unsigned)rows ? cv_slot(A.row_slot, cur) : -1;
    if (sc >= 0) {
        const int n1 = min(min(max(A.n_ord[sc], 0), rows), A.nn);          // src/KeyFrame.cc:177-180
        const int *first = A.ord_kf + (size_t)sc * A.stride;
        if (A.nn2 == 0) {
            for (int i = lane; i < n1; i += 64) out[i] = first[i];
            size = n1;
        } else {
#define CV_BAD(x) (A.kf_bad && A.kf_bad[(x)])
#define CV_STAMPED(x) ((s_stamp[(x) >> 5] >> ((x) & 31)) & 1u)
            for (int v = 0; v < n1; ++v) {
                const int a = first[v];
                if ((unsigned)a >= (unsigned)rows || CV_BAD(a) || CV_STAMPED(a)) continue;        // :465
                if (lane == 0) { out[size] = a; s_stamp[a >> 5] |= 1u << (a & 31); }               // :467-468
                ++size;
                wave_lds_handoff();
                const int sa = cv_slot(A.row_slot, a);
                if (sa < 0) continue;
                const int n2 = min(min(max(A.n_ord[sa], 0), rows), A.nn2);                         // :471
                const int *second = A.ord_kf + (size_t)sa * A.stride;
                for (int b = 0; b < n2; b += 64) {                         // second neighbours are not stamped: no hand-off
                    const int k2 = b + lane < n2 ? second[b + lane] : -1;
                    const bool ok = (unsigned)k2 < (unsigned)rows && !CV_BAD(k2) && !CV_STAMPED(k2) && k2 != cur;      // :475
                    const unsigned long long mk = __ballot(ok);
                    if (ok) out[size + lane_prefix(mk)] = k2;
                    size += __popcll(mk);
                }
            }
#undef CV_BAD
#undef CV_STAMPED
        }
    }
    for (int i = size + lane; i < out_cap; i += 64) out[i] = -1;
    if (lane == 0) A.counts[q] = size;
}

// mspChildrens of every row as CSR, ascending row inside a list: count, scan, ordered emit, one workgroup, all in LDS.
__global__ __launch_bounds__(256) void k_cv_children(int rows, const int *__restrict__ parent, const uint8_t *__restrict__ kf_bad,
                                                     int *__restrict__ child_start, int *__restrict__ child)
{
    __shared__ int s_cur[kCvMaxRows];      // the count of a row, then the next free entry of its list
    __shared__ int s_par[256], s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < rows; i += 256) s_cur[i] = 0;
    __syncthreads();
    for (int c = tid; c < rows; c += 256) {
        const int p = parent[c];
        if ((unsigned)p < (unsigned)rows && !(kf_bad && kf_bad[c])) atomicAdd(&s_cur[p], 1);
    }
    __syncthreads();
    int running = 0;
    for (int b = 0; b < rows; b += 256) {
        const int i = b + tid;
        const int v = i < rows ? s_cur[i] : 0;
        const int incl = wave_incl_scan_add(v);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_w[w];
        if (i < rows) { child_start[i] = off + incl - v; s_cur[i] = off + incl - v; }
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) child_start[rows] = running;
    for (int b = 0; b < rows; b += 256) {
        const int c = b + tid;
        int p = -1;
        if (c < rows) {
            p = parent[c];
            if ((unsigned)p >= (unsigned)rows || (kf_bad && kf_bad[c])) p = -1;
        }
        s_par[tid] = p;
        __syncthreads();
        if (p >= 0) {
            int rank = 0;
            for (int j = 0; j < tid; ++j) rank += s_par[j] == p;
            child[s_cur[p] + rank] = c;
        }
        __syncthreads();
        if (p >= 0) atomicAdd(&s_cur[p], 1);
        __syncthreads();
    }
}

}  // namespace

size_t covis_workspace_bytes(int U, int rows) { return al256((size_t)U * rows * sizeof(int)) + al256((size_t)U * 4 * sizeof(int)); }

int launch_update_connections(hipStream_t stream, CovisArgs A, void *workspace)
{
    const size_t cbytes = (size_t)A.U * A.rows * sizeof(int);
    A.counter = (int *)workspace;
    A.summary = (int *)((uint8_t *)workspace + al256(cbytes));
    ORBHIP_HIP_CHECK(hipMemsetAsync(A.counter, 0, cbytes, stream));
    const int slot_blocks = std::max(1, std::min(8, (A.cap + 127) / 128));
    hipLaunchKernelGGL(k_cv_counters, dim3(slot_blocks, A.U), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_cv_summary, dim3(A.U), dim3(256), 0, stream, A);
    for (int u = 0; u < A.U; ++u) hipLaunchKernelGGL(k_cv_apply, dim3(A.rows), dim3(256), 0, stream, A, u);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int launch_covisible_targets(hipStream_t stream, CovisTargetArgs A, int Q)
{
    hipLaunchKernelGGL(k_cv_targets, dim3(Q), dim3(64), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int launch_children_from_parents(hipStream_t stream, int rows, const int *parent, const uint8_t *kf_bad, int *child_start, int *child)
{
    hipLaunchKernelGGL(k_cv_children, dim3(1), dim3(256), 0, stream, rows, parent, kf_bad, child_start, child);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
