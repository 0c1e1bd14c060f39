// Culling on the device: LocalMapping::MapPointCulling (src/LocalMapping.cc:170-205) and KeyFrameCulling (:632-696) with
// MapPoint::SetBadFlag (src/MapPoint.cc:151-168), MapPoint::EraseObservation (:111-137), KeyFrame::SetBadFlag
// (src/KeyFrame.cc:453-545) and KeyFrame::EraseConnection (:553-567), over tables (include/orbhip.h,
// orbhip_cull_key_frames_device).  gfx950 only, wave64.  Integer work throughout: the report counts are sums, an observation
// is erased by whoever claims its alive mark and the result is the same whoever that is, two stores to one slot store the
// same -1, so nothing depends on the order in which atomics arrive.
//
// mObservations of a point is its list in the observation table with a mark per entry (alive); Observations() is a count
// derived at the start of a call.  Launches, all on the caller's stream:
//   k_cull_init        16 lanes per point: marks, counts, the reference observation; the call's copy of the candidate list
//   map points         k_mp_own (first list position of each point), k_mp_decide (one workgroup: the branch of every entry,
//                      ordered emit of the kept ones), k_mp_act (16 lanes per culled entry: SetBadFlag)
//   key frames         per candidate, in list order: k_kf_apply (workgroup c < rows: EraseConnection on row c; the workgroups
//                      behind them: EraseObservation over r's slots; all of them leave at once unless the verdict is
//                      "culled") and k_kf_step (one wavefront: the spanning tree of this candidate; one workgroup: the verdict
//                      of the next one), with one k_kf_step in front for the first verdict
//   close-out          k_cull_count, k_cull_scan, k_cull_scatter: the table without the erased entries; for key frames then
//                      k_cv_children
// 7 launches for the map points, 2 U + 6 for U candidates (5 for none).
#include "orbhip_internal.h"

#include <algorithm>
#include <climits>

namespace orbhip {
namespace {

constexpr int kCuGroup = 16;        // lanes per point / per entry
constexpr int kCuMaxRows = 4096;    // the dense covisibility state and the LDS sort
constexpr int kCuCovis = 10;

__device__ __forceinline__ int group_sum(int v)
{
    for (int s = kCuGroup / 2; s >= 1; s >>= 1) v += __shfl_xor(v, s, kCuGroup);
    return v;
}

// the list of point p, clipped to the table
__device__ __forceinline__ void cu_list(const CullArgs &A, int p, int &o0, int &o1)
{
    o0 = min(max(A.obs_start[p], 0), A.obs_cap);
    o1 = min(max(A.obs_start[p + 1], o0), A.obs_cap);
}
__device__ __forceinline__ bool cu_obs_ok(const CullArgs &A, int kf, int idx)
{
    return (unsigned)kf < (unsigned)A.rows && (unsigned)idx < (unsigned)A.cap;
}

// Observations() as AddObservation leaves it (src/MapPoint.cc:98-109): 2 for an entry with a right coordinate, else 1.  A
// point that is bad when the call starts has no observations (SetBadFlag cleared them, :159).
__global__ __launch_bounds__(256) void k_cull_init(CullArgs A)
{
    const int g = (blockIdx.x * 256 + threadIdx.x) / kCuGroup, gl = threadIdx.x & (kCuGroup - 1);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < A.U) A.cand[t] = A.cand_in[t];
    if (g >= A.np) return;
    const int p = g;
    int o0, o1;
    cu_list(A, p, o0, o1);
    const bool present = A.flags[p] & ORBHIP_POINT_PRESENT;
    int sum = 0;
    for (int o = o0 + gl; o < o1; o += kCuGroup) {
        A.alive[o] = present ? 1 : 0;
        const int kf = A.obs_kf[o], idx = A.obs_idx[o];
        sum += A.u_right && cu_obs_ok(A, kf, idx) && A.u_right[(size_t)kf * A.cap + idx] >= 0.f ? 2 : 1;
    }
    sum = group_sum(sum);
    if (gl != 0) return;
    const int ref = A.ref_obs[p];
    A.nobs[p] = present ? sum : 0;
    A.ref_cur[p] = present && (unsigned)ref < (unsigned)(o1 - o0) ? ref : -1;
    A.owner[p] = INT_MAX;
}

// MapPoint::SetBadFlag (src/MapPoint.cc:151-168) by a group of 16 lanes: every observation dies and EraseMapPointMatch
// (by index, whatever the slot holds) clears its slot.
__device__ __forceinline__ void cu_set_bad_group(const CullArgs &A, int p, int gl)
{
    int o0, o1;
    cu_list(A, p, o0, o1);
    for (int o = o0 + gl; o < o1; o += kCuGroup) {
        if (!A.alive[o]) continue;
        A.alive[o] = 0;
        const int kf = A.obs_kf[o], idx = A.obs_idx[o];
        if (cu_obs_ok(A, kf, idx)) A.slot_point[(size_t)kf * A.cap + idx] = -1;
    }
    if (gl == 0) A.flags[p] &= (uint8_t)~ORBHIP_POINT_PRESENT;
}

// a point listed twice belongs to its first entry
__global__ __launch_bounds__(256) void k_mp_own(CullArgs A)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.R) return;
    const int p = A.recent[e];
    if ((unsigned)p < (unsigned)A.np) atomicMin(&A.owner[p], e);
}

// src/LocalMapping.cc:183-204 for every entry, then the ordered emit of the kept ones: one workgroup, 256 entries a round.
// Nothing an entry reads is written by another entry's SetBadFlag, which k_mp_act does afterwards.
__global__ __launch_bounds__(256) void k_mp_decide(CullArgs A)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int running = 0;
    for (int b = 0; b < A.R; b += 256) {
        const int e = b + tid;
        int st = ORBHIP_CULLPOINT_ALREADY_BAD, p = -1;
        if (e < A.R) {
            p = A.recent[e];
            if ((unsigned)p < (unsigned)A.np && (A.flags[p] & ORBHIP_POINT_PRESENT)) {                 // :186
                const int age = A.cur_kf_id - A.first_kf_id[p];
                if (4ll * A.found[p] < (long long)A.visible[p]) st = ORBHIP_CULLPOINT_BAD_RATIO;        // :190
                else if (age >= 2 && A.nobs[p] <= A.th_obs) st = ORBHIP_CULLPOINT_BAD_OBS;              // :195
                else if (age >= 3) st = ORBHIP_CULLPOINT_DROPPED_OLD;                                   // :200
                else st = ORBHIP_CULLPOINT_KEPT;
                if (A.owner[p] != e && (st == ORBHIP_CULLPOINT_BAD_RATIO || st == ORBHIP_CULLPOINT_BAD_OBS))
                    st = ORBHIP_CULLPOINT_ALREADY_BAD;                     // the first entry culled it
            }
            A.status[e] = (uint8_t)st;
        }
        const int keep = e < A.R && st == ORBHIP_CULLPOINT_KEPT;
        const int incl = wave_incl_scan_add(keep);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_w[w];
        if (keep) A.recent_out[off + incl - 1] = p;
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) A.n_recent_out[0] = running;
}

__global__ __launch_bounds__(256) void k_mp_act(CullArgs A)
{
    const int e = (blockIdx.x * 256 + threadIdx.x) / kCuGroup, gl = threadIdx.x & (kCuGroup - 1);
    if (e >= A.R) return;
    const int st = A.status[e];
    if (st != ORBHIP_CULLPOINT_BAD_RATIO && st != ORBHIP_CULLPOINT_BAD_OBS) return;
    cu_set_bad_group(A, A.recent[e], gl);
}

// src/LocalMapping.cc:643-694 for candidate u against the state as the candidates before it left it: one workgroup.
__device__ __forceinline__ void kf_decide(const CullArgs &A, int u)
{
    __shared__ int s_mp[4], s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int *rep = A.report + (size_t)u * 8;
    const int r = A.cand[u];
    if ((unsigned)r >= (unsigned)A.rows || r == A.id0_row) {                // :643
        if (tid < 8) rep[tid] = tid ? 0 : ((unsigned)r >= (unsigned)A.rows ? ORBHIP_CULLKF_SKIPPED_ENTRY : ORBHIP_CULLKF_SKIPPED_ID0);
        if (tid == 0) A.verdict[u] = rep[0];
        return;
    }
    const int n = min(max(A.n[r], 0), A.cap);
    const int *sp = A.slot_point + (size_t)r * A.cap;
    int n_mp = 0, n_red = 0;
    for (int i = tid; i < n; i += 256) {
        const int p = sp[i];
        if ((unsigned)p >= (unsigned)A.np || !(A.flags[p] & ORBHIP_POINT_PRESENT)) continue;           // :654-656
        if (!A.mono) {
            const float d = A.depth[(size_t)r * A.cap + i];
            if (d > A.th_depth || d < 0.f) continue;                       // :660
        }
        ++n_mp;
        if (A.nobs[p] <= 3) continue;                                      // :665
        const int level = A.kps[(size_t)r * A.cap + i].octave;
        int o0, o1, cnt = 0;
        cu_list(A, p, o0, o1);
        for (int o = o0; o < o1 && cnt < 3; ++o) {                          // :670-683
            if (!A.alive[o]) continue;
            const int kf = A.obs_kf[o], idx = A.obs_idx[o];
            if (kf == r || !cu_obs_ok(A, kf, idx)) continue;
            if (A.kps[(size_t)kf * A.cap + idx].octave <= level + 1) ++cnt;
        }
        n_red += cnt >= 3;
    }
    n_mp = wave_sum(n_mp);
    n_red = wave_sum(n_red);
    if (lane == 0) { s_mp[wv] = n_mp; s_red[wv] = n_red; }
    __syncthreads();
    if (tid != 0) return;
    n_mp = s_mp[0] + s_mp[1] + s_mp[2] + s_mp[3];
    n_red = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    int st = 10 * n_red > 9 * n_mp ? ORBHIP_CULLKF_CULLED : ORBHIP_CULLKF_NOT_CULLED;                   // :693
    if (st == ORBHIP_CULLKF_CULLED && A.not_erase && A.not_erase[r]) {      // src/KeyFrame.cc:459-463
        st = ORBHIP_CULLKF_NOT_ERASE;
        A.to_be_erased[r] = 1;
    }
    rep[0] = st; rep[1] = n_mp; rep[2] = n_red;
    for (int k = 3; k < 8; ++k) rep[k] = 0;
    A.verdict[u] = st;
}

// KeyFrame::SetBadFlag of candidate u up to the spanning tree (src/KeyFrame.cc:466-477).  Workgroup c < rows:
// EraseConnection on row c and entry c of the own row; it writes row c of the state and conn_w[r][c] only.  The workgroups
// behind them: EraseObservation for r's slots, one thread per slot.  r's slots are not written by this launch.
__global__ __launch_bounds__(256) void k_kf_apply(CullArgs A, int u)
{
    __shared__ unsigned long long s_key[kCuMaxRows];
    __shared__ int s_cnt[4];
    if (A.verdict[u] != ORBHIP_CULLKF_CULLED) return;
    const int tid = threadIdx.x, rows = A.rows, r = A.cand[u];
    int *rep = A.report + (size_t)u * 8;
    if ((int)blockIdx.x < rows) {
        const int c = blockIdx.x;
        if (c == r) {                                                      // :476-477
            if (tid < kCuCovis) A.covis[(size_t)r * kCuCovis + tid] = -1;
            if (tid == 0) { A.n_ord[r] = 0; A.conn_w[(size_t)r * rows + r] = 0; }
            return;
        }
        int *cw = A.conn_w + (size_t)c * rows;
        const int own = A.conn_w[(size_t)r * rows + c], back = cw[r];
        __syncthreads();                                                   // every read of the two entries is before their writes
        if (own == 0) return;                                              // :466: the own map names who is told
        if (tid == 0) A.conn_w[(size_t)r * rows + c] = 0;
        if (back == 0) return;                                             // :558: count() == 0, the row is left alone
        int N = 2;
        while (N < rows) N <<= 1;
        int mine = 0;
        for (int i = tid; i < N; i += 256) {
            unsigned long long key = 0;
            if (i < rows) {
                int v = cw[i];
                if (i == r) { cw[i] = 0; v = 0; }                          // :560
                if (v > 0) { key = (unsigned long long)(unsigned)v << 32 | (unsigned)i; ++mine; }
            }
            s_key[i] = key;
        }
        cv_resort_row(s_key, s_cnt, mine, N, A.ord_kf + (size_t)c * rows, A.ord_w + (size_t)c * rows, A.covis + (size_t)c * kCuCovis,
                      A.n_ord + c);
        if (tid == 0) atomicAdd(rep + 5, 1);
        return;
    }
    // :469-471
    const int n = min(max(A.n[r], 0), A.cap), stride = (gridDim.x - rows) * 256;
    int erased = 0, turned_bad = 0;
    for (int i = (blockIdx.x - rows) * 256 + tid; i < n; i += stride) {
        const int p = A.slot_point[(size_t)r * A.cap + i];
        if ((unsigned)p >= (unsigned)A.np) continue;
        int o0, o1, mine = -1;
        cu_list(A, p, o0, o1);
        for (int o = o0; o < o1; ++o)
            if (A.obs_kf[o] == r && A.alive[o]) {                          // mObservations.count(pKF): a row comes once
                if (atomicExch(&A.alive[o], 0) == 1) mine = o;             // the same point in another slot of r: one of us erases
                break;
            }
        if (mine < 0) continue;
        ++erased;
        const int idx = A.obs_idx[mine];
        const int nb = A.nobs[p] - (A.u_right && (unsigned)idx < (unsigned)A.cap && A.u_right[(size_t)r * A.cap + idx] >= 0.f ? 2 : 1);
        A.nobs[p] = nb;                                                    // src/MapPoint.cc:119-122
        if (A.ref_cur[p] == mine - o0) {                                   // :126-127: begin() is the first entry left
            int first = -1;
            for (int o = o0; o < o1 && first < 0; ++o)
                if (A.alive[o]) first = o - o0;
            A.ref_cur[p] = first;
        }
        int f = (A.flags[p] & ~ORBHIP_POINT_OBSERVED) | (nb > 0 ? ORBHIP_POINT_OBSERVED : 0);
        if (nb <= 2) {                                                     // :130-136
            f &= ~ORBHIP_POINT_PRESENT;
            ++turned_bad;
            for (int o = o0; o < o1; ++o) {
                if (!A.alive[o]) continue;
                A.alive[o] = 0;
                const int kf = A.obs_kf[o], ix = A.obs_idx[o];
                if (cu_obs_ok(A, kf, ix)) A.slot_point[(size_t)kf * A.cap + ix] = -1;
            }
        }
        A.flags[p] = (uint8_t)f;
    }
    erased = wave_sum(erased);
    turned_bad = wave_sum(turned_bad);
    if ((tid & 63) == 0) {
        if (erased) atomicAdd(rep + 3, erased);
        if (turned_bad) atomicAdd(rep + 4, turned_bad);
    }
}

// src/KeyFrame.cc:479-539 without mTcp: one wavefront.  The children of r (parent == r, not bad) and sParentCandidates are
// bitsets in LDS; a round walks the children in ascending row and their ordered lists in list order, and the first
// strictly largest weight to a candidate wins.
__device__ __forceinline__ void kf_reparent(const CullArgs &A, int u)
{
    __shared__ uint32_t s_cand[kCuMaxRows / 32], s_child[kCuMaxRows / 32];
    if (A.verdict[u] != ORBHIP_CULLKF_CULLED) return;
    const int lane = threadIdx.x, rows = A.rows, r = A.cand[u];
    for (int w = lane; w < kCuMaxRows / 32; w += 64) { s_cand[w] = 0; s_child[w] = 0; }
    wave_lds_handoff();
    int nchild = 0;
    for (int b = 0; b < rows; b += 64) {
        const int c = b + lane;
        const unsigned long long mk = __ballot(c < rows && A.parent[c] == r && !A.kf_bad[c]);
        if (lane == 0) { s_child[b >> 5] = (uint32_t)mk; s_child[(b >> 5) + 1] = (uint32_t)(mk >> 32); }
        nchild += __popcll(mk);
    }
    const int pr = A.parent[r];
    const bool has_parent = (unsigned)pr < (unsigned)rows;
    if (has_parent && lane == 0) s_cand[pr >> 5] |= 1u << (pr & 31);       // :481
    wave_lds_handoff();
    const int total = nchild, words = (rows + 31) >> 5;
    while (nchild > 0) {                                                   // :485
        int best_w = -1, best_c = -1, best_p = -1;
        for (int wd = 0; wd < words; ++wd) {
            uint32_t bits = s_child[wd];
            while (bits) {
                const int c = wd * 32 + __ffs(bits) - 1;
                bits &= bits - 1;
                const int n = min(max(A.n_ord[c], 0), rows);
                for (int b = 0; b < n; b += 64) {                          // :500-517
                    const int k = b + lane < n ? A.ord_kf[(size_t)c * rows + b + lane] : -1;
                    const bool ok = (unsigned)k < (unsigned)rows && ((s_cand[k >> 5] >> (k & 31)) & 1u);
                    const int w = ok ? max(A.conn_w[(size_t)c * rows + k], -1) : -2;
                    const int wmax = -wave_min(-w);
                    if (wmax > best_w) {                                   // :508
                        const unsigned long long mk = __ballot(ok && w == wmax);
                        best_w = wmax; best_c = c; best_p = __shfl(k, __ffsll((long long)mk) - 1);
                    }
                }
            }
        }
        if (best_c < 0) break;                                             // :526
        if (lane == 0) {                                                   // :522-524
            A.parent[best_c] = best_p;
            s_cand[best_c >> 5] |= 1u << (best_c & 31);
            s_child[best_c >> 5] &= ~(1u << (best_c & 31));
        }
        wave_lds_handoff();
        --nchild;
    }
    for (int wd = lane; wd < words; wd += 64) {                            // :531-535
        uint32_t bits = s_child[wd];
        while (bits) {
            A.parent[wd * 32 + __ffs(bits) - 1] = has_parent ? pr : -1;
            bits &= bits - 1;
        }
    }
    if (lane != 0) return;
    A.kf_bad[r] = 1;                                                       // :539
    A.report[(size_t)u * 8 + 6] = total;
    A.report[(size_t)u * 8 + 7] = nchild > 0 || !has_parent ? 1 : 0;
}

// Between two apply launches: workgroup 0 finishes candidate u (the spanning tree, first wavefront only), workgroup 1
// decides candidate u + 1.  The two touch different arrays: the verdict reads neither parents nor kf_bad, the spanning tree
// writes nothing else but its two report fields.
__global__ __launch_bounds__(256) void k_kf_step(CullArgs A, int u)
{
    if (blockIdx.x == 0) {
        if (u >= 0 && threadIdx.x < 64) kf_reparent(A, u);
    } else if (u + 1 < A.U) {
        kf_decide(A, u + 1);
    }
}

// The table without the erased entries: count, exclusive scan, ordered scatter.
__global__ __launch_bounds__(256) void k_cull_count(CullArgs A)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) / kCuGroup, gl = threadIdx.x & (kCuGroup - 1);
    if (p >= A.np) return;
    int o0, o1, cnt = 0;
    cu_list(A, p, o0, o1);
    for (int o = o0 + gl; o < o1; o += kCuGroup) cnt += A.alive[o] != 0;
    cnt = group_sum(cnt);
    if (gl == 0) A.obs_start_out[p] = cnt;
}

__global__ __launch_bounds__(256) void k_cull_scan(CullArgs A)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int running = 0;
    for (int b = 0; b < A.np; b += 256) {
        const int i = b + tid;
        const int v = i < A.np ? A.obs_start_out[i] : 0;
        const int incl = wave_incl_scan_add(v);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_w[w];
        if (i < A.np) A.obs_start_out[i] = off + incl - v;
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) A.obs_start_out[A.np] = running;
}

__global__ __launch_bounds__(256) void k_cull_scatter(CullArgs A)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) / kCuGroup, gl = threadIdx.x & (kCuGroup - 1);
    const int shift = threadIdx.x & 48;                                    // this group's 16 bits of a ballot
    const bool in = p < A.np;
    int o0 = 0, o1 = 0;
    if (in) cu_list(A, p, o0, o1);
    const int len = o1 - o0, ref = in ? A.ref_cur[p] : -1;
    int longest = len;                                                     // the ballots need every lane of the wavefront
    for (int s = 32; s >= kCuGroup; s >>= 1) longest = max(longest, __shfl_xor(longest, s));
    int out = in ? A.obs_start_out[p] : 0, ref_out = -1;
    for (int b = 0; b < longest; b += kCuGroup) {
        const int j = b + gl;
        const bool a = j < len && A.alive[o0 + j];
        const unsigned bits = (unsigned)(__ballot(a) >> shift) & 0xffffu;
        if (a) {
            const int dst = out + __popc(bits & ((1u << gl) - 1u));
            A.obs_kf_out[dst] = A.obs_kf[o0 + j];
            A.obs_idx_out[dst] = A.obs_idx[o0 + j];
            if (j == ref) A.ref_obs_out[p] = dst - A.obs_start_out[p];
        }
        if (j == ref && a) ref_out = 1;
        out += __popc(bits);
    }
    // the list is empty, or its reference observation is not in it
    const unsigned have = (unsigned)(__ballot(ref_out > 0) >> shift) & 0xffffu;
    if (in && gl == 0 && !have) A.ref_obs_out[p] = -1;
}

void carve(CullArgs &A, void *workspace)
{
    uint8_t *w = (uint8_t *)workspace;
    auto take = [&](size_t count) { int *q = (int *)w; w += al256(count * sizeof(int)); return q; };
    A.nobs = take(A.np); A.ref_cur = take(A.np); A.owner = take(A.np); A.alive = take(A.obs_cap); A.cand = take(A.U); A.verdict = take(A.U);
}

int point_blocks(int count) { return std::max(1, (int)(((size_t)count * kCuGroup + 255) / 256)); }

void close_out(hipStream_t stream, const CullArgs &A)
{
    hipLaunchKernelGGL(k_cull_count, dim3(point_blocks(A.np)), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(256), 0, stream, A);
    hipLaunchKernelGGL(k_cull_scatter, dim3(point_blocks(A.np)), dim3(256), 0, stream, A);
}

}  // namespace

size_t cull_workspace_bytes(int np, int obs_cap, int U)
{
    return 3 * al256((size_t)np * sizeof(int)) + al256((size_t)obs_cap * sizeof(int)) + 2 * al256((size_t)U * sizeof(int));
}

int launch_cull_map_points(hipStream_t stream, CullArgs A, void *workspace)
{
    A.U = 0;
    carve(A, workspace);
    hipLaunchKernelGGL(k_cull_init, dim3(point_blocks(A.np)), dim3(256), 0, stream, A);
    if (A.R > 0) {
        hipLaunchKernelGGL(k_mp_own, dim3((A.R + 255) / 256), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(k_mp_decide, dim3(1), dim3(256), 0, stream, A);
        hipLaunchKernelGGL(k_mp_act, dim3(point_blocks(A.R)), dim3(256), 0, stream, A);
    } else {
        ORBHIP_HIP_CHECK(hipMemsetAsync(A.n_recent_out, 0, sizeof(int), stream));
    }
    close_out(stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int launch_cull_key_frames(hipStream_t stream, CullArgs A, void *workspace)
{
    carve(A, workspace);
    const int init_blocks = std::max(point_blocks(A.np), (A.U + 255) / 256);
    hipLaunchKernelGGL(k_cull_init, dim3(init_blocks), dim3(256), 0, stream, A);
    const int slot_blocks = std::max(1, std::min(16, (A.cap + 255) / 256));
    if (A.U > 0) hipLaunchKernelGGL(k_kf_step, dim3(2), dim3(256), 0, stream, A, -1);
    for (int u = 0; u < A.U; ++u) {
        hipLaunchKernelGGL(k_kf_apply, dim3(A.rows + slot_blocks), dim3(256), 0, stream, A, u);
        hipLaunchKernelGGL(k_kf_step, dim3(2), dim3(256), 0, stream, A, u);
    }
    close_out(stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return launch_children_from_parents(stream, A.rows, A.parent, A.kf_bad, A.child_start, A.child);
}

}  // namespace orbhip
