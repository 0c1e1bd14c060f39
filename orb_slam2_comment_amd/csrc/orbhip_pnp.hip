// PnP RANSAC on the device: PnPsolver (src/PnPsolver.cc) for the current frame and C relocalisation candidates
// (include/orbhip.h, section "PnP RANSAC").  gfx950 only, wave64.  The arithmetic is tests/seqref/pnp.py operation by
// operation; EPnP itself is orbhip_pnp_core.h, which the host can replay bit for bit.  No float
// atomics: a floating-point sum belongs to one lane and runs in the order of the correspondences, the only values reduced
// across lanes are inlier bits and integer counts, so nothing depends on the launch geometry.
//
// Launches, all on the caller's stream:
//   k_pnp_setup        one workgroup per candidate: the keep rule of the constructor per slot of the frame, ordered compaction,
//                      the adjusted (min inliers, limit) of the table entry N
//   k_pnp_hypotheses   one team of 16 lanes per (candidate, iteration of this call), four teams per wavefront: the draw replay,
//                      four-point EPnP with its workspace in LDS (12 lanes own the rows of the 12x12 eigenproblem)
//   k_pnp_score        one wavefront per hypothesis: CheckInliers over N, a ballot per 64, mask bytes and the count
//   k_pnp_select       one wavefront per candidate: the strict running maximum over the iteration numbers, seeded from the
//                      state; marks the record-setters that pass the gate -- the sets Refine() can ever see
//   k_pnp_refine       one workgroup per (candidate, entry): entry 0 is the best set the solver record holds, entry 1 + j the
//                      set of record-setter j; idle workgroups leave at once.  n-point EPnP, CheckInliers, the refined count
//   k_pnp_final        one wavefront per candidate: the first iteration that passes the gate while the refinement of the
//                      best set so far succeeds returns; otherwise the limit rule; report, state, best set, outputs
#include "orbhip_internal.h"
#include "orbhip_pnp_core.h"

#include <algorithm>

namespace orbhip {
namespace {

__global__ __launch_bounds__(256) void k_pnp_setup(PnpArgs A)
{
    __shared__ int s_w[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int kf = A.match_form == ORBHIP_PNP_MATCH_SLOTS ? A.kf_index[c] : 0;
    const bool kf_ok = A.match_form != ORBHIP_PNP_MATCH_SLOTS || (unsigned)kf < (unsigned)A.rows;
    const size_t row = (size_t)c * A.cap;
    const int lv_max = min(max(A.n_levels, 1), ORBHIP_MAX_LEVELS) - 1;
    int running = 0;
    for (int b = 0; b < A.n; b += 256) {
        const int i = b + tid;
        int p = -1;
        if (i < A.n && kf_ok) {
            const int m = A.matches[row + i];
            if (m >= 0) p = A.match_form == ORBHIP_PNP_MATCH_SLOTS ? (m < A.cap ? A.slot_point[(size_t)kf * A.cap + m] : -1) : m;   // :83
        }
        const bool keep = (unsigned)p < (unsigned)A.np && (A.flags[p] & ORBHIP_POINT_PRESENT);                                        // :85
        const int incl = wave_incl_scan_add(keep ? 1 : 0);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_w[w];
        if (keep) {
            const size_t k = row + off + incl - 1;
            const orbhip_keypoint kp = A.kps[i];
            A.p2d[k * 2] = kp.x; A.p2d[k * 2 + 1] = kp.y;
            A.max_err[k] = A.max_err_lv[min(max(kp.octave, 0), lv_max)];
            for (int r = 0; r < 3; ++r) A.p3d[k * 3 + r] = A.world[(size_t)p * 3 + r];
            A.kp_index[k] = i;
        }
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) {
        A.n_corr[c] = running;
        A.min_inliers[c] = A.tab[2 * running];
        A.limit[c] = A.tab[2 * running + 1];
        A.state[2 * c] = 0;
        A.state[2 * c + 1] = 0;
    }
}

// the iteration numbers a call runs for candidate c: [it0, it0 + n_run), n_run = max(limit, it0 + n_iterations) - it0 (:182)
__device__ __forceinline__ int pnp_run(const PnpArgs &A, int c, int &it0, int &N, int &n_min)
{
    N = min(max(A.n_corr[c], 0), A.cap);
    n_min = A.min_inliers[c];
    it0 = A.state[2 * c];
    if (N < n_min || N < 4 || it0 < 0) return 0;
    const int end = min(max(A.limit[c], it0 + A.n_iter), A.draw_rows);
    return min(max(end - it0, 0), A.W);
}

__device__ __forceinline__ PnpCorr pnp_corr(const PnpArgs &A, int c)
{
    PnpCorr S;
    S.p3d = A.p3d + (size_t)c * A.cap * 3;
    S.p2d = A.p2d + (size_t)c * A.cap * 2;
    S.mask = nullptr; S.idx = nullptr; S.lim = 0;
    S.fu = A.fu; S.fv = A.fv; S.uc = A.uc; S.vc = A.vc;
    return S;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(PnpArgs A)
{
    __shared__ PnpWs s_ws[4];
    __shared__ int s_opos[4][4], s_oval[4][4];
    const int c = blockIdx.y, team = threadIdx.x >> 4, tl = threadIdx.x & 15, j = blockIdx.x * 4 + team;
    int it0, N, n_min;
    if (j >= pnp_run(A, c, it0, N, n_min)) return;
    PnpWs &W = s_ws[team];
    if (tl == 0) {
        // :188-201.  The list starts as the identity; taking position r out moves the last entry there: at most three
        // positions ever differ from their index.
        const int *d = A.draws + ((size_t)c * A.draw_rows + it0 + j) * 4;
        int *opos = s_opos[team], *oval = s_oval[team];
        for (int k = 0; k < 4; ++k) {
            const int size = N - k, r = min(max(d[k], 0), size - 1);
            int at = r, last = size - 1;
            for (int m = k - 1; m >= 0; --m)
                if (opos[m] == r) { at = oval[m]; break; }
            for (int m = k - 1; m >= 0; --m)
                if (opos[m] == size - 1) { last = oval[m]; break; }
            W.idx[k] = at;
            opos[k] = r; oval[k] = last;
        }
        W.n = 4;
        W.first = W.idx[0];
    }
    wave_lds_handoff();
    PnpCorr S = pnp_corr(A, c);
    S.idx = W.idx; S.lim = 4;
    pnp_compute_pose<16>(W, S, tl);
    double *h = A.hyp + ((size_t)c * A.W + j) * 12;
    if (tl < 9) h[tl] = W.bestR[tl];
    else if (tl < 12) h[tl] = W.bestT[tl - 9];
}

__global__ __launch_bounds__(256) void k_pnp_score(PnpArgs A)
{
    const int c = blockIdx.y, lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    int it0, N, n_min;
    if (j >= pnp_run(A, c, it0, N, n_min)) return;
    const double *hp = A.hyp + ((size_t)c * A.W + j) * 12;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = hp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = hp[9 + i];
    uint8_t *mask = A.mask + ((size_t)c * A.W + j) * A.cap;
    const size_t row = (size_t)c * A.cap;
    int count = 0;
    for (int b = 0; b < N; b += 64) {
        const int i = b + lane;
        const bool in = i < N && pnp_inlier(R, t, A.p3d + (row + i) * 3, A.p2d + (row + i) * 2, A.max_err[row + i], A.fu, A.fv, A.uc, A.vc);
        if (i < N) mask[i] = in ? 1 : 0;
        count += __popcll(__ballot(in));
    }
    if (lane == 0) A.count[(size_t)c * A.W + j] = count;
}

// inclusive maximum scan over the wavefront
__device__ __forceinline__ int wave_scan_max(int v, int lane)
{
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s);
        if (lane >= s) v = max(v, o);
    }
    return v;
}

__global__ __launch_bounds__(64) void k_pnp_select(PnpArgs A)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    int it0, N, n_min;
    const int n_run = pnp_run(A, c, it0, N, n_min);
    int best = A.state[2 * c + 1];
    for (int b = 0; b < n_run; b += 64) {
        const int j = b + lane;
        int cnt = j < n_run ? A.count[(size_t)c * A.W + j] : -1;
        if (cnt < n_min) cnt = -1;                                              // :209: only a count that passes the gate can be a best
        const int incl = wave_scan_max(cnt, lane);
        int before = __shfl_up(incl, 1);
        before = lane == 0 ? best : max(before, best);
        if (j < n_run) A.is_rec[(size_t)c * A.W + j] = cnt > before ? 1 : 0;     // :212, strict
        best = max(best, __shfl(incl, 63));
    }
}

__global__ __launch_bounds__(256) void k_pnp_refine(PnpArgs A)
{
    __shared__ PnpWs W;
    __shared__ int s_n, s_first, s_inl;
    const int c = blockIdx.y, e = blockIdx.x, tid = threadIdx.x;
    int it0, N, n_min;
    const int n_run = pnp_run(A, c, it0, N, n_min);
    if (n_run <= 0) return;
    const uint8_t *src;
    if (e == 0) {
        if (A.state[2 * c + 1] < n_min) return;                                 // the record holds no best set
        src = A.best_inliers + (size_t)c * A.cap;
    } else {
        if (e - 1 >= n_run || !A.is_rec[(size_t)c * A.W + e - 1]) return;
        src = A.mask + ((size_t)c * A.W + e - 1) * A.cap;
    }
    if (tid == 0) { s_n = 0; s_first = N; s_inl = 0; }
    __syncthreads();
    int mine = 0, first = N;
    for (int i = tid; i < N; i += 256)
        if (src[i]) { ++mine; first = min(first, i); }
    if (mine) { atomicAdd(&s_n, mine); atomicMin(&s_first, first); }
    __syncthreads();
    if (s_n <= 0) return;
    if (tid == 0) { W.n = s_n; W.first = s_first; }
    __syncthreads();
    PnpCorr S = pnp_corr(A, c);
    S.mask = src; S.lim = N;
    pnp_compute_pose<256>(W, S, tid);
    const size_t row = (size_t)c * A.cap, ent = (size_t)c * (A.W + 1) + e;
    uint8_t *out = A.ref_mask + ent * A.cap;
    mine = 0;
    for (int i = tid; i < N; i += 256) {
        const bool in = pnp_inlier(W.bestR, W.bestT, A.p3d + (row + i) * 3, A.p2d + (row + i) * 2, A.max_err[row + i], A.fu, A.fv, A.uc, A.vc);
        out[i] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    if (mine) atomicAdd(&s_inl, mine);
    __syncthreads();
    if (tid < 12) A.ref_T[ent * 12 + tid] = (float)((tid & 3) == 3 ? W.bestT[tid >> 2] : W.bestR[(tid >> 2) * 3 + (tid & 3)]);
    if (tid == 0) A.ref_cnt[ent] = s_inl;
}

__global__ __launch_bounds__(64) void k_pnp_final(PnpArgs A)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    int it0, N, n_min;
    const int n_run = pnp_run(A, c, it0, N, n_min);
    int *rep = A.report + (size_t)c * 8;
    const int limit = A.limit[c], best0 = A.state[2 * c + 1];
    if (N < n_min) {                                                            // :173
        if (lane == 0) {
            rep[0] = ORBHIP_PNP_TOO_FEW; rep[1] = N; rep[2] = limit; rep[3] = A.state[2 * c]; rep[4] = best0; rep[5] = -1; rep[6] = 0;
            rep[7] = n_min;
        }
        return;
    }
    const int *cnts = A.count + (size_t)c * A.W, *is_rec = A.is_rec + (size_t)c * A.W;
    const int *ref_cnt = A.ref_cnt + (size_t)c * (A.W + 1);
    int last_rec = -1, found = -1, found_e = 0;
    for (int b = 0; b < n_run && found < 0; b += 64) {
        const int j = b + lane;
        const bool in = j < n_run;
        const int cnt = in ? cnts[j] : -1;
        const int rec = wave_scan_max(in && is_rec[j] ? j : -1, lane);          // the record-setter whose set is the best after j
        const int cur = max(rec, last_rec);
        bool ok = false;
        if (in && cnt >= n_min) {                                               // :209, then Refine() of the best set so far
            if (cur >= 0) ok = ref_cnt[cur + 1] > n_min;                        // :292, strict
            else if (best0 >= n_min) ok = ref_cnt[0] > n_min;
        }
        const unsigned long long hit = __ballot(ok);
        if (hit) {
            const int l = __ffsll((long long)hit) - 1;
            found = b + l;
            last_rec = __shfl(cur, l);
            found_e = last_rec + 1;
        } else {
            last_rec = __shfl(cur, 63);
        }
    }
    const int best = last_rec >= 0 ? cnts[last_rec] : best0;
    const int iters = found >= 0 ? it0 + found + 1 : it0 + n_run;
    const int status = found >= 0 ? ORBHIP_PNP_REFINED : (best >= n_min ? ORBHIP_PNP_BEST : ORBHIP_PNP_NO_MORE);
    const size_t ent = (size_t)c * (A.W + 1) + found_e;
    if (lane == 0) {
        rep[0] = status; rep[1] = N; rep[2] = limit; rep[3] = iters; rep[4] = best;
        rep[5] = found >= 0 ? it0 + found : -1;
        rep[6] = found >= 0 ? ref_cnt[found_e] : (status == ORBHIP_PNP_BEST ? best : 0);
        rep[7] = n_min;
        A.state[2 * c] = iters; A.state[2 * c + 1] = best;
    }
    // mvbBestInliers / mBestTcw (:214-223) of the last record-setter the loop reached
    uint8_t *bi = A.best_inliers + (size_t)c * A.cap;
    float *bt = A.best_Tcw + (size_t)c * 12;
    float tcw = 0.f;
    if (last_rec >= 0) {
        const uint8_t *m = A.mask + ((size_t)c * A.W + last_rec) * A.cap;
        for (int i = lane; i < N; i += 64) bi[i] = m[i];
        const double *h = A.hyp + ((size_t)c * A.W + last_rec) * 12;
        if (lane < 12) {
            tcw = (float)((lane & 3) == 3 ? h[9 + (lane >> 2)] : h[(lane >> 2) * 3 + (lane & 3)]);
            bt[lane] = tcw;
        }
    } else if (lane < 12 && status == ORBHIP_PNP_BEST) {
        tcw = bt[lane];
    }
    if (status == ORBHIP_PNP_NO_MORE) return;
    // the returned pose and vbInliers over the key-point slots (:228-235, :246-253)
    const uint8_t *m = found >= 0 ? A.ref_mask + ent * A.cap
                                  : (last_rec >= 0 ? A.mask + ((size_t)c * A.W + last_rec) * A.cap : A.best_inliers + (size_t)c * A.cap);
    if (lane < 12) A.Tcw[(size_t)c * 12 + lane] = found >= 0 ? A.ref_T[ent * 12 + lane] : tcw;
    uint8_t *inl = A.inliers + (size_t)c * A.cap;
    const int n = min(A.n, A.cap);
    for (int i = lane; i < n; i += 64) inl[i] = 0;
    __threadfence();                                                            // the zeros land before the marks
    const int *kp_index = A.kp_index + (size_t)c * A.cap;
    for (int i = lane; i < N; i += 64)
        if (m[i]) {
            const int s = kp_index[i];
            if ((unsigned)s < (unsigned)n) inl[s] = 1;
        }
}

}  // namespace

static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

size_t pnp_workspace_bytes(int C, int W, int cap)
{
    const size_t H = (size_t)std::max(C, 1) * std::max(W, 1), E = (size_t)std::max(C, 1) * (std::max(W, 1) + 1);
    return al(H * 12 * sizeof(double)) + 2 * al(H * sizeof(int)) + al(H * cap) + al(E * 12 * sizeof(float)) + al(E * sizeof(int)) +
           al(E * cap) + 256;
}

int launch_pnp_setup(hipStream_t stream, PnpArgs A)
{
    if (A.C <= 0) return ORBHIP_OK;
    hipLaunchKernelGGL(k_pnp_setup, dim3(A.C), dim3(256), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int launch_pnp_iterate(hipStream_t stream, PnpArgs A, void *workspace)
{
    if (A.C <= 0) return ORBHIP_OK;
    const size_t H = (size_t)A.C * A.W, E = (size_t)A.C * (A.W + 1);
    uint8_t *w = (uint8_t *)workspace;
    A.hyp = (double *)w;      w += al(H * 12 * sizeof(double));
    A.count = (int *)w;       w += al(H * sizeof(int));
    A.is_rec = (int *)w;      w += al(H * sizeof(int));
    A.mask = w;               w += al(H * A.cap);
    A.ref_T = (float *)w;     w += al(E * 12 * sizeof(float));
    A.ref_cnt = (int *)w;     w += al(E * sizeof(int));
    A.ref_mask = w;
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((A.W + 3) / 4, A.C), dim3(64), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_score, dim3((A.W + 3) / 4, A.C), dim3(256), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_select, dim3(A.C), dim3(64), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_refine, dim3(A.W + 1, A.C), dim3(256), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_final, dim3(A.C), dim3(64), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
