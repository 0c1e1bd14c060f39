// Global bundle adjustment on the device: Optimizer::BundleAdjustment (src/Optimizer.cc:49-237) and the map update of
// LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:676-737), include/orbhip.h section "global bundle adjustment".
// gfx950 only, wave64.  The arithmetic is tests/seqref/gba.py operation by operation; the items are
// orbhip_lba_core.h's and orbhip_gba_core.h's, which the host replays bit for bit.
//
// The number of trials depends on the data, so the launch function reads the state record back once after the setup and once
// per trial (one small pinned copy, one stream synchronisation) and enqueues the next step from it: the call synchronises.
// One stream, no cooperative launch, no workgroup waits for another; every kernel reads the phase of the state record first and
// leaves when its step is not due.
//   k_gba_setup        one workgroup of 1024: the vertices by a scan over the key-frame list, maxKFid, the free poses by a scan
//                      over the vertices, then per listed point its edges counted, two scans (included points, edges) and the
//                      edges written in creation order; the first estimates
//   k_gba_index        one wavefront per free pose: its edges ascending (ballot compaction over the edge list); the
//                      co-visibility table cleared
//   k_gba_covis        per point: the pairs (i1 <= i2) of free poses among its edges
//   k_gba_linearize, k_gba_blocks, k_gba_begin   a linearisation: edge records, Hll / b_l per point, Hpp / b_p per free pose
//                      (one wavefront each), chi2, the largest diagonal, lambda
//   k_gba_dinv, k_gba_schur   a trial's system: one wavefront per pair of free poses; a pair that shares no point stores its
//                      zero block without walking an edge list (at 512 free poses most of the 131 k pairs are such)
//   ldlt::k_*          orbhip_ldlt.h: the blocked unpivoted LDLt and the substitutions, panels of kGbaPanel poses, in place on b
//   k_gba_x, k_gba_update, k_gba_trial, k_gba_judge   the solution taken, the tried estimates, chi2 at them, the decision
//   k_gba_finish       one workgroup of 1024: the write-back of the mode, the report
//   k_gba_apply_walk   one wavefront: lpKFtoCheck in LDS, a popped row's children found by a ballot over the parent table
//   k_gba_apply_points one lane per point
#include "orbhip_internal.h"
#include "orbhip_lba_dev.h"
#include "orbhip_ldlt.h"

namespace orbhip {
namespace {
using namespace lbadev;

constexpr int kBig = 1024, kItem = 256, kItemBlocks = 240, kSchurBlocks = 1024, kRowsMax = 4096;

enum { kSMaxId = 0, kSRemoved, kSSkipped, kSNull, kSStereo, kSPoses, kSInts };

__device__ void gba_setup_done(GbaWs &G, const int *s_i, int nv, int nfree, int npts, int ne, int status)
{
    LbaState &S = *G.L.S;
    GbaCount &C = *G.C;
    memset(&S, 0, sizeof(S));
    memset(&C, 0, sizeof(C));
    S.n_lkf = nv; S.n_free = nfree; S.n_pts = npts; S.n_edges = ne; S.n_stereo = s_i[kSStereo]; S.n_mono = ne - s_i[kSStereo];
    S.n_active = ne; S.poses[0] = s_i[kSPoses]; S.status = status;
    C.max_kfid = s_i[kSMaxId]; C.n_removed = s_i[kSRemoved]; C.n_skipped = s_i[kSSkipped]; C.n_null = s_i[kSNull];
    gba_begin(G);
}

__global__ __launch_bounds__(kBig) void k_gba_setup(GbaWs G)
{
    __shared__ int s_w[kBig / 64];
    __shared__ int s_i[kSInts];
    __shared__ int s_cnt[kGbaMaxKf + 1];
    LbaWs &W = G.L;
    const int tid = threadIdx.x;
    for (int r = tid; r < W.rows; r += kBig) { W.kf_vtx[r] = -1; W.vtx_free[r] = -1; }
    for (int k = tid; k < 6 * W.max_free; k += kBig) W.xp[k] = 0.0;
    if (tid <= kGbaMaxKf) s_cnt[tid] = 0;
    if (tid < kSInts) s_i[tid] = 0;
    __syncthreads();
    // the vertices (:71-83): the listed rows that are not bad, in list order; maxKFid
    const int nkf = gba_nkf(G), vcap = W.rows < kGbaMaxKf ? W.rows : kGbaMaxKf;
    int nv = 0;
    for (int base = 0; base < nkf; base += kBig) {
        const int i = base + tid, r = i < nkf ? gba_kf_at(G, i) : -1;
        const bool good = i < nkf && gba_row_good(G, r);
        int all;
        const int pos = nv + block_excl_scan<kBig>(good ? 1 : 0, s_w, &all);
        if (good && pos < vcap) { W.lkf[pos] = r; W.vtx_row[pos] = r; W.kf_vtx[r] = pos; }
        if (good) atomicMax(&s_i[kSMaxId], G.kf_id[r]);
        nv += all;
    }
    __syncthreads();
    if (nv > kGbaMaxKf) {
        if (tid == 0) gba_setup_done(G, s_i, nv, 0, 0, 0, ORBHIP_GBA_CAPACITY);
        return;
    }
    int nfree = 0;
    for (int base = 0; base < nv; base += kBig) {
        const int v = base + tid;
        const bool fr = v < nv && G.kf_id[W.vtx_row[v]] != 0;                      // setFixed(pKF->mnId == 0)
        int all;
        const int pos = nfree + block_excl_scan<kBig>(fr ? 1 : 0, s_w, &all);
        if (v < nv) W.vtx_free[v] = fr ? pos : -1;
        nfree += all;
    }
    __syncthreads();
    // the points and their edges (:89-184), in list order
    const int npt = gba_npt(G), max_kfid = s_i[kSMaxId];
    int npts = 0, ne = 0;
    for (int base = 0; base < npt; base += kBig) {
        const int i = base + tid, p = i < npt ? gba_pt_at(G, i) : -1;
        const bool cand = i < npt && gba_point_listed(G, p);
        int c = 0, ns = 0, sk = 0, nl = 0;
        if (cand)
            for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
                const int kind = gba_obs_kind(G, o, max_kfid);
                if (kind == 1) { ++sk; continue; }
                if (kind == 2) { ++nl; continue; }
                ++c;
                if (gba_obs_stereo(G, o)) ++ns;
            }
        if (sk) atomicAdd(&s_i[kSSkipped], sk);
        if (nl) atomicAdd(&s_i[kSNull], nl);
        if (ns) atomicAdd(&s_i[kSStereo], ns);
        if (cand && c == 0) atomicAdd(&s_i[kSRemoved], 1);                         // vbNotIncludedMP
        int all_p, all_e;
        const int pos = npts + block_excl_scan<kBig>(c > 0 ? 1 : 0, s_w, &all_p);
        const int off = ne + block_excl_scan<kBig>(c, s_w, &all_e);
        if (c > 0 && pos < W.max_points && off + c <= W.max_edges) {
            W.pt_e0[pos] = off;
            gba_point_init(G, pos, p);
            int j = off;
            for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
                if (gba_obs_kind(G, o, max_kfid) != 0) continue;
                gba_edge_write(G, j, o, pos);
                const int f = G.e_free[j];
                if (f >= 0) atomicAdd(&s_cnt[f + 1], 1);
                ++j;
            }
        }
        npts += all_p; ne += all_e;
    }
    __syncthreads();
    if (npts > W.max_points || ne > W.max_edges) {
        if (tid == 0) gba_setup_done(G, s_i, nv, nfree, npts, ne, ORBHIP_GBA_CAPACITY);
        return;
    }
    for (int v = tid; v < nv; v += kBig) gba_vertex_init(G, v);
    if (tid == 0) {
        W.pt_e0[npts] = ne;
        int poses = 0;
        for (int f = 0; f < nfree; ++f) { W.pose_active[f] = s_cnt[f + 1] > 0 ? 1 : 0; poses += W.pose_active[f]; s_cnt[f + 1] += s_cnt[f]; }
        for (int f = 0; f <= nfree; ++f) W.kf_e0[f] = s_cnt[f];
        s_i[kSPoses] = poses;
        gba_setup_done(G, s_i, nv, nfree, npts, ne, ORBHIP_GBA_OK);
    }
}

__global__ __launch_bounds__(kItem) void k_gba_index(GbaWs G)
{
    const LbaWs &W = G.L;
    if (W.S->phase != kLbaBuild) return;
    const int tid = threadIdx.x, lane = tid & 63, nfree = W.S->n_free, ne = W.S->n_edges;
    const int waves = gridDim.x * (kItem / 64);
    for (int f = blockIdx.x * (kItem / 64) + (tid >> 6); f < nfree; f += waves) {
        int base = W.kf_e0[f];
        for (int j0 = 0; j0 < ne; j0 += 64) {
            const int j = j0 + lane;
            const bool mine = j < ne && G.e_free[j] == f;
            const unsigned long long mask = __ballot(mine);
            if (mine) W.kf_edges[base + lane_prefix(mask)] = j;
            base += __popcll(mask);
        }
    }
    const int nn = nfree * nfree;
    for (int k = blockIdx.x * kItem + tid; k < nn; k += gridDim.x * kItem) G.cov[k] = 0;
}

__global__ __launch_bounds__(kItem) void k_gba_covis(GbaWs G)
{
    const LbaWs &W = G.L;
    if (W.S->phase != kLbaBuild) return;
    const int np = W.S->n_pts, nfree = W.S->n_free;
    for (int i = blockIdx.x * kItem + threadIdx.x; i < np; i += gridDim.x * kItem) {
        const int e0 = W.pt_e0[i], e1 = W.pt_e0[i + 1];
        for (int j1 = e0; j1 < e1; ++j1) {
            const int f1 = G.e_free[j1];
            if (f1 < 0) continue;
            for (int j2 = e0; j2 < e1; ++j2) {
                const int f2 = G.e_free[j2];
                if (f2 >= f1) G.cov[(size_t)f1 * nfree + f2] = 1;
            }
        }
    }
}

// ---- a linearisation --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kItem) void k_gba_linearize(LbaWs W)
{
    if (W.S->phase == kLbaBuild) phase_linearize<kItem>(W);
}

__global__ __launch_bounds__(kItem) void k_gba_blocks(LbaWs W)
{
    if (W.S->phase != kLbaBuild) return;
    const int tid = threadIdx.x, lane = tid & 63, nfree = W.S->n_free, np = W.S->n_pts;
    const int waves = gridDim.x * (kItem / 64);
    for (int f = blockIdx.x * (kItem / 64) + (tid >> 6); f < nfree; f += waves) pose_block(W, f, lane);
    for (int i = blockIdx.x * kItem + tid; i < np; i += gridDim.x * kItem) lba_point_block(W, i);
}

// a factorisation that has not failed is ok2 = 1: the solve kernels only ever clear it (GbaView::fail)
__global__ __launch_bounds__(kLbaTeam) void k_gba_begin(LbaWs W)
{
    __shared__ double s_part[kLbaTeam / kLbaWave];
    if (W.S->phase != kLbaBuild) return;
    phase_lm_begin(W, s_part);
    if (threadIdx.x == 0) W.S->ok2 = 1;
}

// ---- a trial ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kItem) void k_gba_dinv(LbaWs W)
{
    if (W.S->phase == kLbaTrial) phase_dinv<kItem>(W);
}

__global__ __launch_bounds__(kItem) void k_gba_schur(GbaWs G)
{
    const LbaWs &W = G.L;
    if (W.S->phase != kLbaTrial) return;
    const int tid = threadIdx.x, lane = tid & 63, nfree = W.S->n_free;
    const int waves = gridDim.x * (kItem / 64);
    for (int t = blockIdx.x * (kItem / 64) + (tid >> 6); t < nfree * nfree; t += waves) {
        const int i1 = t / nfree, i2 = t - i1 * nfree;
        if (i2 < i1) continue;
        schur_pair(W, i1, i2, lane, i1 == i2 || G.cov[t] != 0);
    }
}

// the system as orbhip_ldlt.h sees it: solved in place on b; a failed pivot is ok2 = false of the state machine
struct GbaView {
    LbaWs W;
    __device__ __forceinline__ double *A() const { return W.A; }
    __device__ __forceinline__ double *y() const { return W.bs; }
    __device__ __forceinline__ int n() const { return 6 * W.S->n_free; }
    __device__ __forceinline__ bool due() const { return W.S->phase == kLbaTrial && W.S->ok2 != 0; }
    __device__ __forceinline__ void fail() const { W.S->ok2 = 0; }
};

__global__ __launch_bounds__(kItem) void k_gba_x(LbaWs W)
{
    if (W.S->phase != kLbaTrial || !W.S->ok2) return;                              // a failed factorisation leaves the stale x
    const int n = 6 * W.S->n_free;
    for (int k = blockIdx.x * kItem + threadIdx.x; k < n; k += gridDim.x * kItem) W.xp[k] = W.bs[k];
}

__global__ __launch_bounds__(kItem) void k_gba_update(LbaWs W)
{
    if (W.S->phase == kLbaTrial) phase_update<kItem>(W);
}

__global__ __launch_bounds__(kItem) void k_gba_trial(LbaWs W)
{
    if (W.S->phase == kLbaTrial) phase_trial<kItem>(W);
}

__global__ __launch_bounds__(kLbaTeam) void k_gba_judge(LbaWs W)
{
    __shared__ double s_part[kLbaTeam / kLbaWave];
    if (W.S->phase != kLbaTrial) return;
    phase_lm_judge(W, s_part);
    if (threadIdx.x == 0) W.S->ok2 = 1;
}

__global__ __launch_bounds__(kBig) void k_gba_finish(GbaWs G)
{
    const LbaWs &W = G.L;
    if (W.S->phase != kLbaFinal) return;
    const int tid = threadIdx.x;
    LbaState &S = *W.S;
    if (gba_writes(S)) {
        for (int v = tid; v < S.n_lkf; v += kBig) gba_write_pose(G, v);
        for (int i = tid; i < S.n_pts; i += kBig) gba_write_point(G, i);
    }
    __syncthreads();
    if (tid == 0) {
        G.C->n_listed = gba_writes(S) && G.mode == ORBHIP_GBA_IN_PLACE ? S.n_pts : 0;
        gba_write_report(G);
        S.phase = kLbaDone;
    }
}

// ---- the apply step -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_gba_apply_walk(GbaApply A)
{
    __shared__ int s_par[kRowsMax], s_q[kRowsMax];
    const int lane = threadIdx.x, rows = A.rows;
    for (int r = lane; r < rows; r += 64) { s_par[r] = gba_apply_row_good(A, r) ? A.parent[r] : -2; A.visited[r] = 0; }
    __syncthreads();
    int tail = 0, pops = 0, propagated = 0;
    for (int base = 0; base < A.n_origins; base += 64) {                           // lpKFtoCheck(mvpKeyFrameOrigins)
        const int i = base + lane, o = i < A.n_origins ? A.origins[i] : -1;
        const bool ok = i < A.n_origins && gba_apply_origin(A, o);
        const unsigned long long mask = __ballot(ok);
        const int pos = tail + lane_prefix(mask);
        if (ok && pos < rows) s_q[pos] = o;
        tail = min(rows, tail + __popcll(mask));
    }
    __syncthreads();
    for (int head = 0; head < tail; ++head) {                                      // at most `rows` pops: the queue holds no more
        const int k = s_q[head];
        float Twc[12];
        gba_inverse(A.Tcw + (size_t)k * 12, Twc);                                  // GetPoseInverse() before this row's SetPose
        for (int c0 = 0; c0 < rows; c0 += 64) {                                    // GetChilds(): ascending row
            const int c = c0 + lane;
            const bool child = c < rows && s_par[c] == k;
            const bool fresh = child && !A.kf_mark[c];
            if (fresh) gba_apply_child(A, k, c, Twc);
            propagated += __popcll(__ballot(fresh));
            const unsigned long long mask = __ballot(child);
            const int pos = tail + lane_prefix(mask);
            if (child && pos < rows) s_q[pos] = c;
            tail = min(rows, tail + __popcll(mask));
        }
        __syncthreads();                                                           // every lane has read Tcw[k]; the children are written
        if (lane < 12) {
            const size_t at = (size_t)k * 12 + lane;
            A.TcwBef[at] = A.Tcw[at]; A.Tcw[at] = A.TcwGBA[at];
        }
        if (lane == 0) A.visited[k] = 1;
        __syncthreads();
        ++pops;
    }
    if (lane < 8) A.o_report[lane] = lane == 0 ? pops : (lane == 1 ? propagated : 0);
}

__global__ __launch_bounds__(kItem) void k_gba_apply_points(GbaApply A)
{
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * kItem; base < A.pcap; base += gridDim.x * kItem) {
        const int p = base + threadIdx.x;
        const int kind = p < A.pcap ? gba_apply_point(A, p) : 0;
        for (int q = 1; q <= 3; ++q) {
            const int c = __popcll(__ballot(kind == q));
            if (c && lane == 0) { atomicAdd(&A.o_report[1 + q], c); atomicAdd(&A.o_report[5], c); }
        }
    }
}

}  // namespace

size_t gba_workspace_bytes(GbaWs G) { return gba_carve(G, nullptr); }
size_t gba_apply_workspace_bytes(GbaApply A) { return gba_apply_carve(A, nullptr); }

// h_state: a pinned LbaState the call reads the device's record into; counters[2], nullable, receives the synchronisations and
// the launches of the call
int launch_global_bundle_adjustment(hipStream_t stream, GbaWs G, void *workspace, LbaState *h_state, int *counters)
{
    gba_carve(G, (uint8_t *)workspace);
    const LbaWs &W = G.L;
    const dim3 one(1), items(kItemBlocks), it(kItem), big(kBig), team(kLbaTeam);
    int syncs = 0, launches = 0;
    auto read_state = [&]() -> int {
        ORBHIP_HIP_CHECK(hipGetLastError());
        ORBHIP_HIP_CHECK(hipMemcpyAsync(h_state, W.S, sizeof(LbaState), hipMemcpyDeviceToHost, stream));
        ORBHIP_HIP_CHECK(hipStreamSynchronize(stream));
        ++syncs;
        return ORBHIP_OK;
    };
    hipLaunchKernelGGL(k_gba_setup, one, big, 0, stream, G);
    hipLaunchKernelGGL(k_gba_index, items, it, 0, stream, G);
    hipLaunchKernelGGL(k_gba_covis, items, it, 0, stream, G);
    launches += 3;
    if (int rc = read_state()) return rc;
    for (int step = 0; h_state->phase != kLbaDone; ++step) {
        if (step > W.single_its * 10 + 2) { set_error("global_bundle_adjustment: the state machine did not finish"); return ORBHIP_E_HIP; }
        if (h_state->phase == kLbaBuild) {
            hipLaunchKernelGGL(k_gba_linearize, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_gba_blocks, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_gba_begin, one, team, 0, stream, W);
            launches += 3;
        }
        if (h_state->phase == kLbaBuild || h_state->phase == kLbaTrial) {
            const int n = 6 * h_state->n_free;
            hipLaunchKernelGGL(k_gba_dinv, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_gba_schur, dim3(kSchurBlocks), it, 0, stream, G);
            launches += 2;
            if (n > 0) launches += ldlt::enqueue_solve<GbaView, kGbaNb>(stream, GbaView{W}, n);
            hipLaunchKernelGGL(k_gba_x, dim3(16), it, 0, stream, W);
            hipLaunchKernelGGL(k_gba_update, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_gba_trial, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_gba_judge, one, team, 0, stream, W);
            launches += 4;
        } else {                                                               // kLbaFinal
            hipLaunchKernelGGL(k_gba_finish, one, big, 0, stream, G);
            ++launches;
        }
        if (int rc = read_state()) return rc;
    }
    if (counters) { counters[0] = syncs; counters[1] = launches; }
    return ORBHIP_OK;
}

int launch_apply_global_ba(hipStream_t stream, GbaApply A, void *workspace)
{
    gba_apply_carve(A, (uint8_t *)workspace);
    hipLaunchKernelGGL(k_gba_apply_walk, dim3(1), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k_gba_apply_points, dim3(kItemBlocks), dim3(kItem), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
