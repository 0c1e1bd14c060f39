// Essential-graph optimisation on the device: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044), include/orbhip.h
// section "essential-graph optimisation".  gfx950 only, wave64.  The arithmetic is tests/seqref/essgraph.py operation by
// operation; the items and the state machine are orbhip_essgraph_core.h, which the host replays bit
// for bit.
//
// The number of trials depends on the data, so the launch function reads the state record back once after the setup and once
// per trial (one small pinned copy, one stream synchronisation) and enqueues the next step from it: the call synchronises.
// The launches per trial depend on rows only.  No cooperative launch, no workgroup waits for another, one stream; every
// kernel reads the phase of the state record first and leaves when its step is not due.
//   k_eg_setup         one workgroup of 1024: the vertices in row order (a scan over the rows that are not bad), the first
//                      estimates, the 14 perturbations, the edges in creation order (a row's edges counted, a scan, then written,
//                      for the loop connections and again for the other three kinds), each free vertex's edges ascending
//   k_eg_eval          one 64-lane team per edge: 29 lanes, one error evaluation each (14 per free end, and the estimate)
//   k_eg_blocks        one 64-lane team per edge: the 162 elements of its record (J_i^T J_i, J_j^T J_j, J_i^T J_j, the two b, chi2)
//   k_eg_vertex        one team per free vertex: its diagonal block and b over its edges in creation order, no float atomics
//   k_eg_lm_begin      256 lanes: chi2, lambda
//   k_eg_zero, k_eg_scatter   the dense system at the current lambda: zeroed, then one team per free vertex writes its rows
//   ldlt::k_factor_diag / _panel / _trail, k_fwd_diag / _upd, k_dscale, k_bwd_diag / _upd (orbhip_ldlt.h, shared with global
//                      bundle adjustment): the unpivoted LDLt of lba_solve and its two substitutions, blocked in panels of
//                      kEgPanel poses (kEgNb = 7 kEgPanel columns) out of global memory, byte-identical to the one-thread host
//                      build whatever the panel width
//   k_eg_update, k_eg_trial, k_eg_judge   the tried estimates, chi2 at them, the Levenberg-Marquardt decision
//   k_eg_finish        one workgroup of 1024: the poses, the list of present points (a scan) and their correction, the report
#include "orbhip_internal.h"
#include "orbhip_ldlt.h"
#include "orbhip_team_dev.h"

namespace orbhip {
namespace {

constexpr int kBig = 1024, kItem = 256, kItemBlocks = 240, kNb = kEgNb;

// exclusive scan of v over the 1024 lanes of the workgroup; *total = the sum.  s_w [16].
__device__ __forceinline__ int eg_block_scan(int v, int *s_w, int *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int incl = wave_incl_scan_add(v);
    __syncthreads();
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < kBig / 64; ++w) {
        if (w < wv) off += s_w[w];
        all += s_w[w];
    }
    *total = all;
    return off + incl - v;
}

__device__ __forceinline__ int eg_free_vtx(const EgState &S, int f) { return (S.loop_vtx >= 0 && f >= S.loop_vtx) ? f + 1 : f; }

__global__ __launch_bounds__(kBig) void k_eg_setup(EgWs W)
{
    __shared__ int s_w[kBig / 64];
    __shared__ int s_cnt[kEgCnts + 1];
    const int tid = threadIdx.x;
    EgState &S = *W.S;
    if (tid <= kEgCnts) s_cnt[tid] = 0;
    int nv = 0;
    for (int base = 0; base < W.rows; base += kBig) {
        const int r = base + tid;
        const bool good = r < W.rows && !eg_bad(W, r);
        int all;
        const int pos = nv + eg_block_scan(good ? 1 : 0, s_w, &all);
        if (r < W.rows) W.row_vtx[r] = good && pos < kEgMaxKf ? pos : -1;
        if (good && pos < kEgMaxKf) W.vtx_row[pos] = r;
        nv += all;
    }
    __syncthreads();
    if (nv > kEgMaxKf) {
        if (tid == 0) {
            memset(&S, 0, sizeof(S));
            S.nv = nv; S.loop_vtx = -1; S.status = ORBHIP_EG_CAPACITY;
            eg_begin(W);
        }
        return;
    }
    const int lv = W.row_vtx[W.loop_row], nf = lv >= 0 ? nv - 1 : nv;
    for (int v = tid; v < nv; v += kBig) {
        W.vtx_free[v] = v == lv ? -1 : (lv >= 0 && v > lv ? v - 1 : v);
        eg_vertex_init(W, v);
    }
    if (tid < 14) eg_perturb_init(W, tid);
    for (int t = tid; t < 7 * nf; t += kBig) W.xp[t] = 0.0;
    __syncthreads();
    // the edges: per pass, a row's edges counted, a scan over the rows, then written from the row's start
    int ne = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int base = 0; base < W.rows; base += kBig) {
            const int r = base + tid;
            int c = 0, cnt[kEgCnts + 1];
#pragma unroll
            for (int k = 0; k <= kEgCnts; ++k) cnt[k] = 0;
            if (r < W.rows) c = eg_row_edges(W, r, pass, 0, false, cnt);
#pragma unroll
            for (int k = 0; k < kEgCnts; ++k)
                if (cnt[k]) atomicAdd(&s_cnt[k], cnt[k]);
            int all;
            const int off = ne + eg_block_scan(c, s_w, &all);
            if (r < W.rows) W.row_e0[pass * (W.rows + 1) + r] = off;
            ne += all;
        }
    __syncthreads();
    if (ne > W.max_edges) {
        if (tid == 0) {
            memset(&S, 0, sizeof(S));
            S.nv = nv; S.n_free = nf; S.n = 7 * nf; S.n_edges = ne; S.loop_vtx = lv; S.status = ORBHIP_EG_CAPACITY;
            for (int k = 0; k < kEgCnts; ++k) S.cnt[k] = s_cnt[k];
            eg_begin(W);
        }
        return;
    }
    for (int pass = 0; pass < 2; ++pass)
        for (int r = tid; r < W.rows; r += kBig) eg_row_edges(W, r, pass, W.row_e0[pass * (W.rows + 1) + r], true, nullptr);
    __syncthreads();
    // each free vertex's edges, ascending (nv <= kEgMaxKf <= 1024: one lane per vertex)
    {
        const int v = tid;
        const bool mine = v < nv && v != lv;
        int c = 0;
        if (mine)
            for (int e = 0; e < ne; ++e) c += (W.e_i[e] == v || W.e_j[e] == v) ? 1 : 0;
        int all;
        int k = eg_block_scan(c, s_w, &all);
        if (mine) {
            W.vf_e0[W.vtx_free[v]] = k;
            for (int e = 0; e < ne; ++e)
                if (W.e_i[e] == v || W.e_j[e] == v) W.vf_edges[k++] = e;
        }
        if (tid == 0) W.vf_e0[nf] = all;
    }
    __syncthreads();
    if (tid == 0) {
        memset(&S, 0, sizeof(S));
        S.nv = nv; S.n_free = nf; S.n = 7 * nf; S.n_edges = ne; S.loop_vtx = lv;
        for (int k = 0; k < kEgCnts; ++k) S.cnt[k] = s_cnt[k];
        eg_begin(W);
    }
}

// ---- a linearisation ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kItem) void k_eg_eval(EgWs W)
{
    if (W.S->phase != kEgBuild) return;
    const int lane = threadIdx.x & 63, ne = W.S->n_edges, teams = gridDim.x * (kItem / 64);
    if (lane >= kEgEvals) return;
    for (int e = blockIdx.x * (kItem / 64) + (threadIdx.x >> 6); e < ne; e += teams) eg_edge_eval(W, e, lane);
}

__global__ __launch_bounds__(kItem) void k_eg_blocks(EgWs W)
{
    if (W.S->phase != kEgBuild) return;
    const int lane = threadIdx.x & 63, ne = W.S->n_edges, teams = gridDim.x * (kItem / 64);
    for (int e = blockIdx.x * (kItem / 64) + (threadIdx.x >> 6); e < ne; e += teams)
        for (int t = lane; t < kEgRec; t += 64) eg_edge_block(W, e, t);
}

__global__ __launch_bounds__(kItem) void k_eg_vertex(EgWs W)
{
    if (W.S->phase != kEgBuild) return;
    const int lane = threadIdx.x & 63, nf = W.S->n_free, teams = gridDim.x * (kItem / 64);
    if (lane >= 56) return;
    for (int f = blockIdx.x * (kItem / 64) + (threadIdx.x >> 6); f < nf; f += teams) eg_vertex_block(W, f, eg_free_vtx(*W.S, f), lane);
}

// a team sum by a workgroup of kEgTeam lanes; s_part [kEgTeam / kEgWave]
__device__ __forceinline__ double team_sum(const EgWs &W, int kind, double *s_part)
{
    return team_reduce<kEgTeam>(eg_sum_lane(W, kind, threadIdx.x), TeamAdd(), s_part);
}

__global__ __launch_bounds__(kEgTeam) void k_eg_lm_begin(EgWs W)
{
    __shared__ double s_part[kEgTeam / kEgWave];
    if (W.S->phase != kEgBuild) return;
    const double chi = team_sum(W, kEgSumLin, s_part);
    __syncthreads();
    if (threadIdx.x == 0) eg_lm_begin(W, chi);
}

// ---- a trial: the system ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kItem) void k_eg_zero(EgWs W)
{
    if (W.S->phase != kEgTrial) return;
    const size_t nn = (size_t)W.S->n * W.S->n, step = (size_t)gridDim.x * kItem;
    for (size_t k = (size_t)blockIdx.x * kItem + threadIdx.x; k < nn; k += step) W.A[k] = 0.0;
}

__global__ __launch_bounds__(kItem) void k_eg_scatter(EgWs W)
{
    if (W.S->phase != kEgTrial) return;
    const int lane = threadIdx.x & 63, nf = W.S->n_free, teams = gridDim.x * (kItem / 64);
    if (lane >= 56) return;
    for (int f = blockIdx.x * (kItem / 64) + (threadIdx.x >> 6); f < nf; f += teams) eg_vertex_scatter(W, f, eg_free_vtx(*W.S, f), lane);
}

// ---- the factorisation and the substitutions: orbhip_ldlt.h over this view of the system -------------------------------------------
struct EgView {
    EgWs W;
    __device__ __forceinline__ double *A() const { return W.A; }
    __device__ __forceinline__ double *y() const { return W.y; }
    __device__ __forceinline__ int n() const { return W.S->n; }
    __device__ __forceinline__ bool due() const { return W.S->phase == kEgTrial && !W.S->fail; }
    __device__ __forceinline__ void fail() const { W.S->fail = 1; }
};

// ---- the rest of a trial ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kItem) void k_eg_update(EgWs W)
{
    if (W.S->phase != kEgTrial) return;
    const int nv = W.S->nv;
    const bool ok = !W.S->fail;
    for (int v = blockIdx.x * kItem + threadIdx.x; v < nv; v += gridDim.x * kItem) {
        const int f = W.vtx_free[v];
        if (ok && f >= 0)
            for (int k = 0; k < 7; ++k) W.xp[7 * f + k] = W.y[7 * f + k];      // a failed factorisation leaves the stale x
        eg_vertex_update(W, v);
    }
}

__global__ __launch_bounds__(kItem) void k_eg_trial(EgWs W)
{
    if (W.S->phase != kEgTrial) return;
    const int ne = W.S->n_edges;
    for (int e = blockIdx.x * kItem + threadIdx.x; e < ne; e += gridDim.x * kItem) eg_trial_chi(W, e);
}

__global__ __launch_bounds__(kEgTeam) void k_eg_judge(EgWs W)
{
    __shared__ double s_part[kEgTeam / kEgWave];
    if (W.S->phase != kEgTrial) return;
    const double chi = team_sum(W, kEgSumTrial, s_part);
    const double scale = team_sum(W, kEgSumScale, s_part);
    __syncthreads();
    if (threadIdx.x == 0) {
        W.S->ok2 = W.S->fail ? 0 : 1;
        eg_lm_judge(W, chi, scale);
    }
}

__global__ __launch_bounds__(kBig) void k_eg_finish(EgWs W)
{
    __shared__ int s_w[kBig / 64];
    if (W.S->phase != kEgFinal) return;
    const int tid = threadIdx.x;
    EgState &S = *W.S;
    int np = 0;
    if (S.status != ORBHIP_EG_CAPACITY) {
        for (int v = tid; v < S.nv; v += kBig) eg_write_pose(W, v);
        for (int base = 0; base < W.pcap; base += kBig) {
            const int p = base + tid;
            const bool present = p < W.pcap && (W.flags[p] & ORBHIP_POINT_PRESENT);
            int all;
            const int pos = np + eg_block_scan(present ? 1 : 0, s_w, &all);
            if (present) { W.o_point_list[pos] = p; eg_write_point(W, p); }
            np += all;
        }
    }
    __syncthreads();
    if (tid == 0) {
        S.n_pts = np;
        eg_write_report(W);
        S.phase = kEgDone;
    }
}

}  // namespace

size_t eg_workspace_bytes(EgWs W) { return eg_carve(W, nullptr); }

// h_state: a pinned EgState the call reads the device's record into; counters[2], nullable, receives the synchronisations and
// the launches of the call
int launch_optimize_essential_graph(hipStream_t stream, EgWs W, void *workspace, EgState *h_state, int *counters)
{
    eg_carve(W, (uint8_t *)workspace);
    const dim3 one(1), items(kItemBlocks), it(kItem), big(kBig), team(kEgTeam);
    const int nmax = 7 * eg_mk(W);
    int syncs = 0, launches = 0;
    auto read_state = [&]() -> int {
        ORBHIP_HIP_CHECK(hipGetLastError());
        ORBHIP_HIP_CHECK(hipMemcpyAsync(h_state, W.S, sizeof(EgState), hipMemcpyDeviceToHost, stream));
        ORBHIP_HIP_CHECK(hipStreamSynchronize(stream));
        ++syncs;
        return ORBHIP_OK;
    };
    hipLaunchKernelGGL(k_eg_setup, one, big, 0, stream, W);
    ++launches;
    if (int rc = read_state()) return rc;
    for (int step = 0; h_state->phase != kEgDone; ++step) {
        if (step > 20 * 10 + 2) { set_error("optimize_essential_graph: the state machine did not finish"); return ORBHIP_E_HIP; }
        if (h_state->phase == kEgBuild) {
            hipLaunchKernelGGL(k_eg_eval, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_eg_blocks, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_eg_vertex, dim3((eg_mk(W) + 3) / 4), it, 0, stream, W);
            hipLaunchKernelGGL(k_eg_lm_begin, one, team, 0, stream, W);
            launches += 4;
        }
        if (h_state->phase == kEgBuild || h_state->phase == kEgTrial) {
            hipLaunchKernelGGL(k_eg_zero, dim3(1024), it, 0, stream, W);
            hipLaunchKernelGGL(k_eg_scatter, dim3((eg_mk(W) + 3) / 4), it, 0, stream, W);
            launches += ldlt::enqueue_solve<EgView, kNb>(stream, EgView{W}, nmax);
            hipLaunchKernelGGL(k_eg_update, dim3(4), it, 0, stream, W);
            hipLaunchKernelGGL(k_eg_trial, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_eg_judge, one, team, 0, stream, W);
            launches += 5;
        } else {                                                               // kEgFinal
            hipLaunchKernelGGL(k_eg_finish, one, big, 0, stream, W);
            ++launches;
        }
        if (int rc = read_state()) return rc;
    }
    if (counters) { counters[0] = syncs; counters[1] = launches; }
    return ORBHIP_OK;
}

}  // namespace orbhip
