// Local bundle adjustment on the device: Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778), include/orbhip.h
// section "local bundle adjustment".  gfx950 only, wave64.  The arithmetic is tests/seqref/lba.py operation by operation
// (DESIGN.md section 3); the items and the state machine are orbhip_lba_core.h, which the host replays bit for bit.
//
// A fixed sequence of phase kernels on the caller's stream, enqueued without looking at any result: the setup, then for 5
// and for 10 outer iterations {linearise, blocks, begin, 10 x {Dinv, Schur, solve, update, trial errors, judge}}, the
// level-1 rule between the rounds and the epilogue.  Every kernel reads the phase of the state record first and leaves
// when its step is not due.  No cooperative launch, no workgroup waits for another, every loop has a bound known when the
// kernel starts.  The grids are fixed and small, items are dealt out by grid-stride loops; the geometry enters no sum.
//   k_lba_setup        one workgroup of 1024: the three lists as ordered first occurrences (atomicMin of the order key, then
//                      a scan over the keys), the edges in creation order, the edge index of each free pose (one wavefront
//                      per pose, ballot compaction, ascending), the first estimates
//   k_lba_linearize    per edge: error, Jacobians, the edge record (its terms of Hll, b_l, Hpp, b_p, and B)
//   k_lba_blocks       per point: Hll, b_l over its contiguous edges; one wavefront per free pose: Hpp, b_p
//   k_lba_begin        256 lanes: robust chi2, largest diagonal, lambda
//   k_lba_dinv         per point: (Hll + lambda)^-1, Dinv b_l
//   k_lba_schur        one wavefront per pair (i1 <= i2) of free poses: the block of S and, on the diagonal, of b
//   k_lba_solve        one workgroup of 1024: unpivoted LDLt of S in global memory, the two substitutions
//   k_lba_update       per point: x_l and the tried point; per vertex: the tried pose
//   k_lba_trial        per edge: error at the tried estimate
//   k_lba_judge        256 lanes: robust chi2, computeScale, the Levenberg-Marquardt decision
//   k_lba_classify, k_lba_round2, k_lba_final_edges, k_lba_finish: the level-1 rule, the second round's system, the
//                      erase rows (monocular, then stereo, by two scans), the write-back and the report
#include "orbhip_internal.h"
#include "orbhip_lba_dev.h"

namespace orbhip {
namespace {
using namespace lbadev;

constexpr int kSetupThreads = 1024, kItemThreads = 256, kItemBlocks = 120, kPoseBlocks = kLbaMaxLocal / 4, kSchurBlocks = 256;
constexpr int kIntMax = 0x7fffffff;

__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kSetupThreads) void k_lba_setup(LbaWs W)
{
    __shared__ int s_w[kSetupThreads / 64];
    __shared__ int s_i[8];
    __shared__ int s_cnt[kLbaMaxLocal + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    LbaState &S = *W.S;
    for (int r = tid; r < W.rows; r += kSetupThreads) { W.kf_stamp[r] = 0; W.kf_vtx[r] = -1; W.vtx_free[r] = -1; W.kf_key[r] = kIntMax; }
    for (int p = tid; p < W.pcap; p += kSetupThreads) W.pt_key[p] = kIntMax;
    for (int k = tid; k < 6 * kLbaMaxLocal; k += kSetupThreads) W.xp[k] = 0.0;
    if (tid <= kLbaMaxLocal) s_cnt[tid] = 0;
    if (tid < 8) s_i[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        // lLocalKeyFrames (:456-468): the current key frame, then its covisible key frames that are not bad
        int nl = 0;
        W.lkf[nl++] = W.cur; W.kf_stamp[W.cur] = 1;
        const int no = min(max(W.n_ord[W.cur], 0), W.rows);
        for (int i = 0; i < no; ++i) {
            const int r = W.ord_kf[(size_t)W.cur * W.rows + i];
            if (r < 0 || r >= W.rows || W.kf_stamp[r]) continue;
            W.kf_stamp[r] = 1;
            if (!(W.kf_bad && W.kf_bad[r])) W.lkf[nl++] = r;
        }
        int nfree = 0;
        for (int li = 0; li < nl; ++li) {
            const int r = W.lkf[li];
            W.kf_vtx[r] = li; W.vtx_row[li] = r;
            W.vtx_free[li] = r == W.id0_row ? -1 : nfree++;
        }
        s_i[0] = nl; s_i[1] = nfree;
    }
    __syncthreads();
    const int nl = s_i[0], nfree = s_i[1];
    // lLocalMapPoints (:470-486): a point at its first occurrence over (list position, slot)
    const int K = nl * W.cap;
    for (int key = tid; key < K; key += kSetupThreads) {
        const int li = key / W.cap, s = key - li * W.cap, r = W.lkf[li];
        if (s >= W.n[r]) continue;
        const int p = W.slot_point[(size_t)r * W.cap + s];
        if (p >= 0 && p < W.np && (W.flags[p] & ORBHIP_POINT_PRESENT)) atomicMin(&W.pt_key[p], key);
    }
    __syncthreads();
    int npts = 0;
    for (int base = 0; base < K; base += kSetupThreads) {
        const int key = base + tid;
        int p = -1;
        bool first = false;
        if (key < K) {
            const int li = key / W.cap, s = key - li * W.cap, r = W.lkf[li];
            if (s < W.n[r]) {
                p = W.slot_point[(size_t)r * W.cap + s];
                first = p >= 0 && p < W.np && (W.flags[p] & ORBHIP_POINT_PRESENT) && ld_agent(&W.pt_key[p]) == key;
            }
        }
        int all;
        const int pos = npts + block_excl_scan<kSetupThreads>(first ? 1 : 0, s_w, &all);
        if (first && pos < W.max_points) W.lpt[pos] = p;
        npts += all;
    }
    if (nfree > kLbaMaxLocal || npts > W.max_points) {
        if (tid == 0) {
            memset(&S, 0, sizeof(S));
            S.n_lkf = nl; S.n_free = nfree; S.n_pts = npts; S.status = ORBHIP_LBA_CAPACITY;
            lba_begin(W);
        }
        return;
    }
    __syncthreads();
    // lFixedCameras (:488-504): a key frame at its first occurrence over (point, observation)
    int ncand = 0;
    for (int base = 0; base < npts; base += kSetupThreads) {
        const int i = base + tid;
        int c = 0;
        if (i < npts) { const int p = W.lpt[i]; c = max(W.obs_start[p + 1] - W.obs_start[p], 0); }
        int all;
        const int off = ncand + block_excl_scan<kSetupThreads>(c, s_w, &all);
        if (i < npts) W.pt_c0[i] = off;
        ncand += all;
    }
    __syncthreads();
    for (int i = tid; i < npts; i += kSetupThreads) {
        const int p = W.lpt[i], o0 = W.obs_start[p], o1 = W.obs_start[p + 1];
        for (int o = o0; o < o1; ++o) {
            const int r = W.obs_kf[o];
            if (r >= 0 && r < W.rows && W.kf_stamp[r] == 0) atomicMin(&W.kf_key[r], W.pt_c0[i] + (o - o0));
        }
    }
    __syncthreads();
    for (int r = tid; r < W.rows; r += kSetupThreads) {
        const int key = ld_agent(&W.kf_key[r]);
        if (key == kIntMax || (W.kf_bad && W.kf_bad[r])) continue;
        int rank = 0;
        for (int r2 = 0; r2 < W.rows; ++r2) {
            const int k2 = ld_agent(&W.kf_key[r2]);
            if (k2 < key && !(W.kf_bad && W.kf_bad[r2])) ++rank;
        }
        W.fkf[rank] = r; W.kf_vtx[r] = nl + rank; W.vtx_row[nl + rank] = r; W.vtx_free[nl + rank] = -1;
        atomicAdd(&s_i[2], 1);
    }
    __syncthreads();
    const int nf = s_i[2];
    // the edges (:572-653): every observation of a local point whose key frame is not bad, in creation order
    int ne = 0;
    for (int base = 0; base < npts; base += kSetupThreads) {
        const int i = base + tid;
        int c = 0, ns = 0;
        if (i < npts) {
            const int p = W.lpt[i];
            for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
                const int r = W.obs_kf[o];
                if (r < 0 || r >= W.rows || (W.kf_bad && W.kf_bad[r]) || W.kf_vtx[r] < 0) continue;
                ++c;
                if (W.u_right && !(W.u_right[(size_t)r * W.cap + W.obs_idx[o]] < 0)) ++ns;
            }
        }
        int all;
        const int off = ne + block_excl_scan<kSetupThreads>(c, s_w, &all);
        if (i < npts) W.pt_e0[i] = min(off, W.max_edges);
        if (ns) atomicAdd(&s_i[3], ns);
        ne += all;
    }
    __syncthreads();
    const int n_stereo = s_i[3];
    if (ne > W.max_edges) {
        if (tid == 0) {
            memset(&S, 0, sizeof(S));
            S.n_lkf = nl; S.n_free = nfree; S.n_pts = npts; S.n_fkf = nf; S.n_edges = ne; S.n_stereo = n_stereo; S.n_mono = ne - n_stereo;
            S.status = ORBHIP_LBA_CAPACITY;
            lba_begin(W);
        }
        return;
    }
    if (tid == 0) W.pt_e0[npts] = ne;
    for (int i = tid; i < npts; i += kSetupThreads) {
        const int p = W.lpt[i];
        int j = W.pt_e0[i];
        for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
            const int r = W.obs_kf[o];
            if (r < 0 || r >= W.rows || (W.kf_bad && W.kf_bad[r]) || W.kf_vtx[r] < 0) continue;
            const int idx = W.obs_idx[o];
            const bool stereo = W.u_right && !(W.u_right[(size_t)r * W.cap + idx] < 0);
            const int v = W.kf_vtx[r];
            W.e_vtx[j] = v; W.e_idx[j] = idx; W.e_pt[j] = i; W.e_fl[j] = stereo ? kLbaStereo : 0;
            W.eb[(size_t)j * kLbaRec + kLbaChi2] = 0.0;
            const int f = W.vtx_free[v];
            if (f >= 0) atomicAdd(&s_cnt[f + 1], 1);
            ++j;
        }
        W.pt_active[i] = j > W.pt_e0[i] ? 1 : 0;
        for (int k = 0; k < 3; ++k) {
            const double x = (double)W.world[(size_t)p * 3 + k];
            W.pt[lba_pt_at(W, 0, i) + k] = x; W.pt[lba_pt_at(W, 1, i) + k] = x;
            W.xl[(size_t)i * 3 + k] = 0.0;
        }
    }
    for (int v = tid; v < nl + nf; v += kSetupThreads) {
        double q[7];
        po_pose_from_Tcw(W.Tcw + (size_t)W.vtx_row[v] * 12, q);
#pragma unroll
        for (int k = 0; k < 7; ++k) { W.pose[lba_pose_at(W, 0, v) + k] = q[k]; W.pose[lba_pose_at(W, 1, v) + k] = q[k]; }
    }
    __syncthreads();
    if (tid == 0) {
        int poses = 0;
        for (int f = 0; f < nfree; ++f) { W.pose_active[f] = s_cnt[f + 1] > 0 ? 1 : 0; poses += W.pose_active[f]; s_cnt[f + 1] += s_cnt[f]; }
        for (int f = 0; f <= nfree; ++f) W.kf_e0[f] = s_cnt[f];
        s_i[4] = poses;
    }
    __syncthreads();
    // the edge index of each free pose, ascending: one wavefront per pose over all edges
    for (int f = wv; f < nfree; f += kSetupThreads / 64) {
        int base = s_cnt[f];
        for (int j0 = 0; j0 < ne; j0 += 64) {
            const int j = j0 + lane;
            const bool mine = j < ne && W.vtx_free[W.e_vtx[j]] == f;
            const unsigned long long mask = __ballot(mine);
            if (mine) W.kf_edges[base + lane_prefix(mask)] = j;
            base += __popcll(mask);
        }
    }
    __syncthreads();
    if (tid == 0) {
        memset(&S, 0, sizeof(S));
        S.n_lkf = nl; S.n_free = nfree; S.n_pts = npts; S.n_fkf = nf; S.n_edges = ne; S.n_stereo = n_stereo; S.n_mono = ne - n_stereo;
        S.n_active = ne; S.poses[0] = s_i[4];
        lba_begin(W);
    }
}

__global__ __launch_bounds__(kItemThreads) void k_lba_linearize(LbaWs W)
{
    if (W.S->phase == kLbaBuild) phase_linearize<kItemThreads>(W);
}

__global__ __launch_bounds__(kItemThreads) void k_lba_blocks(LbaWs W)
{
    if (W.S->phase != kLbaBuild) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (blockIdx.x < kPoseBlocks) {
        const int f = blockIdx.x * 4 + wv;
        if (f < W.S->n_free) pose_block(W, f, lane);
        return;
    }
    const int np = W.S->n_pts, nb = gridDim.x - kPoseBlocks;
    for (int i = (blockIdx.x - kPoseBlocks) * kItemThreads + tid; i < np; i += nb * kItemThreads) lba_point_block(W, i);
}

__global__ __launch_bounds__(kLbaTeam) void k_lba_begin(LbaWs W)
{
    __shared__ double s_part[kLbaTeam / kLbaWave];
    if (W.S->phase == kLbaBuild) phase_lm_begin(W, s_part);
}

__global__ __launch_bounds__(kItemThreads) void k_lba_dinv(LbaWs W)
{
    if (W.S->phase == kLbaTrial) phase_dinv<kItemThreads>(W);
}

__global__ __launch_bounds__(kItemThreads) void k_lba_schur(LbaWs W)
{
    if (W.S->phase != kLbaTrial) return;
    const int tid = threadIdx.x, lane = tid & 63, nfree = W.S->n_free;
    const int waves = gridDim.x * (kItemThreads / 64);
    for (int t = blockIdx.x * (kItemThreads / 64) + (tid >> 6); t < nfree * nfree; t += waves) {
        const int i1 = t / nfree, i2 = t - i1 * nfree;
        if (i2 < i1) continue;
        schur_pair(W, i1, i2, lane, true);
    }
}

struct LbaDevTeam {
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int size() const { return kSetupThreads; }
    __device__ __forceinline__ int wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ int waves() const { return kSetupThreads / 64; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(kSetupThreads) void k_lba_solve(LbaWs W)
{
    if (W.S->phase != kLbaTrial) return;
    LbaDevTeam tm;
    const bool ok = lba_solve(tm, W);
    if (threadIdx.x == 0) W.S->ok2 = ok ? 1 : 0;
}

__global__ __launch_bounds__(kItemThreads) void k_lba_update(LbaWs W)
{
    if (W.S->phase == kLbaTrial) phase_update<kItemThreads>(W);
}

__global__ __launch_bounds__(kItemThreads) void k_lba_trial(LbaWs W)
{
    if (W.S->phase == kLbaTrial) phase_trial<kItemThreads>(W);
}

__global__ __launch_bounds__(kLbaTeam) void k_lba_judge(LbaWs W)
{
    __shared__ double s_part[kLbaTeam / kLbaWave];
    if (W.S->phase == kLbaTrial) phase_lm_judge(W, s_part);
}

__global__ __launch_bounds__(kItemThreads) void k_lba_classify(LbaWs W)
{
    if (W.S->phase != kLbaClassify) return;
    const int ne = W.S->n_edges;
    for (int j = blockIdx.x * kItemThreads + threadIdx.x; j < ne; j += gridDim.x * kItemThreads)
        if (lba_edge_bad(W, j)) { W.e_fl[j] = W.e_fl[j] | kLbaLevel1; atomicAdd(&W.S->n_level1, 1); }
}

__global__ __launch_bounds__(kSetupThreads) void k_lba_round2(LbaWs W)
{
    __shared__ int s_poses;
    if (W.S->phase != kLbaClassify) return;
    const int tid = threadIdx.x, np = W.S->n_pts, nfree = W.S->n_free;
    if (tid == 0) s_poses = 0;
    __syncthreads();
    for (int k = tid; k < 6 * nfree; k += kSetupThreads) W.xp[k] = 0.0;
    for (int k = tid; k < 3 * np; k += kSetupThreads) W.xl[k] = 0.0;
    for (int i = tid; i < np; i += kSetupThreads) {
        uint8_t act = 0;
        for (int j = W.pt_e0[i]; j < W.pt_e0[i + 1]; ++j) if (!(W.e_fl[j] & kLbaLevel1)) act = 1;
        W.pt_active[i] = act;
    }
    for (int f = tid; f < nfree; f += kSetupThreads) {
        uint8_t act = 0;
        for (int k = W.kf_e0[f]; k < W.kf_e0[f + 1]; ++k) if (!(W.e_fl[W.kf_edges[k]] & kLbaLevel1)) act = 1;
        W.pose_active[f] = act;
        if (act) atomicAdd(&s_poses, 1);
    }
    __syncthreads();
    if (tid == 0) {
        W.S->poses[1] = s_poses;
        W.S->n_active = W.S->n_edges - ld_agent(&W.S->n_level1);
        lba_round_begin(W, 1);
    }
}

__global__ __launch_bounds__(kItemThreads) void k_lba_final_edges(LbaWs W)
{
    if (W.S->phase != kLbaFinal || !lba_writes(*W.S)) return;
    const int ne = W.S->n_edges;
    for (int j = blockIdx.x * kItemThreads + threadIdx.x; j < ne; j += gridDim.x * kItemThreads) W.e_erase[j] = lba_edge_bad(W, j) ? 1 : 0;
}

__global__ __launch_bounds__(kSetupThreads) void k_lba_finish(LbaWs W)
{
    __shared__ int s_w[kSetupThreads / 64];
    if (W.S->phase != kLbaFinal) return;
    const int tid = threadIdx.x;
    LbaState &S = *W.S;
    int nerase = 0;
    if (lba_writes(S)) {
        const int ne = S.n_edges;
        for (int pass = 0; pass < 2; ++pass)                                     // vToErase: monocular edges, then stereo edges
            for (int base = 0; base < ne; base += kSetupThreads) {
                const int j = base + tid;
                const bool hit = j < ne && W.e_erase[j] && ((W.e_fl[j] & kLbaStereo) != 0) == (pass == 1);
                int all;
                const int pos = nerase + block_excl_scan<kSetupThreads>(hit ? 1 : 0, s_w, &all);
                if (hit) {
                    W.o_erase[(size_t)pos * 3] = W.vtx_row[W.e_vtx[j]]; W.o_erase[(size_t)pos * 3 + 1] = W.e_idx[j];
                    W.o_erase[(size_t)pos * 3 + 2] = W.lpt[W.e_pt[j]];
                }
                nerase += all;
            }
        for (int li = tid; li < S.n_lkf; li += kSetupThreads) { W.o_local_kf[li] = W.lkf[li]; lba_write_pose(W, li); }
        for (int k = tid; k < S.n_fkf; k += kSetupThreads) W.o_fixed_kf[k] = W.fkf[k];
        for (int i = tid; i < S.n_pts; i += kSetupThreads) { W.o_local_point[i] = W.lpt[i]; lba_write_point(W, i); }
    }
    __syncthreads();
    if (tid == 0) {
        S.n_erase = nerase;
        lba_write_report(W);
        S.phase = kLbaDone;
    }
}

}  // namespace

size_t lba_workspace_bytes(LbaWs W) { return lba_carve(W, nullptr); }

int launch_local_bundle_adjustment(hipStream_t stream, LbaWs W, void *workspace)
{
    lba_carve(W, (uint8_t *)workspace);
    const dim3 one(1), items(kItemBlocks), it(kItemThreads), big(kSetupThreads), team(kLbaTeam);
    hipLaunchKernelGGL(k_lba_setup, one, big, 0, stream, W);
    for (int round = 0; round < 2; ++round) {
        for (int i = 0; i < (round == 0 ? 5 : 10); ++i) {
            hipLaunchKernelGGL(k_lba_linearize, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_lba_blocks, dim3(kPoseBlocks + kItemBlocks), it, 0, stream, W);
            hipLaunchKernelGGL(k_lba_begin, one, team, 0, stream, W);
            for (int q = 0; q < 10; ++q) {
                hipLaunchKernelGGL(k_lba_dinv, items, it, 0, stream, W);
                hipLaunchKernelGGL(k_lba_schur, dim3(kSchurBlocks), it, 0, stream, W);
                hipLaunchKernelGGL(k_lba_solve, one, big, 0, stream, W);
                hipLaunchKernelGGL(k_lba_update, items, it, 0, stream, W);
                hipLaunchKernelGGL(k_lba_trial, items, it, 0, stream, W);
                hipLaunchKernelGGL(k_lba_judge, one, team, 0, stream, W);
            }
        }
        if (round == 0) {
            hipLaunchKernelGGL(k_lba_classify, items, it, 0, stream, W);
            hipLaunchKernelGGL(k_lba_round2, one, big, 0, stream, W);
        }
    }
    hipLaunchKernelGGL(k_lba_final_edges, items, it, 0, stream, W);
    hipLaunchKernelGGL(k_lba_finish, one, big, 0, stream, W);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
