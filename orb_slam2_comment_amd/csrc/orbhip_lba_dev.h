// What the kernels of orbhip_lba.hip and orbhip_gba.hip share: the phase bodies that are the same in local and in global
// bundle adjustment (a kernel of either is its phase guard and one call), the workgroup scan of the setups, the blocks of a
// free pose and the Schur block of a pair of free poses with its lane-dealt store.  Device only; the arithmetic is
// orbhip_lba_core.h's (lba_schur_lane, lba_sum_lane, ...), the combines are orbhip_team_dev.h's.
#pragma once
#include "orbhip_lba_core.h"
#include "orbhip_team_dev.h"

namespace orbhip {
namespace lbadev {

// exclusive scan of v over the THREADS lanes of the workgroup; *total = the sum.  s_w [THREADS / 64].
template <int THREADS> __device__ __forceinline__ int block_excl_scan(int v, int *s_w, int *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int incl = wave_incl_scan_add(v);
    __syncthreads();
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
        if (w < wv) off += s_w[w];
        all += s_w[w];
    }
    *total = all;
    return off + incl - v;
}

// a team sum by a workgroup of kLbaTeam lanes; s_part [kLbaTeam / kLbaWave]
__device__ __forceinline__ double team_sum(const LbaWs &W, int kind, double *s_part)
{
    return team_reduce<kLbaTeam>(lba_sum_lane(W, kind, threadIdx.x), LbaSumOp{kind}, s_part);
}

// ---- the phase bodies: grid-stride loops of THREADS-lane workgroups over the items -------------------------------------
template <int THREADS> __device__ __forceinline__ void phase_linearize(const LbaWs &W)
{
    const int ne = W.S->n_edges;
    for (int j = blockIdx.x * THREADS + threadIdx.x; j < ne; j += gridDim.x * THREADS) lba_edge_linearize(W, j);
}
template <int THREADS> __device__ __forceinline__ void phase_dinv(const LbaWs &W)
{
    const int np = W.S->n_pts;
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < np; i += gridDim.x * THREADS) lba_point_dinv(W, i);
}
// every vertex: n_fkf is 0 in global bundle adjustment
template <int THREADS> __device__ __forceinline__ void phase_update(const LbaWs &W)
{
    const int np = W.S->n_pts, nv = W.S->n_lkf + W.S->n_fkf, g = blockIdx.x * THREADS + threadIdx.x, gs = gridDim.x * THREADS;
    for (int i = g; i < np; i += gs) lba_point_update(W, i);
    for (int v = g; v < nv; v += gs) lba_vertex_update(W, v);
}
template <int THREADS> __device__ __forceinline__ void phase_trial(const LbaWs &W)
{
    const int ne = W.S->n_edges, buf = 1 - W.S->cur;
    for (int j = blockIdx.x * THREADS + threadIdx.x; j < ne; j += gridDim.x * THREADS) lba_edge_error(W, j, buf);
}
// one workgroup of kLbaTeam lanes: robust chi2, largest diagonal, lambda; s_part [kLbaTeam / kLbaWave]
__device__ __forceinline__ void phase_lm_begin(LbaWs &W, double *s_part)
{
    const double chi = team_sum(W, kLbaSumChi, s_part);
    const double mx = W.S->it == 0 ? team_sum(W, kLbaSumMax, s_part) : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) lba_lm_begin(W, chi, mx);
}
// one workgroup of kLbaTeam lanes: robust chi2, computeScale, the Levenberg-Marquardt decision
__device__ __forceinline__ void phase_lm_judge(LbaWs &W, double *s_part)
{
    const double chi = team_sum(W, kLbaSumChi, s_part);
    const double scale = team_sum(W, kLbaSumScale, s_part);
    __syncthreads();
    if (threadIdx.x == 0) lba_lm_judge(W, chi, scale);
}

// one wavefront, the free pose f: Hpp and b_p over its edges, stored by lane 0
__device__ __forceinline__ void pose_block(const LbaWs &W, int f, int lane)
{
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    lba_pose_block_lane(W, f, lane, acc);
    wave_butterfly<0, 27>(acc);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 21; ++q) W.Hpp[f * 21 + q] = acc[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) W.bp[f * 6 + q] = acc[21 + q];
    }
}

// One wavefront, the pair (i1 <= i2): the block of S and, on the diagonal, of b, stored as lba_schur_store does.  `shared`
// false says that no point is seen by both poses: every lane's part is 0.0 then and so is the sum, which is stored without
// walking the edges.
__device__ __forceinline__ void schur_pair(const LbaWs &W, int i1, int i2, int lane, bool shared)
{
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; ++k) acc[k] = 0.0;
    if (shared) {
        lba_schur_lane(W, i1, i2, lane, acc);
        wave_butterfly<0, 42>(acc);
    }
    // the store, dealt over the lanes: every lane holds the sums
    const int ld = 6 * W.S->n_free;
    const double lam = W.S->lam;
    if (i1 == i2) {
        const bool act = W.pose_active[i1] != 0;
        if (lane < 36) {
            const int a = lane / 6, b = lane - a * 6;
            if (b <= a) {
                double v = a == b ? 1.0 : 0.0, sm = 0.0;
#pragma unroll
                for (int k = 0; k < 36; ++k) if (k == b * 6 + a) sm = acc[k];
                if (act) {
                    double h = W.Hpp[i1 * 21 + lba_upper(b, a)];
                    if (a == b) h = h + lam;
                    v = h - sm;
                }
                W.A[(size_t)(6 * i1 + a) * ld + 6 * i1 + b] = v;
            }
        } else if (lane < 42) {
            const int a = lane - 36;
            double sm = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k == a) sm = acc[36 + k];
            W.bs[6 * i1 + a] = act ? W.bp[i1 * 6 + a] - sm : 0.0;
        }
    } else if (lane < 36) {
        const int a = lane / 6, b = lane - a * 6;
        double sm = 0.0;
#pragma unroll
        for (int k = 0; k < 36; ++k) if (k == lane) sm = acc[k];
        W.A[(size_t)(6 * i2 + b) * ld + 6 * i1 + a] = 0.0 - sm;
    }
}

}  // namespace lbadev
}  // namespace orbhip
