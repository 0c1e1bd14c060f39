// Wavefront-level pieces of the bundle-adjustment kernels, shared by orbhip_lba.hip and orbhip_gba.hip: the xor butterfly,
// the 256-lane team sums and the Schur block of a pair of free poses with its lane-dealt store.  Device only; the arithmetic
// is orbhip_lba_core.h's (lba_schur_lane, lba_sum_lane), these are its combines.
#pragma once
#include "orbhip_lba_core.h"

namespace orbhip {
namespace lbadev {

// the xor butterfly of N sums over a wavefront
template <int N> __device__ __forceinline__ void wave_butterfly(double *s)
{
#pragma unroll
    for (int off = 1; off < kLbaWave; off <<= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = s[k] + __shfl_xor(s[k], off);
    }
}

// a team sum by a workgroup of kLbaTeam lanes; s_part [kLbaTeam / kLbaWave]
__device__ __forceinline__ double team_sum(const LbaWs &W, int kind, double *s_part)
{
    const int tid = threadIdx.x;
    double v = lba_sum_lane(W, kind, tid);
#pragma unroll
    for (int off = 1; off < kLbaWave; off <<= 1) v = lba_sum_op(kind, v, __shfl_xor(v, off));
    __syncthreads();
    if ((tid & 63) == 0) s_part[tid >> 6] = v;
    __syncthreads();
    double t = s_part[0];
#pragma unroll
    for (int w = 1; w < kLbaTeam / kLbaWave; ++w) t = lba_sum_op(kind, t, s_part[w]);
    return t;
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
        wave_butterfly<42>(acc);
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
