// The device form of the optimisers' team sums and of the team itself; orbhip_lm_core.h's host_team_combine replays these
// bit for bit.  Device only, wave64.  A team sum is an xor butterfly over each wavefront (offsets 1 .. 32), lane 0 of each
// wavefront writing its sum to LDS, a barrier, and every lane combining the wavefront sums in wavefront order.
#pragma once
#include "orbhip_common.h"
#include "orbhip_lm_core.h"

namespace orbhip {

// the xor butterfly of the sums N0 .. N - 1 over a wavefront
template <int N0, int N> __device__ __forceinline__ void wave_butterfly(double *s)
{
#pragma unroll
    for (int off = 1; off < kTeamWave; off <<= 1) {
#pragma unroll
        for (int k = N0; k < N; ++k) s[k] = s[k] + __shfl_xor(s[k], off);
    }
}

// The sums N0 .. N - 1 of a team of TEAM lanes, left in s on every lane; part [TEAM / 64][N].  No barrier in front of the
// write to part: the caller keeps a team sync between two calls on the same part.  A team of one wavefront is the butterfly.
template <int TEAM, int N0, int N> __device__ __forceinline__ void team_combine(double *s, double (*part)[N], int tid)
{
    wave_butterfly<N0, N>(s);
    if constexpr (TEAM > kTeamWave) {
        if ((tid & (kTeamWave - 1)) == 0) {
#pragma unroll
            for (int k = N0; k < N; ++k) part[tid / kTeamWave][k] = s[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = N0; k < N; ++k) {
            double t = part[0][k];
#pragma unroll
            for (int w = 1; w < TEAM / kTeamWave; ++w) t = t + part[w][k];
            s[k] = t;
        }
    }
}

// One value per lane of a workgroup of TEAM lanes combined by op; s_part [TEAM / 64].  Opens with a barrier, so two calls
// in a row may share s_part.
template <int TEAM, class Op> __device__ __forceinline__ double team_reduce(double v, Op op, double *s_part)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 1; off < kTeamWave; off <<= 1) v = op(v, __shfl_xor(v, off));
    __syncthreads();
    if ((tid & (kTeamWave - 1)) == 0) s_part[tid / kTeamWave] = v;
    __syncthreads();
    double t = s_part[0];
#pragma unroll
    for (int w = 1; w < TEAM / kTeamWave; ++w) t = op(t, s_part[w]);
    return t;
}

// The team a workgroup of TEAM lanes is to the shared cores: lane 0 runs the serial part, the per-item loops are dealt out
// by lane, integers are added by atomics.  An optimiser's team adds its sum<FULL>.
template <int TEAM> struct DevTeam {
    int tid;
    __device__ __forceinline__ bool is0() const { return tid == 0; }
    __device__ __forceinline__ int first() const { return tid; }
    __device__ __forceinline__ int stride() const { return TEAM; }
    __device__ __forceinline__ void sync()
    {
        if (TEAM <= kTeamWave) wave_lds_handoff(); else __syncthreads();
    }
    __device__ __forceinline__ void add(int *dst, int v)
    {
        if (v) atomicAdd(dst, v);
    }
};

}  // namespace orbhip
