// The dense unpivoted LDLt of lba_solve (orbhip_lba_core.h), blocked in panels out of global memory, and its two
// substitutions: one text for the essential-graph optimisation (7 unknowns per vertex) and for global bundle adjustment
// (6 per pose).  Device only; included by orbhip_essgraph.hip and orbhip_gba.hip.
//
// A "system view" V is a small record passed by value with
//   __device__ double *A() const      the matrix, row-major, lower triangle in, L and D out (the upper triangle is scratch)
//   __device__ int n() const          its order; the leading dimension is n as well
//   __device__ double *y() const      the right-hand side in, the solution out
//   __device__ bool due() const       the step is due: the phase is the trial's and no pivot has failed yet
//   __device__ void fail() const      a pivot was <= 0
// NB is the panel width in columns.  Per panel p (columns c0 .. c0 + w): one workgroup factorises the diagonal block in LDS;
// workgroups of 16 rows scale the panel below it; 64 x 64 tiles of the trailing matrix take the panel's update from two LDS
// tiles.  The lower triangle receives L, the upper triangle the unscaled columns c_jk = l_jk d_k as they were before the
// division (both are needed: l_ik * c_jk).  Every element (i, j) still sees a - l_ik * c_jk for k ascending -- across panels,
// and inside a tile -- one multiply and one subtract each (ldlt_fnma), so the result does not depend on NB or on how tiles
// are dealt out and is byte-identical to one thread running lba_solve.  That rules out FMA and the fp64 MFMA instructions
// (v_mfma_f64_*): both round once where the reference order rounds twice.
#pragma once
#include <hip/hip_runtime.h>

namespace orbhip {
namespace ldlt {

constexpr int kItem = 256, kTile = 64, kPanelRows = 16;

__device__ __forceinline__ double ldlt_fnma(double a, double l, double c) { const double p = l * c; return a - p; }

struct Panel { int n, c0, w; size_t ld; bool due; };
template <class V, int NB> __device__ __forceinline__ Panel panel_of(const V &v, int p)
{
    Panel P;
    P.n = v.n(); P.ld = (size_t)P.n; P.c0 = p * NB;
    P.w = P.n - P.c0 < NB ? P.n - P.c0 : NB;
    P.due = v.due() && P.c0 < P.n;
    return P;
}

template <class V, int NB> __global__ __launch_bounds__(kItem) void k_factor_diag(V v, int p)
{
    __shared__ double sA[NB][NB + 1], sL[NB][NB + 1];
    const Panel P = panel_of<V, NB>(v, p);
    if (!P.due) return;
    const int tid = threadIdx.x, w = P.w;
    double *A = v.A();
    for (int idx = tid; idx < w * w; idx += kItem) {
        const int i = idx / w, j = idx - i * w;
        if (j <= i) sA[i][j] = A[(size_t)(P.c0 + i) * P.ld + P.c0 + j];
    }
    __syncthreads();
    for (int k = 0; k < w; ++k) {
        const double d = sA[k][k];
        if (!(d > 0)) {                                                        // uniform: every lane reads the same pivot
            if (tid == 0) v.fail();
            return;
        }
        for (int i = k + 1 + tid; i < w; i += kItem) sL[i][k] = sA[i][k] / d;
        __syncthreads();
        const int m = w - k - 1;
        for (int idx = tid; idx < m * m; idx += kItem) {
            const int i = k + 1 + idx / m, j = k + 1 + idx % m;
            if (j <= i) sA[i][j] = ldlt_fnma(sA[i][j], sL[i][k], sA[j][k]);
        }
        __syncthreads();
    }
    for (int idx = tid; idx < w * w; idx += kItem) {
        const int i = idx / w, j = idx - i * w;
        if (j == i) A[(size_t)(P.c0 + i) * P.ld + P.c0 + i] = sA[i][i];
        else if (j < i) {
            A[(size_t)(P.c0 + i) * P.ld + P.c0 + j] = sL[i][j];
            A[(size_t)(P.c0 + j) * P.ld + P.c0 + i] = sA[i][j];
        }
    }
}

// 16 rows below the diagonal block per workgroup, 16 lanes per row: column k' is divided, then the columns right of it updated
template <class V, int NB> __global__ __launch_bounds__(kItem) void k_factor_panel(V v, int p)
{
    __shared__ double sC[NB][NB + 1], sR[kPanelRows][NB + 1], sLr[kPanelRows][NB + 1], sd[NB];
    const Panel P = panel_of<V, NB>(v, p);
    const int r0 = P.c0 + P.w + blockIdx.x * kPanelRows;
    if (!P.due || r0 >= P.n) return;
    const int tid = threadIdx.x, w = P.w, tr = tid >> 4, tl = tid & 15;
    double *A = v.A();
    for (int idx = tid; idx < w * w; idx += kItem) {
        const int kp = idx / w, k = idx - kp * w;                              // c_k,k' sits in the upper triangle at (k', k)
        if (kp < k) sC[k][kp] = A[(size_t)(P.c0 + kp) * P.ld + P.c0 + k];
    }
    for (int k = tid; k < w; k += kItem) sd[k] = A[(size_t)(P.c0 + k) * P.ld + P.c0 + k];
    for (int idx = tid; idx < kPanelRows * w; idx += kItem) {
        const int r = idx / w, k = idx - r * w;
        sR[r][k] = r0 + r < P.n ? A[(size_t)(r0 + r) * P.ld + P.c0 + k] : 0.0;
    }
    __syncthreads();
    for (int kp = 0; kp < w; ++kp) {
        const double l = sR[tr][kp] / sd[kp];
        if (tl == 0) sLr[tr][kp] = l;
        for (int k = kp + 1 + tl; k < w; k += 16) sR[tr][k] = ldlt_fnma(sR[tr][k], l, sC[k][kp]);
        __syncthreads();
    }
    for (int idx = tid; idx < kPanelRows * w; idx += kItem) {
        const int r = idx / w, k = idx - r * w;
        if (r0 + r < P.n) A[(size_t)(r0 + r) * P.ld + P.c0 + k] = sLr[r][k];
    }
    for (int idx = tid; idx < kPanelRows * w; idx += kItem) {
        const int k = idx / kPanelRows, r = idx - k * kPanelRows;
        if (r0 + r < P.n) A[(size_t)(P.c0 + k) * P.ld + r0 + r] = sR[r][k];
    }
}

// a 64 x 64 tile (bi, bj), bj <= bi, of the trailing matrix: 256 lanes, 4 x 4 elements each, strided by 16 so that the LDS
// rows a wavefront reads fall on different banks
template <class V, int NB> __global__ __launch_bounds__(kItem) void k_factor_trail(V v, int p)
{
    __shared__ double sL[kTile][NB + 1], sC[kTile][NB + 1];
    const Panel P = panel_of<V, NB>(v, p);
    const int c1 = P.c0 + P.w, i0 = c1 + blockIdx.y * kTile, j0 = c1 + blockIdx.x * kTile;
    if (!P.due || blockIdx.x > blockIdx.y || i0 >= P.n) return;
    const int tid = threadIdx.x, w = P.w, tx = tid & 15, ty = tid >> 4;
    double *A = v.A();
    for (int idx = tid; idx < kTile * w; idx += kItem) {
        const int r = idx / w, k = idx - r * w;
        sL[r][k] = i0 + r < P.n ? A[(size_t)(i0 + r) * P.ld + P.c0 + k] : 0.0;
    }
    for (int idx = tid; idx < kTile * w; idx += kItem) {
        const int k = idx / kTile, r = idx - k * kTile;
        sC[r][k] = j0 + r < P.n ? A[(size_t)(P.c0 + k) * P.ld + j0 + r] : 0.0;
    }
    __syncthreads();
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            acc[a][b] = (i < P.n && j <= i) ? A[(size_t)i * P.ld + j] : 0.0;
        }
#pragma unroll 2
    for (int k = 0; k < w; ++k) {
        double l[4], c[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { l[a] = sL[ty + 16 * a][k]; c[a] = sC[tx + 16 * a][k]; }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = ldlt_fnma(acc[a][b], l[a], c[b]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < P.n && j <= i) A[(size_t)i * P.ld + j] = acc[a][b];
        }
}

// ---- the substitutions ---------------------------------------------------------------------------------------------------------
// L y = b: the panel's own rows, column by column
template <class V, int NB> __global__ __launch_bounds__(64) void k_fwd_diag(V v, int p)
{
    __shared__ double sLd[NB][NB + 1], sy[NB];
    const Panel P = panel_of<V, NB>(v, p);
    if (!P.due) return;
    const int tid = threadIdx.x, w = P.w;
    const double *A = v.A();
    double *y = v.y();
    for (int idx = tid; idx < w * w; idx += 64) {
        const int i = idx / w, j = idx - i * w;
        if (j < i) sLd[i][j] = A[(size_t)(P.c0 + i) * P.ld + P.c0 + j];
    }
    if (tid < w) sy[tid] = y[P.c0 + tid];
    __syncthreads();
    for (int k = 0; k < w; ++k) {
        const double yk = sy[k];
        __syncthreads();
        if (tid > k && tid < w) sy[tid] = ldlt_fnma(sy[tid], sLd[tid][k], yk);
        __syncthreads();
    }
    if (tid < w) y[P.c0 + tid] = sy[tid];
}
// the rows below the panel: one lane per row over the panel's columns in order, the tile staged through LDS
template <class V, int NB> __global__ __launch_bounds__(64) void k_fwd_upd(V v, int p)
{
    __shared__ double sT[kTile][NB + 1], sy[NB];
    const Panel P = panel_of<V, NB>(v, p);
    const int r0 = P.c0 + P.w + blockIdx.x * kTile;
    if (!P.due || r0 >= P.n) return;
    const int tid = threadIdx.x, w = P.w;
    const double *A = v.A();
    double *y = v.y();
    for (int idx = tid; idx < kTile * w; idx += 64) {
        const int r = idx / w, k = idx - r * w;
        sT[r][k] = r0 + r < P.n ? A[(size_t)(r0 + r) * P.ld + P.c0 + k] : 0.0;
    }
    if (tid < w) sy[tid] = y[P.c0 + tid];
    __syncthreads();
    if (r0 + tid >= P.n) return;
    double s = y[r0 + tid];
    for (int k = 0; k < w; ++k) s = ldlt_fnma(s, sT[tid][k], sy[k]);
    y[r0 + tid] = s;
}
template <class V> __global__ __launch_bounds__(kItem) void k_dscale(V v)
{
    if (!v.due()) return;
    const int n = v.n();
    const double *A = v.A();
    double *y = v.y();
    for (int i = blockIdx.x * kItem + threadIdx.x; i < n; i += gridDim.x * kItem) y[i] = y[i] / A[(size_t)i * n + i];
}
// L^T x = y: the panel's own rows from its last column, then the rows above it
template <class V, int NB> __global__ __launch_bounds__(64) void k_bwd_diag(V v, int p)
{
    __shared__ double sLd[NB][NB + 1], sy[NB];
    const Panel P = panel_of<V, NB>(v, p);
    if (!P.due) return;
    const int tid = threadIdx.x, w = P.w;
    const double *A = v.A();
    double *y = v.y();
    for (int idx = tid; idx < w * w; idx += 64) {
        const int i = idx / w, j = idx - i * w;
        if (j < i) sLd[i][j] = A[(size_t)(P.c0 + i) * P.ld + P.c0 + j];
    }
    if (tid < w) sy[tid] = y[P.c0 + tid];
    __syncthreads();
    for (int j = w - 1; j > 0; --j) {
        const double yj = sy[j];
        __syncthreads();
        if (tid < j) sy[tid] = ldlt_fnma(sy[tid], sLd[j][tid], yj);
        __syncthreads();
    }
    if (tid < w) y[P.c0 + tid] = sy[tid];
}
template <class V, int NB> __global__ __launch_bounds__(kItem) void k_bwd_upd(V v, int p)
{
    __shared__ double sy[NB];
    const Panel P = panel_of<V, NB>(v, p);
    const int i = blockIdx.x * kItem + threadIdx.x;
    if (!P.due || (int)(blockIdx.x * kItem) >= P.c0) return;
    const double *A = v.A();
    double *y = v.y();
    if ((int)threadIdx.x < P.w) sy[threadIdx.x] = y[P.c0 + threadIdx.x];
    __syncthreads();
    if (i >= P.c0) return;
    double s = y[i];
    for (int j = P.w - 1; j >= 0; --j) s = ldlt_fnma(s, A[(size_t)(P.c0 + j) * P.ld + i], sy[j]);
    y[i] = s;
}

// Enqueues the factorisation and both substitutions of a system of at most nmax columns (the grids are sized from nmax; the
// kernels read the order itself from the view).  Returns the number of launches.
template <class V, int NB> int enqueue_solve(hipStream_t stream, const V &v, int nmax)
{
    const dim3 one(1), it(kItem), w64(64);
    const int panels = (nmax + NB - 1) / NB;
    int launches = 0;
    for (int p = 0; p < panels; ++p) {
        const int below = nmax - (p + 1) * NB;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_factor_diag<V, NB>), one, it, 0, stream, v, p);
        ++launches;
        if (below <= 0) continue;
        const int tiles = (below + kTile - 1) / kTile;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_factor_panel<V, NB>), dim3((below + kPanelRows - 1) / kPanelRows), it, 0, stream, v, p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_factor_trail<V, NB>), dim3(tiles, tiles), it, 0, stream, v, p);
        launches += 2;
    }
    for (int p = 0; p < panels; ++p) {
        const int below = nmax - (p + 1) * NB;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fwd_diag<V, NB>), one, w64, 0, stream, v, p);
        ++launches;
        if (below <= 0) continue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fwd_upd<V, NB>), dim3((below + kTile - 1) / kTile), w64, 0, stream, v, p);
        ++launches;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dscale<V>), dim3(16), it, 0, stream, v);
    ++launches;
    for (int p = panels - 1; p >= 0; --p) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bwd_diag<V, NB>), one, w64, 0, stream, v, p);
        ++launches;
        if (p == 0) continue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bwd_upd<V, NB>), dim3((p * NB + kItem - 1) / kItem), it, 0, stream, v, p);
        ++launches;
    }
    return launches;
}

}  // namespace ldlt
}  // namespace orbhip
