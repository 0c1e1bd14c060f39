// Sim3 RANSAC on the device: Sim3Solver (src/Sim3Solver.cc) for the current key frame and C candidates, over tables
// (include/orbhip.h, section "Sim3 RANSAC").  gfx950 only, wave64.  The arithmetic is tests/seqref/sim3.py operation by
// operation: cv::Mat products accumulate in fp64 and round once, Mat::dot is a double, everything else
// is fp32 with one rounding per operation; the eigenvector comes from a two-sided cyclic Jacobi method in fp32.  No float
// atomics and no reductions over floats: every float result is computed by one lane from its own operands, the only values
// that cross lanes are inlier bits and their integer counts, so nothing depends on the launch geometry.
//
// Launches, all on the caller's stream:
//   k_sim3_setup        one workgroup per candidate: the skip rules of the constructor per slot of the current key frame,
//                       ordered compaction of the kept slots, camera coordinates, projections, truncated thresholds
//   k_sim3_hypotheses   one lane per (candidate, iteration of this call): the draw replay in closed form, Horn's method,
//                       Jacobi, T12 / T21 into the workspace
//   k_sim3_score        one team of 16 lanes (N <= 64) or one wavefront per hypothesis: both projections of every
//                       correspondence, a ballot per 64, the inlier mask in 16-bit units and the count
//   k_sim3_select       one wavefront per candidate: the state machine of iterate as an exclusive prefix maximum over the
//                       counts of this call, the report, the state, the returned Sim3 and vbInliers through slot1
#include "orbhip_internal.h"

#include <algorithm>

namespace orbhip {
namespace {

constexpr int kSim3GroupMax = 64;   // up to this many correspondences a hypothesis is scored by 16 lanes, above by 64
constexpr int kSim3Sweeps = 10;     // JACOBI_SWEEPS of the sequential reference

// (a0 b0 + a1 b1) + a2 b2 in double
__device__ __forceinline__ double dot3d(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return __dadd_rn(__dadd_rn(__dmul_rn((double)a0, (double)b0), __dmul_rn((double)a1, (double)b1)), __dmul_rn((double)a2, (double)b2));
}
// one row of a cv::Mat product R X + t: fp64 accumulation, one rounding
__device__ __forceinline__ float row_dot(const float *T, const float X0, const float X1, const float X2)
{
    return (float)__dadd_rn(dot3d(T[0], T[1], T[2], X0, X1, X2), (double)T[3]);
}
// FromCameraToImage (:405-423) and the tail of Project (:397-401)
__device__ __forceinline__ void to_image(const Sim3Args &A, float X, float Y, float Z, float &u, float &v)
{
    const float invz = __fdiv_rn(1.0f, Z);
    u = __fadd_rn(__fmul_rn(A.fx, __fmul_rn(X, invz)), A.cx);
    v = __fadd_rn(__fmul_rn(A.fy, __fmul_rn(Y, invz)), A.cy);
}

// MapPoint::GetIndexInKeyFrame: the first entry of the point's list that names the row
__device__ __forceinline__ int index_in_key_frame(const Sim3Args &A, int p, int row)
{
    const int o1 = A.obs_start[p + 1];
    for (int o = A.obs_start[p]; o < o1; ++o)
        if (A.obs_kf[o] == row) return A.obs_idx[o];
    return -1;
}

__global__ __launch_bounds__(256) void k_sim3_setup(Sim3Args A)
{
    __shared__ int s_w[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int kf = A.kf_index[c], cur = A.cur;
    const bool kf_ok = (unsigned)kf < (unsigned)A.rows;
    const int n1 = min(max(A.n[cur], 0), A.cap);
    const size_t row = (size_t)c * A.cap;
    const int lv_max = min(max(A.n_levels, 1), ORBHIP_MAX_LEVELS) - 1;
    int running = 0;
    for (int b = 0; b < n1; b += 256) {
        const int i1 = b + tid;
        int p1 = -1, p2 = -1, idx1 = -1, idx2 = -1;
        bool keep = false;
        if (i1 < n1 && kf_ok) {
            const int m = A.matched12[row + i1];
            if (m >= 0) {                                                                               // :64
                p2 = A.match_form == ORBHIP_SIM3_MATCH_SLOTS ? (m < A.cap ? A.slot_point[(size_t)kf * A.cap + m] : -1) : m;
                p1 = A.slot_point[(size_t)cur * A.cap + i1];                                            // :69
                if ((unsigned)p1 < (unsigned)A.np && (unsigned)p2 < (unsigned)A.np && (A.flags[p1] & ORBHIP_POINT_PRESENT) &&
                    (A.flags[p2] & ORBHIP_POINT_PRESENT)) {                                             // :72
                    idx1 = index_in_key_frame(A, p1, cur);
                    idx2 = index_in_key_frame(A, p2, kf);
                    keep = (unsigned)idx1 < (unsigned)A.cap && (unsigned)idx2 < (unsigned)A.cap;        // :78
                }
            }
        }
        const int incl = wave_incl_scan_add(keep ? 1 : 0);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int off = running;
        for (int w = 0; w < wv; ++w) off += s_w[w];
        if (keep) {
            const size_t k = row + off + incl - 1;
            const int o1 = A.kps[(size_t)cur * A.cap + idx1].octave, o2 = A.kps[(size_t)kf * A.cap + idx2].octave;
            A.max_err1[k] = A.thr[min(max(o1, 0), lv_max)];
            A.max_err2[k] = A.thr[min(max(o2, 0), lv_max)];
            A.slot1[k] = i1;
            const float *T1 = A.Tcw + (size_t)cur * 12, *T2 = A.Tcw + (size_t)kf * 12;
            const float *W1 = A.world + (size_t)p1 * 3, *W2 = A.world + (size_t)p2 * 3;
            float X[3], Y[3], u, v;
            for (int r = 0; r < 3; ++r) {
                X[r] = row_dot(T1 + 4 * r, W1[0], W1[1], W1[2]);
                Y[r] = row_dot(T2 + 4 * r, W2[0], W2[1], W2[2]);
                A.x1[k * 3 + r] = X[r];
                A.x2[k * 3 + r] = Y[r];
            }
            to_image(A, X[0], X[1], X[2], u, v);
            A.p1[k * 2] = u; A.p1[k * 2 + 1] = v;
            to_image(A, Y[0], Y[1], Y[2], u, v);
            A.p2[k * 2] = u; A.p2[k * 2 + 1] = v;
        }
        running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (tid == 0) {
        A.n_corr[c] = running;
        A.n1[c] = n1;
        A.limit[c] = A.limit_tab[running];
        A.state[2 * c] = 0;
        A.state[2 * c + 1] = 0;
    }
}

// Eigenvector of the largest eigenvalue of the symmetric 4x4 a: two-sided cyclic Jacobi in fp32, jacobi_eig4 of the
// sequential reference.  A pair is skipped when |a_pq| <= 2 eps ||a||_F (the norm of the matrix as it comes in); a rotation
// updates the two columns, then the two rows, then stores exact zeros at (p,q) and (q,p).  Stops after a sweep without a
// rotation or after kSim3Sweeps.  The first maximum of the diagonal names the column of V.  All indices are compile-time.
__device__ __forceinline__ void jacobi_eig4(float (&a)[4][4], float (&x)[4])
{
    float v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.f : 0.f;
    float fro = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) fro = __fadd_rn(fro, __fmul_rn(a[i][j], a[i][j]));
    const float thresh = __fmul_rn(2.384185791015625e-07f, sqrt_rn(fro));   // 2 * FLT_EPSILON
    for (int sweep = 0; sweep < kSim3Sweeps; ++sweep) {
        bool changed = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const float gamma = a[p][q];
                if (!(fabsf(gamma) > thresh)) continue;
                changed = true;
                const float p2 = __fmul_rn(gamma, 2.f), bt = __fsub_rn(a[p][p], a[q][q]);
                const float g = sqrt_rn(__fadd_rn(__fmul_rn(p2, p2), __fmul_rn(bt, bt)));
                float cs, sn;
                if (bt < 0.f) {
                    const float delta = __fmul_rn(__fsub_rn(g, bt), 0.5f);
                    sn = sqrt_rn(__fdiv_rn(delta, g));
                    cs = __fdiv_rn(p2, __fmul_rn(__fmul_rn(g, sn), 2.f));
                } else {
                    cs = sqrt_rn(__fdiv_rn(__fadd_rn(g, bt), __fmul_rn(g, 2.f)));
                    sn = __fdiv_rn(p2, __fmul_rn(__fmul_rn(g, cs), 2.f));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float ap = a[r][p], aq = a[r][q], vp = v[r][p], vq = v[r][q];
                    a[r][p] = __fadd_rn(__fmul_rn(cs, ap), __fmul_rn(sn, aq));
                    a[r][q] = __fsub_rn(__fmul_rn(cs, aq), __fmul_rn(sn, ap));
                    v[r][p] = __fadd_rn(__fmul_rn(cs, vp), __fmul_rn(sn, vq));
                    v[r][q] = __fsub_rn(__fmul_rn(cs, vq), __fmul_rn(sn, vp));
                }
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const float ap = a[p][cc], aq = a[q][cc];
                    a[p][cc] = __fadd_rn(__fmul_rn(cs, ap), __fmul_rn(sn, aq));
                    a[q][cc] = __fsub_rn(__fmul_rn(cs, aq), __fmul_rn(sn, ap));
                }
                a[p][q] = 0.f;
                a[q][p] = 0.f;
            }
        if (!changed) break;
    }
    float w = a[0][0];
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = v[r][0];
#pragma unroll
    for (int cc = 1; cc < 4; ++cc) {
        const bool more = a[cc][cc] > w;
        w = more ? a[cc][cc] : w;
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = more ? v[r][cc] : x[r];
    }
}

// ComputeSim3 (:226-337).  P1[k] / P2[k] = point k of the sample (a column of the reference's 3x3).  out: T12 [12], T21 [12],
// R12 [9], t12 [3], s12.
__device__ __forceinline__ void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, float *out)
{
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3], M[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        O1[r] = __fdiv_rn(__fadd_rn(__fadd_rn(P1[0][r], P1[1][r]), P1[2][r]), 3.0f);
        O2[r] = __fdiv_rn(__fadd_rn(__fadd_rn(P2[0][r], P2[1][r]), P2[2][r]), 3.0f);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Pr1[k][r] = __fsub_rn(P1[k][r], O1[r]);
            Pr2[k][r] = __fsub_rn(P2[k][r], O2[r]);
        }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = (float)dot3d(Pr2[0][r], Pr2[1][r], Pr2[2][r], Pr1[0][c], Pr1[1][c], Pr1[2][c]);   // :243
    float N[4][4];
    N[0][0] = __fadd_rn(__fadd_rn(M[0][0], M[1][1]), M[2][2]);                  // :251-260, float sums
    N[0][1] = __fsub_rn(M[1][2], M[2][1]);
    N[0][2] = __fsub_rn(M[2][0], M[0][2]);
    N[0][3] = __fsub_rn(M[0][1], M[1][0]);
    N[1][1] = __fsub_rn(__fsub_rn(M[0][0], M[1][1]), M[2][2]);
    N[1][2] = __fadd_rn(M[0][1], M[1][0]);
    N[1][3] = __fadd_rn(M[2][0], M[0][2]);
    N[2][2] = __fsub_rn(__fadd_rn(-M[0][0], M[1][1]), M[2][2]);
    N[2][3] = __fadd_rn(M[1][2], M[2][1]);
    N[3][3] = __fadd_rn(__fsub_rn(-M[0][0], M[1][1]), M[2][2]);
    N[1][0] = N[0][1]; N[2][0] = N[0][2]; N[3][0] = N[0][3]; N[2][1] = N[1][2]; N[3][1] = N[1][3]; N[3][2] = N[2][3];
    float q[4];
    jacobi_eig4(N, q);
    // the rotation of the normalised quaternion (w, x, y, z)
    const float nrm = sqrt_rn(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[1], q[1])), __fmul_rn(q[2], q[2])),
                                        __fmul_rn(q[3], q[3])));
    const float w = __fdiv_rn(q[0], nrm), x = __fdiv_rn(q[1], nrm), y = __fdiv_rn(q[2], nrm), z = __fdiv_rn(q[3], nrm);
    const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
    const float xy = __fmul_rn(x, y), xz = __fmul_rn(x, z), yz = __fmul_rn(y, z);
    const float wx = __fmul_rn(w, x), wy = __fmul_rn(w, y), wz = __fmul_rn(w, z);
    float R[3][3];
    R[0][0] = __fsub_rn(1.f, __fmul_rn(2.f, __fadd_rn(yy, zz)));
    R[0][1] = __fmul_rn(2.f, __fsub_rn(xy, wz));
    R[0][2] = __fmul_rn(2.f, __fadd_rn(xz, wy));
    R[1][0] = __fmul_rn(2.f, __fadd_rn(xy, wz));
    R[1][1] = __fsub_rn(1.f, __fmul_rn(2.f, __fadd_rn(xx, zz)));
    R[1][2] = __fmul_rn(2.f, __fsub_rn(yz, wx));
    R[2][0] = __fmul_rn(2.f, __fsub_rn(xz, wy));
    R[2][1] = __fmul_rn(2.f, __fadd_rn(yz, wx));
    R[2][2] = __fsub_rn(1.f, __fmul_rn(2.f, __fadd_rn(xx, yy)));
    float s = 1.0f;
    if (!fix_scale) {                                                           // :292-309
        float P3[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r) P3[k][r] = (float)dot3d(R[r][0], R[r][1], R[r][2], Pr2[k][0], Pr2[k][1], Pr2[k][2]);
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                nom = __dadd_rn(nom, __dmul_rn((double)Pr1[k][r], (double)P3[k][r]));
                den = __dadd_rn(den, (double)__fmul_rn(P3[k][r], P3[k][r]));
            }
        s = (float)__ddiv_rn(nom, den);
    }
    float t[3], sRinv[3][3];
    const double inv = __ddiv_rn(1.0, (double)s);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        t[r] = (float)__dsub_rn((double)O1[r], __dmul_rn((double)s, dot3d(R[r][0], R[r][1], R[r][2], O2[0], O2[1], O2[2])));   // :316
#pragma unroll
        for (int c = 0; c < 3; ++c) sRinv[r][c] = (float)__dmul_rn(inv, (double)R[c][r]);                                     // :332
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out[4 * r + c] = __fmul_rn(s, R[r][c]);                             // :323
            out[12 + 4 * r + c] = sRinv[r][c];
            out[24 + 3 * r + c] = R[r][c];
        }
        out[4 * r + 3] = t[r];
        out[12 + 4 * r + 3] = (float)(-dot3d(sRinv[r][0], sRinv[r][1], sRinv[r][2], t[0], t[1], t[2]));                        // :335
        out[33 + r] = t[r];
    }
    out[36] = s;
}

// the iteration numbers a call runs for candidate c: [it0, it0 + n_run)
__device__ __forceinline__ int sim3_run(const Sim3Args &A, int c, int &it0, int &N)
{
    N = min(max(A.n_corr[c], 0), A.cap);
    it0 = A.state[2 * c];
    if (N < A.min_inliers || N < 3 || it0 < 0) return 0;
    return max(min(A.n_iter, min(A.limit[c], A.max_its) - it0), 0);
}

__global__ __launch_bounds__(64) void k_sim3_hypotheses(Sim3Args A)
{
    const int c = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    int it0, N;
    if (j >= sim3_run(A, c, it0, N)) return;
    const int *d = A.draws + ((size_t)c * A.max_its + it0 + j) * 3;
    // :163-177 in closed form.  The list starts as the identity; taking position r out moves the last entry there.
    const int r0 = d[0], r1 = d[1], r2 = d[2];
    const int back1 = r0 == N - 2 ? N - 1 : N - 2;                 // the last entry when the second draw is taken out
    int idx[3];
    idx[0] = r0;
    idx[1] = r1 == r0 ? N - 1 : r1;
    idx[2] = r2 == r1 ? back1 : (r2 == r0 ? N - 1 : r2);
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t e = ((size_t)c * A.cap + min(max(idx[k], 0), N - 1)) * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) { P1[k][r] = A.x1[e + r]; P2[k][r] = A.x2[e + r]; }
    }
    float out[kSim3HypFloats];
    compute_sim3(P1, P2, A.fix_scale != 0, out);
    float *h = A.hyp + ((size_t)c * A.n_iter + j) * kSim3HypFloats;
#pragma unroll
    for (int i = 0; i < 37; ++i) h[i] = out[i];
}

// CheckInliers (:340-364) for correspondence i of candidate c under the hypothesis h
__device__ __forceinline__ bool sim3_inlier(const Sim3Args &A, const float *h, size_t e)
{
    const float *X1 = A.x1 + e * 3, *X2 = A.x2 + e * 3;
    float u1, v1, u2, v2;
    to_image(A, row_dot(h, X2[0], X2[1], X2[2]), row_dot(h + 4, X2[0], X2[1], X2[2]), row_dot(h + 8, X2[0], X2[1], X2[2]), u1, v1);
    to_image(A, row_dot(h + 12, X1[0], X1[1], X1[2]), row_dot(h + 16, X1[0], X1[1], X1[2]), row_dot(h + 20, X1[0], X1[1], X1[2]), u2, v2);
    const float dx1 = __fsub_rn(A.p1[e * 2], u1), dy1 = __fsub_rn(A.p1[e * 2 + 1], v1);
    const float dx2 = __fsub_rn(u2, A.p2[e * 2]), dy2 = __fsub_rn(v2, A.p2[e * 2 + 1]);
    const float err1 = (float)__dadd_rn(__dmul_rn((double)dx1, (double)dx1), __dmul_rn((double)dy1, (double)dy1));
    const float err2 = (float)__dadd_rn(__dmul_rn((double)dx2, (double)dx2), __dmul_rn((double)dy2, (double)dy2));
    return err1 < (float)A.max_err1[e] && err2 < (float)A.max_err2[e];
}

// A team of `lanes` lanes (16 or 64) scores hypothesis j over all correspondences.  Every 16-lane row of the ballot is one
// mask unit; its leader stores it.
__device__ __forceinline__ void sim3_score_team(const Sim3Args &A, int c, int j, int N, int tl, int lanes)
{
    const int lane = threadIdx.x & 63, row_shift = lane & ~15;
    float h[24];
    const float *hp = A.hyp + ((size_t)c * A.n_iter + j) * kSim3HypFloats;
#pragma unroll
    for (int i = 0; i < 24; ++i) h[i] = hp[i];
    uint16_t *mask = A.mask + ((size_t)c * A.n_iter + j) * A.cap16;
    int count = 0;
    for (int b = 0; b < N; b += lanes) {
        const int i = b + tl;
        const bool in = i < N && sim3_inlier(A, h, (size_t)c * A.cap + i);
        const unsigned bits = (unsigned)(__ballot(in) >> row_shift) & 0xffffu;
        if ((lane & 15) == 0 && i < N) { mask[i >> 4] = (uint16_t)bits; count += __popc(bits); }
    }
    for (int s = 16; s < lanes; s <<= 1) count += __shfl_xor(count, s);
    if (tl == 0) A.count[(size_t)c * A.n_iter + j] = count;
}

__global__ __launch_bounds__(256) void k_sim3_score(Sim3Args A)
{
    const int c = blockIdx.y, tid = threadIdx.x;
    int it0, N;
    const int n_run = sim3_run(A, c, it0, N);
    if (N <= kSim3GroupMax) {
        for (int j = blockIdx.x * 16 + (tid >> 4); j < n_run; j += gridDim.x * 16) sim3_score_team(A, c, j, N, tid & 15, 16);
    } else {
        for (int j = blockIdx.x * 4 + (tid >> 6); j < n_run; j += gridDim.x * 4) sim3_score_team(A, c, j, N, tid & 63, 64);
    }
}

// inclusive maximum scan over the wavefront
__device__ __forceinline__ int wave_incl_scan_max(int v, int lane)
{
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s);
        if (lane >= s) v = max(v, o);
    }
    return v;
}

__global__ __launch_bounds__(64) void k_sim3_select(Sim3Args A)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    int it0, N;
    const int n_run = sim3_run(A, c, it0, N);
    const int n1 = min(max(A.n1[c], 0), A.cap);
    uint8_t *inl = A.inliers + (size_t)c * A.cap;
    for (int i = lane; i < n1; i += 64) inl[i] = 0;                             // :143
    int best = A.state[2 * c + 1], found = -1, found_count = 0;
    for (int b = 0; b < n_run && found < 0; b += 64) {
        const int j = b + lane;
        const int cnt = j < n_run ? A.count[(size_t)c * A.n_iter + j] : -1;
        const int incl = wave_incl_scan_max(cnt, lane);
        int before = __shfl_up(incl, 1);                                        // the best of the iterations in front
        before = lane == 0 ? best : max(before, best);
        const unsigned long long hit = __ballot(j < n_run && cnt >= before && cnt > A.min_inliers);   // :183, :192
        if (hit) {
            const int l = __ffsll((long long)hit) - 1;
            found = b + l;
            found_count = __shfl(cnt, l);
        } else {
            best = max(best, __shfl(incl, 63));
        }
    }
    int *rep = A.report + (size_t)c * 8;
    const bool too_few = N < A.min_inliers;
    const int limit = A.limit[c];
    int status, iters, ret_it = -1, n_inl = 0;
    if (found >= 0) {
        status = ORBHIP_SIM3_RETURNED; iters = it0 + found + 1; best = found_count; ret_it = it0 + found; n_inl = found_count;
    } else {
        iters = it0 + n_run;
        status = too_few ? ORBHIP_SIM3_TOO_FEW : (iters >= limit ? ORBHIP_SIM3_NO_MORE : ORBHIP_SIM3_CONTINUE);   // :203
    }
    if (lane == 0) {
        rep[0] = status; rep[1] = N; rep[2] = limit; rep[3] = iters; rep[4] = best; rep[5] = ret_it; rep[6] = n_inl; rep[7] = 0;
        if (!too_few) { A.state[2 * c] = iters; A.state[2 * c + 1] = best; }
    }
    if (found < 0) return;
    const float *h = A.hyp + ((size_t)c * A.n_iter + found) * kSim3HypFloats;
    if (lane < 16) A.sim3[(size_t)c * 16 + lane] = lane < 13 ? h[24 + lane] : 0.f;
    __threadfence();                                                            // the zeros above land before the marks below
    const uint16_t *mask = A.mask + ((size_t)c * A.n_iter + found) * A.cap16;
    const int *slot1 = A.slot1 + (size_t)c * A.cap;
    for (int i = lane; i < N; i += 64)
        if ((mask[i >> 4] >> (i & 15)) & 1) {
            const int s = slot1[i];
            if ((unsigned)s < (unsigned)A.cap) inl[s] = 1;                      // :197
        }
}

}  // namespace

size_t sim3_workspace_bytes(int C, int n_iter, int cap)
{
    const size_t H = (size_t)std::max(C, 1) * std::max(n_iter, 1), cap16 = ((size_t)cap + 15) / 16;
    return H * kSim3HypFloats * sizeof(float) + H * sizeof(int) + H * cap16 * sizeof(uint16_t) + 512;
}

int launch_sim3_setup(hipStream_t stream, Sim3Args A)
{
    if (A.C <= 0) return ORBHIP_OK;
    hipLaunchKernelGGL(k_sim3_setup, dim3(A.C), dim3(256), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

int launch_sim3_iterate(hipStream_t stream, Sim3Args A, void *workspace)
{
    if (A.C <= 0) return ORBHIP_OK;
    const size_t H = (size_t)A.C * std::max(A.n_iter, 1);
    A.cap16 = (A.cap + 15) / 16;
    uint8_t *w = (uint8_t *)workspace;
    A.hyp = (float *)w;
    w += (H * kSim3HypFloats * sizeof(float) + 255) & ~(size_t)255;
    A.count = (int *)w;
    w += (H * sizeof(int) + 255) & ~(size_t)255;
    A.mask = (uint16_t *)w;
    if (A.n_iter > 0) {
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3((A.n_iter + 63) / 64, A.C), dim3(64), 0, stream, A);
        ORBHIP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_sim3_score, dim3((A.n_iter + 3) / 4, A.C), dim3(256), 0, stream, A);
        ORBHIP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sim3_select, dim3(A.C), dim3(64), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
