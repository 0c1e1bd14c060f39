// What the five optimisers share below their own arithmetic, written once for the device and for one host thread
// (DESIGN.md section 3):
//   - g2o's Levenberg-Marquardt rule (optimization_algorithm_levenberg.cpp:75-163) over any record that carries the fields
//     lam, ni, current, ini, rho, qmax, n_bad_lm, it: PoWs, S3oWs, LbaState and EgState do.  What an optimiser does around
//     the rule -- restoring a backup or flipping a buffer, its counters, its phases -- stays in its own *_lm_judge;
//   - the pivoted LDLt of a small dense system held in registers (6 unknowns for a pose, 7 for a Sim3);
//   - the host replay of a team sum: lanes j mod TEAM, an xor butterfly over each 64 lanes (offsets 1 .. 32), then the
//     wavefronts in order.  The device form of the same combine is orbhip_team_dev.h.
// Everything is fp64, one rounding per operation.  Nothing here indexes a private array at run time.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PO_HD __host__ __device__ __forceinline__
#else
#define PO_HD inline
#endif

namespace orbhip {

constexpr double kPoDblMax = 1.7976931348623157e308;
constexpr int kTeamWave = 64;                           // lanes of a wavefront: part of the order of every team sum

// ---- OptimizationAlgorithmLevenberg::solve, cut where a team has to sum ------------------------------------------------
// :75-101 with the robust chi2 at the estimate; lam0 is the first iteration's lambda and is read then only
template <class S> PO_HD void lm_begin(S &st, double chi, double lam0)
{
    st.current = st.ini = chi;
    if (st.it == 0) { st.lam = lam0; st.ni = 2.0; st.n_bad_lm = 0; }
    st.rho = 0.0;
    st.qmax = 0;
}
// std::max(fabs(h), maxDiagonal) over the diagonal of a dense N x N H
template <int N> PO_HD double lm_max_diag(const double *H)
{
    double mx = 0.0;
    for (int j = 0; j < N; ++j) {
        const double a = fabs(H[j * N + j]);
        mx = a < mx ? mx : a;
    }
    return mx;
}
// computeScale of a dense system: sum of x (lambda x + b), ascending from 0.0
template <int N> PO_HD double lm_scale(const double *x, const double *b, double lam)
{
    double scale = 0.0;
    for (int j = 0; j < N; ++j) scale = scale + x[j] * (lam * x[j] + b[j]);
    return scale;
}
// :123-149 with the trial's robust chi2 and computeScale: the gain, the new lambda, one more trial counted.  Returns whether
// the trial is accepted (discardTop); the caller pops the estimate otherwise.
template <class S> PO_HD bool lm_gain(S &st, bool ok2, double temp, double scale)
{
    if (!ok2) temp = kPoDblMax;
    double rho = st.current - temp;
    scale = scale + 1e-3;
    rho = rho / scale;
    const bool accepted = rho > 0 && fabs(temp) <= kPoDblMax;
    if (accepted) {
        const double y = 2 * rho - 1;
        double alpha = 1.0 - (y * y) * y;
        alpha = 2.0 / 3.0 < alpha ? 2.0 / 3.0 : alpha;                         // std::min(alpha, 2/3)
        const double sf = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;                // std::max(1/3, alpha)
        st.lam = st.lam * sf;
        st.ni = 2.0;
        st.current = temp;
    } else {
        st.lam = st.lam * st.ni;
        st.ni = st.ni * 2;
    }
    st.rho = rho;
    st.qmax = st.qmax + 1;
    return accepted;
}
// :150: another trial of the same iteration
template <class S> PO_HD bool lm_retry(const S &st) { return st.rho < 0 && st.qmax < 10; }
// :152-163 when the trials of an iteration are over: false ends optimize()
template <class S> PO_HD bool lm_iteration_ok(S &st)
{
    if (st.qmax == 10 || st.rho == 0) return false;
    if ((st.ini - st.current) * 1e3 < st.ini) st.n_bad_lm = st.n_bad_lm + 1;
    else st.n_bad_lm = 0;
    return st.n_bad_lm < 3;
}

// ---- pivoted LDLt of a full symmetric N x N A, largest |d| first, the first of equals; b -> x when every pivot is > 0 -----
// The matrix is held in registers: every index below is a compile-time constant once the loops are unrolled, and a pivot
// found at run time is applied by comparing it with each candidate position in turn.  A failure leaves x as it was.
template <int N> PO_HD bool ldlt_solve_small(const double *A0, const double *b, double *x)
{
    double A[N * N], y[N];
    int tr[N];
#pragma unroll
    for (int k = 0; k < N * N; ++k) A[k] = A0[k];
#pragma unroll
    for (int k = 0; k < N; ++k) y[k] = b[k];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        double big = fabs(A[k * N + k]);
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double v = fabs(A[i * N + i]);
            if (v > big) { big = v; p = i; }
        }
        tr[k] = p;
#pragma unroll
        for (int q = k + 1; q < N; ++q)
            if (p == q) {
#pragma unroll
                for (int c = 0; c < N; ++c) { const double t = A[k * N + c]; A[k * N + c] = A[q * N + c]; A[q * N + c] = t; }
#pragma unroll
                for (int r = 0; r < N; ++r) { const double t = A[r * N + k]; A[r * N + k] = A[r * N + q]; A[r * N + q] = t; }
                const double t = y[k]; y[k] = y[q]; y[q] = t;                    // P b, a transposition at a time
            }
        const double d = A[k * N + k];
        if (!(d > 0)) return false;
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double l = A[i * N + k] / d;
#pragma unroll
            for (int j = k + 1; j <= i; ++j) {
                A[i * N + j] = A[i * N + j] - l * A[j * N + k];
                A[j * N + i] = A[i * N + j];
            }
        }
#pragma unroll
        for (int i = k + 1; i < N; ++i) A[i * N + k] = A[i * N + k] / d;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) y[i] = y[i] - A[i * N + j] * y[j];
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = y[i] / A[i * N + i];
#pragma unroll
    for (int i = N - 1; i >= 0; --i)
#pragma unroll
        for (int j = i + 1; j < N; ++j) y[i] = y[i] - A[j * N + i] * y[j];
#pragma unroll
    for (int k = N - 1; k >= 0; --k)                                              // P^T x: the transpositions undone, last first
#pragma unroll
        for (int q = k + 1; q < N; ++q)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = y[k];
    return true;
}

// ---- what two lanes' parts of a team sum become ----------------------------------------------------------------------------
struct TeamAdd {
    PO_HD double operator()(double a, double b) const { return a + b; }
};

// ---- the host team: one thread that replays the device team's order ----------------------------------------------------
struct HostTeam {
    bool is0() const { return true; }
    int first() const { return 0; }
    int stride() const { return 1; }
    void sync() {}
    void add(int *dst, int v) { *dst += v; }
};
// lanes[l] holds what lane l of a team of TEAM accumulated; sums k0 .. N - 1 of them meet in an xor butterfly over each
// wavefront (lanes is overwritten), then the wavefronts are combined in wavefront order into s[k0 .. N - 1]
template <int TEAM, int N, class Op> inline void host_team_combine(double (*lanes)[N], int k0, double *s, Op op)
{
    for (int w0 = 0; w0 < TEAM; w0 += kTeamWave) {
        for (int off = 1; off < kTeamWave; off <<= 1) {
            double nxt[kTeamWave][N];
            for (int l = 0; l < kTeamWave; ++l)
                for (int k = k0; k < N; ++k) nxt[l][k] = op(lanes[w0 + l][k], lanes[w0 + (l ^ off)][k]);
            for (int l = 0; l < kTeamWave; ++l)
                for (int k = k0; k < N; ++k) lanes[w0 + l][k] = nxt[l][k];
        }
        for (int k = k0; k < N; ++k) s[k] = w0 == 0 ? lanes[0][k] : op(s[k], lanes[w0][k]);
    }
}

}  // namespace orbhip
