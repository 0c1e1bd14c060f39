// EPnP (src/PnPsolver.cc:375-858) over a workspace, operation by operation what tests/seqref/pnp.py does.
// Everything is fp64, one rounding per operation (the library is built with -ffp-contract=off).  The same text serves a
// team of TS lanes on the device and a single host thread (TS = 1), so the host can replay a device result bit for bit:
//   - a sum over correspondences belongs to ONE lane, which adds left to right in the order of the correspondences, so the
//     value does not depend on TS or on the launch geometry;
//   - the Jacobi eigen-solver gives row r of A and of V to lane r of the first 16 lanes; a rotation reads the pivots, then
//     every lane rewrites its own row's two entries and their mirror images.  No lane reads what another lane writes between
//     two hand-offs, so running the lanes one after the other (TS = 1) gives the same bits;
//   - everything else is small and serial: lane 0 does it.
// All arrays live in the workspace (LDS on the device) and are indexed there; nothing here needs a private array.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ __forceinline__
#else
#define PNP_HD inline
#endif

namespace orbhip {

constexpr int kPnpEigSweeps = 15, kPnpSvdSweeps = 30;
constexpr double kPnpEigEps = 1.1102230246251565e-16;    // 2^-53
constexpr double kPnpSvdEps = 2.220446049250313e-16;     // 2^-52
constexpr double kPnpSvdCut = 6 * 2.220446049250313e-16;

struct PnpWs {
    double A[144], V[144];          // the symmetric eigenproblem, row stride = its size (12 or 3)
    double w[12];
    double v4[48];                  // v[0..3] of compute_L_6x10: the eigenvectors of the four smallest eigenvalues
    double c0[3], cws[12], ci[9];   // centroid, control points [4][3], cc_inv
    double L[60], rho[6];
    double B[30], Vs[25], s2[5], coef[5], x[5];   // one-sided Jacobi: B [m][n] -> B V, Vs, squared column norms
    double ga[24], gb[6], gx[4], A1[4], A2[4];    // gauss_newton / qr_solve
    double betas[4], ccs[12];
    double sums[16];
    double pc0[3], pw0[3], R[9], t[3];
    double bestR[9], bestT[3], best_err;
    int order[12];
    int idx[4];                     // the sample of a four-point hypothesis
    int n, first;
};

// the correspondences of one pose: idx != nullptr: idx[0 .. lim) in this order; else every i < lim with mask[i] != 0
struct PnpCorr {
    const float *p3d, *p2d;         // [.][3], [.][2]
    const uint8_t *mask;
    const int *idx;
    int lim;
    double fu, fv, uc, vc;
};

template <int TS> PNP_HD void pnp_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (TS <= 16) wave_lds_handoff(); else __syncthreads();
#endif
}
PNP_HD void pnp_sync16()
{
#if defined(__HIP_DEVICE_COMPILE__)
    wave_lds_handoff();
#endif
}

#define PNP_FOR_CORR(S, k, e)                       \
    for (int k = 0, e = 0; k < (S).lim; ++k)        \
        if (((S).idx ? (e = (S).idx[k], true) : (e = k, (S).mask[k] != 0)))

PNP_HD void pnp_rot(double theta, double &c, double &s, double &t)
{
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0) t = -t;
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

// jacobi_eig of the seqref on W.A (n x n, stride n): lanes jl, jl + js, ... < n own the rows.  Called by the first
// min(TS, 16) lanes of a team, which sit in one wavefront.  Leaves W.w (diagonal) and W.order (descending, stable).
PNP_HD void pnp_jacobi_eig(PnpWs &W, int n, int jl, int js)
{
    for (int r = jl; r < n; r += js)
        for (int c = 0; c < n; ++c) W.V[r * n + c] = r == c ? 1.0 : 0.0;
    double fro = 0.0;
    for (int i = 0; i < n * n; ++i) fro = fro + W.A[i] * W.A[i];
    const double thresh = kPnpEigEps * sqrt(fro);
    pnp_sync16();
    for (int sweep = 0; sweep < kPnpEigSweeps; ++sweep) {
        bool changed = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = W.A[p * n + q];
                if (!(fabs(apq) > thresh)) continue;
                changed = true;
                const double app = W.A[p * n + p], aqq = W.A[q * n + q];
                pnp_sync16();                                   // the pivots are read before anyone rewrites them
                double c, s, t;
                pnp_rot((aqq - app) / (2.0 * apq), c, s, t);
                for (int r = jl; r < n; r += js) {
                    if (r == p) {
                        W.A[p * n + p] = app - t * apq;
                        W.A[p * n + q] = 0.0;
                    } else if (r == q) {
                        W.A[q * n + q] = aqq + t * apq;
                        W.A[q * n + p] = 0.0;
                    } else {
                        const double ap = W.A[r * n + p], aq = W.A[r * n + q];
                        const double np_ = c * ap - s * aq, nq = s * ap + c * aq;
                        W.A[r * n + p] = np_; W.A[p * n + r] = np_;
                        W.A[r * n + q] = nq; W.A[q * n + r] = nq;
                    }
                    const double vp = W.V[r * n + p], vq = W.V[r * n + q];
                    W.V[r * n + p] = c * vp - s * vq;
                    W.V[r * n + q] = s * vp + c * vq;
                }
                pnp_sync16();
            }
        if (!changed) break;
    }
    if (jl == 0) {
        for (int i = 0; i < n; ++i) W.w[i] = W.A[i * n + i];
        unsigned used = 0;
        for (int k = 0; k < n; ++k) {
            int b = -1;
            for (int i = 0; i < n; ++i)
                if (!((used >> i) & 1) && (b < 0 || W.w[i] > W.w[b])) b = i;
            used |= 1u << b;
            W.order[k] = b;
        }
    }
    pnp_sync16();
}

// svd_cols of the seqref on W.B [m][n] (row stride n) and W.Vs [n][n]; leaves W.s2.  Serial.
PNP_HD void pnp_svd_cols(PnpWs &W, int m, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) W.Vs[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kPnpSvdSweeps; ++sweep) {
        bool changed = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int i = 0; i < m; ++i) {
                    const double xp = W.B[i * n + p], xq = W.B[i * n + q];
                    al = al + xp * xp;
                    be = be + xq * xq;
                    ga = ga + xp * xq;
                }
                if (!(fabs(ga) > kPnpSvdEps * sqrt(al * be))) continue;
                changed = true;
                double c, s, t;
                pnp_rot((be - al) / (2.0 * ga), c, s, t);
                for (int i = 0; i < m; ++i) {
                    const double xp = W.B[i * n + p], xq = W.B[i * n + q];
                    W.B[i * n + p] = c * xp - s * xq;
                    W.B[i * n + q] = s * xp + c * xq;
                }
                for (int i = 0; i < n; ++i) {
                    const double xp = W.Vs[i * n + p], xq = W.Vs[i * n + q];
                    W.Vs[i * n + p] = c * xp - s * xq;
                    W.Vs[i * n + q] = s * xp + c * xq;
                }
            }
        if (!changed) break;
    }
    for (int j = 0; j < n; ++j) {
        double a = 0.0;
        for (int i = 0; i < m; ++i) a = a + W.B[i * n + j] * W.B[i * n + j];
        W.s2[j] = a;
    }
}
// the cut-off of the pseudo-inverse: sigma_j > kPnpSvdCut * sigma_max
PNP_HD double pnp_svd_floor(const PnpWs &W, int n)
{
    double smax = 0.0;
    for (int j = 0; j < n; ++j) {
        const double s = sqrt(W.s2[j]);
        if (s > smax) smax = s;
    }
    return kPnpSvdCut * smax;
}
// svd_solve: W.B [m][n] x = b, x into W.x
PNP_HD void pnp_svd_solve(PnpWs &W, int m, int n, const double *b)
{
    pnp_svd_cols(W, m, n);
    const double fl = pnp_svd_floor(W, n);
    for (int j = 0; j < n; ++j) {
        double d = 0.0;
        for (int i = 0; i < m; ++i) d = d + W.B[i * n + j] * b[i];
        W.coef[j] = d / W.s2[j];
    }
    for (int k = 0; k < n; ++k) {
        double a = 0.0;
        for (int j = 0; j < n; ++j)
            if (sqrt(W.s2[j]) > fl) a = a + W.coef[j] * W.Vs[k * n + j];
        W.x[k] = a;
    }
}

// qr_solve (:860-950) on W.ga [6][4], W.gb, X = W.gx
PNP_HD void pnp_qr_solve(PnpWs &W)
{
    const int nr = 6, nc = 4;
    double *A = W.ga, *b = W.gb, *X = W.gx;
    for (int k = 0; k < nc; ++k) {
        const int kk = k * nc + k;
        int p = kk;
        double eta = fabs(A[p]);
        for (int i = k + 1; i < nr; ++i) {          // :881-885: the pointer lags the index by one row
            const double elt = fabs(A[p]);
            if (eta < elt) eta = elt;
            p += nc;
        }
        if (eta == 0) return;                       // :887-890, X keeps what it held
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        p = kk;
        for (int i = k; i < nr; ++i) {
            A[p] = A[p] * inv_eta;
            sum = sum + A[p] * A[p];
            p += nc;
        }
        double sigma = sqrt(sum);
        if (A[kk] < 0) sigma = -sigma;
        A[kk] = A[kk] + sigma;
        W.A1[k] = sigma * A[kk];
        W.A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s = 0.0;
            p = kk;
            for (int i = k; i < nr; ++i) { s = s + A[p] * A[p + j - k]; p += nc; }
            const double tau = s / W.A1[k];
            p = kk;
            for (int i = k; i < nr; ++i) { A[p + j - k] = A[p + j - k] - tau * A[p]; p += nc; }
        }
    }
    for (int j = 0; j < nc; ++j) {
        double tau = 0.0;
        int p = j * nc + j;
        for (int i = j; i < nr; ++i) { tau = tau + A[p] * b[i]; p += nc; }
        tau = tau / W.A1[j];
        p = j * nc + j;
        for (int i = j; i < nr; ++i) { b[i] = b[i] - tau * A[p]; p += nc; }
    }
    X[nc - 1] = b[nc - 1] / W.A2[nc - 1];
    for (int i = nc - 2; i >= 0; --i) {
        double s = 0.0;
        for (int j = i + 1; j < nc; ++j) s = s + A[i * nc + j] * X[j];
        X[i] = (b[i] - s) / W.A2[i];
    }
}

PNP_HD void pnp_alphas(const PnpWs &W, const PnpCorr &S, int e, double &a0, double &a1, double &a2, double &a3)
{
    const double d0 = (double)S.p3d[e * 3] - W.c0[0], d1 = (double)S.p3d[e * 3 + 1] - W.c0[1], d2 = (double)S.p3d[e * 3 + 2] - W.c0[2];
    a1 = W.ci[0] * d0 + W.ci[1] * d1 + W.ci[2] * d2;
    a2 = W.ci[3] * d0 + W.ci[4] * d1 + W.ci[5] * d2;
    a3 = W.ci[6] * d0 + W.ci[7] * d1 + W.ci[8] * d2;
    a0 = 1.0 - a1 - a2 - a3;
}
// entry `col` of rows 2i and 2i + 1 of M (fill_M, :436-451)
PNP_HD void pnp_m_entry(const PnpCorr &S, int col, double a0, double a1, double a2, double a3, double u, double v, double &m1, double &m2)
{
    const int i = col / 3, k = col - 3 * i;
    const double as = i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : a3));
    m1 = k == 0 ? as * S.fu : (k == 1 ? 0.0 : as * (S.uc - u));
    m2 = k == 0 ? 0.0 : (k == 1 ? as * S.fv : as * (S.vc - v));
}
// component j of pc = sum_i alpha_i ccs[i]
PNP_HD double pnp_pc(const PnpWs &W, int j, double a0, double a1, double a2, double a3)
{
    return a0 * W.ccs[j] + a1 * W.ccs[3 + j] + a2 * W.ccs[6 + j] + a3 * W.ccs[9 + j];
}

PNP_HD void pnp_find_betas(PnpWs &W, int which)
{
    const int n = which == 1 ? 4 : (which == 2 ? 3 : 5);
    for (int i = 0; i < 6; ++i)
        for (int c = 0; c < n; ++c) {
            const int col = which == 1 ? (c == 0 ? 0 : (c == 1 ? 1 : (c == 2 ? 3 : 6))) : c;
            W.B[i * n + c] = W.L[i * 10 + col];
        }
    pnp_svd_solve(W, 6, n, W.rho);
    const double *b = W.x;
    double *be = W.betas;
    be[0] = be[1] = be[2] = be[3] = 0.0;
    if (which == 1) {
        if (b[0] < 0) {
            be[0] = sqrt(-b[0]);
            be[1] = -b[1] / be[0]; be[2] = -b[2] / be[0]; be[3] = -b[3] / be[0];
        } else {
            be[0] = sqrt(b[0]);
            be[1] = b[1] / be[0]; be[2] = b[2] / be[0]; be[3] = b[3] / be[0];
        }
        return;
    }
    if (b[0] < 0) {
        be[0] = sqrt(-b[0]);
        be[1] = b[2] < 0 ? sqrt(-b[2]) : 0.0;
    } else {
        be[0] = sqrt(b[0]);
        be[1] = b[2] > 0 ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) be[0] = -be[0];
    if (which == 3) be[2] = b[3] / be[0];
}

PNP_HD void pnp_gauss_newton(PnpWs &W)
{
    double *be = W.betas;
    W.gx[0] = W.gx[1] = W.gx[2] = W.gx[3] = 0.0;
    for (int it = 0; it < 5; ++it) {
        for (int i = 0; i < 6; ++i) {
            const double *r = W.L + i * 10;
            double *a = W.ga + i * 4;
            a[0] = 2.0 * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3];
            a[1] = r[1] * be[0] + 2.0 * r[2] * be[1] + r[4] * be[2] + r[7] * be[3];
            a[2] = r[3] * be[0] + r[4] * be[1] + 2.0 * r[5] * be[2] + r[8] * be[3];
            a[3] = r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + 2.0 * r[9] * be[3];
            W.gb[i] = W.rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] + r[3] * be[0] * be[2] +
                                  r[4] * be[1] * be[2] + r[5] * be[2] * be[2] + r[6] * be[0] * be[3] + r[7] * be[1] * be[3] +
                                  r[8] * be[2] * be[3] + r[9] * be[3] * be[3]);
        }
        pnp_qr_solve(W);
        for (int i = 0; i < 4; ++i) be[i] = be[i] + W.gx[i];
    }
}

PNP_HD double pnp_dist2(const double *p1, const double *p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
PNP_HD double pnp_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// compute_L_6x10 (:760-800) and compute_rho (:802-810).  Serial.
PNP_HD void pnp_L_and_rho(PnpWs &W)
{
    int a = 0, b = 1;
    for (int j = 0; j < 6; ++j) {
        // dv[i][j] = v[i][3a ..] - v[i][3b ..], kept in W.ga as [4][3] for this j
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 3; ++k) W.ga[i * 3 + k] = W.v4[i * 12 + 3 * a + k] - W.v4[i * 12 + 3 * b + k];
        double *row = W.L + 10 * j;
        const double *d0 = W.ga, *d1 = W.ga + 3, *d2 = W.ga + 6, *d3 = W.ga + 9;
        row[0] = pnp_dot3(d0, d0);
        row[1] = 2.0 * pnp_dot3(d0, d1);
        row[2] = pnp_dot3(d1, d1);
        row[3] = 2.0 * pnp_dot3(d0, d2);
        row[4] = 2.0 * pnp_dot3(d1, d2);
        row[5] = pnp_dot3(d2, d2);
        row[6] = 2.0 * pnp_dot3(d0, d3);
        row[7] = 2.0 * pnp_dot3(d1, d3);
        row[8] = 2.0 * pnp_dot3(d2, d3);
        row[9] = pnp_dot3(d3, d3);
        b++;
        if (b > 3) { a++; b = a + 1; }
    }
    W.rho[0] = pnp_dist2(W.cws, W.cws + 3);
    W.rho[1] = pnp_dist2(W.cws, W.cws + 6);
    W.rho[2] = pnp_dist2(W.cws, W.cws + 9);
    W.rho[3] = pnp_dist2(W.cws + 3, W.cws + 6);
    W.rho[4] = pnp_dist2(W.cws + 3, W.cws + 9);
    W.rho[5] = pnp_dist2(W.cws + 6, W.cws + 9);
}

// compute_pose (:477-525) for the correspondences S by a team of TS lanes, this lane being tl.  W.n and W.first (the number
// of correspondences and the first of them) are set by the caller.  The pose lands in W.bestR / W.bestT.
template <int TS> PNP_HD void pnp_compute_pose(PnpWs &W, const PnpCorr &S, int tl)
{
    constexpr int JS = TS < 16 ? TS : 16;
    const double dn = (double)W.n;
    // choose_control_points: the centroid
    for (int s = tl; s < 3; s += TS) {
        double a = 0.0;
        PNP_FOR_CORR(S, k, e) a = a + (double)S.p3d[e * 3 + s];
        W.c0[s] = a / dn;
    }
    pnp_sync<TS>();
    for (int s = tl; s < 9; s += TS) {
        const int a = s / 3, b = s - 3 * a;
        double acc = 0.0;
        PNP_FOR_CORR(S, k, e) acc = acc + ((double)S.p3d[e * 3 + a] - W.c0[a]) * ((double)S.p3d[e * 3 + b] - W.c0[b]);
        W.A[s] = acc;
    }
    pnp_sync<TS>();
    if (tl < JS) pnp_jacobi_eig(W, 3, tl, JS);
    if (tl == 0) {
        for (int j = 0; j < 3; ++j) W.cws[j] = W.c0[j];
        for (int i = 1; i < 4; ++i) {
            const int o = W.order[i - 1];
            const double k = sqrt(W.w[o] / dn);
            // pca_sign: the component of largest magnitude (the first of equals) is made non-negative
            int b = 0;
            for (int j = 1; j < 3; ++j)
                if (fabs(W.V[j * 3 + o]) > fabs(W.V[b * 3 + o])) b = j;
            const bool neg = W.V[b * 3 + o] < 0;
            for (int j = 0; j < 3; ++j) W.cws[3 * i + j] = W.c0[j] + k * (neg ? -W.V[j * 3 + o] : W.V[j * 3 + o]);
        }
        // compute_barycentric_coordinates: cc_inv
        for (int i = 0; i < 3; ++i)
            for (int j = 1; j < 4; ++j) W.B[3 * i + j - 1] = W.cws[3 * j + i] - W.cws[i];
        pnp_svd_cols(W, 3, 3);
        const double fl = pnp_svd_floor(W, 3);
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 3; ++i) {
                double a = 0.0;
                for (int j = 0; j < 3; ++j)
                    if (sqrt(W.s2[j]) > fl) a = a + W.Vs[k * 3 + j] * (W.B[i * 3 + j] / W.s2[j]);
                W.ci[k * 3 + i] = a;
            }
    }
    pnp_sync<TS>();
    // M^T M, every entry by one lane
    for (int s = tl; s < 144; s += TS) {
        const int a = s / 12, b = s - 12 * a;
        double acc = 0.0;
        PNP_FOR_CORR(S, k, e) {
            double a0, a1, a2, a3, ma1, ma2, mb1, mb2;
            pnp_alphas(W, S, e, a0, a1, a2, a3);
            const double u = (double)S.p2d[e * 2], v = (double)S.p2d[e * 2 + 1];
            pnp_m_entry(S, a, a0, a1, a2, a3, u, v, ma1, ma2);
            pnp_m_entry(S, b, a0, a1, a2, a3, u, v, mb1, mb2);
            acc = acc + ma1 * mb1;
            acc = acc + ma2 * mb2;
        }
        W.A[s] = acc;
    }
    pnp_sync<TS>();
    if (tl < JS) pnp_jacobi_eig(W, 12, tl, JS);
    if (tl < JS)
        for (int s = tl; s < 48; s += JS) {
            const int i = s / 12, j = s - 12 * i;
            W.v4[s] = W.V[j * 12 + W.order[11 - i]];
        }
    pnp_sync<TS>();
    if (tl == 0) pnp_L_and_rho(W);
    for (int which = 1; which <= 3; ++which) {
        if (tl == 0) {
            pnp_find_betas(W, which);
            pnp_gauss_newton(W);
            // compute_ccs, and solve_for_sign on the first correspondence
            for (int j = 0; j < 12; ++j) W.ccs[j] = 0.0;
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 12; ++j) W.ccs[j] = W.ccs[j] + W.betas[i] * W.v4[i * 12 + j];
            double a0, a1, a2, a3;
            pnp_alphas(W, S, W.first, a0, a1, a2, a3);
            if (pnp_pc(W, 2, a0, a1, a2, a3) < 0.0)
                for (int j = 0; j < 12; ++j) W.ccs[j] = -W.ccs[j];
        }
        pnp_sync<TS>();
        // estimate_R_and_t: the two centroids
        for (int s = tl; s < 6; s += TS) {
            double acc = 0.0;
            if (s < 3) {
                PNP_FOR_CORR(S, k, e) {
                    double a0, a1, a2, a3;
                    pnp_alphas(W, S, e, a0, a1, a2, a3);
                    acc = acc + pnp_pc(W, s, a0, a1, a2, a3);
                }
                W.pc0[s] = acc / dn;
            } else {
                PNP_FOR_CORR(S, k, e) acc = acc + (double)S.p3d[e * 3 + s - 3];
                W.pw0[s - 3] = acc / dn;
            }
        }
        pnp_sync<TS>();
        for (int s = tl; s < 9; s += TS) {
            const int j = s / 3, c = s - 3 * j;
            double acc = 0.0;
            PNP_FOR_CORR(S, k, e) {
                double a0, a1, a2, a3;
                pnp_alphas(W, S, e, a0, a1, a2, a3);
                acc = acc + (pnp_pc(W, j, a0, a1, a2, a3) - W.pc0[j]) * ((double)S.p3d[e * 3 + c] - W.pw0[c]);
            }
            W.sums[s] = acc;
        }
        pnp_sync<TS>();
        if (tl == 0) {
            for (int s = 0; s < 9; ++s) W.B[s] = W.sums[s];
            pnp_svd_cols(W, 3, 3);
            double *R = W.R;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double a = 0.0;
                    for (int k = 0; k < 3; ++k) a = a + (W.B[i * 3 + k] / sqrt(W.s2[k])) * W.Vs[j * 3 + k];
                    R[i * 3 + j] = a;
                }
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                               R[0] * R[5] * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            for (int i = 0; i < 3; ++i) W.t[i] = W.pc0[i] - pnp_dot3(R + 3 * i, W.pw0);
        }
        pnp_sync<TS>();
        if (tl == 0) {
            // reprojection_error (:550-567)
            const double *R = W.R, *t = W.t;
            double sum2 = 0.0;
            PNP_FOR_CORR(S, k, e) {
                const double pw[3] = {(double)S.p3d[e * 3], (double)S.p3d[e * 3 + 1], (double)S.p3d[e * 3 + 2]};
                const double Xc = (R[0] * pw[0] + R[1] * pw[1] + R[2] * pw[2]) + t[0];
                const double Yc = (R[3] * pw[0] + R[4] * pw[1] + R[5] * pw[2]) + t[1];
                const double inv = 1.0 / ((R[6] * pw[0] + R[7] * pw[1] + R[8] * pw[2]) + t[2]);
                const double ue = S.uc + S.fu * Xc * inv, ve = S.vc + S.fv * Yc * inv;
                const double u = (double)S.p2d[e * 2], v = (double)S.p2d[e * 2 + 1];
                sum2 = sum2 + sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
            }
            const double err = sum2 / dn;
            // :518-520: N = 1, then 2 if its error is smaller, then 3 if smaller than the chosen one
            if (which == 1 || err < W.best_err) {
                W.best_err = err;
                for (int i = 0; i < 9; ++i) W.bestR[i] = R[i];
                for (int i = 0; i < 3; ++i) W.bestT[i] = t[i];
            }
        }
        pnp_sync<TS>();
    }
}

// CheckInliers (:308-339) for one correspondence under the pose R [9], t [3]
PNP_HD bool pnp_inlier(const double *R, const double *t, const float *X, const float *p, float max_err, double fu, double fv,
                       double uc, double vc)
{
    const double x = (double)X[0], y = (double)X[1], z = (double)X[2];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
    const float invZc = (float)(1.0 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
    const double ue = uc + fu * (double)Xc * (double)invZc;
    const double ve = vc + fv * (double)Yc * (double)invZc;
    const float dx = (float)((double)p[0] - ue), dy = (float)((double)p[1] - ve);
    const float e1 = dx * dx, e2 = dy * dy;
    const float err = e1 + e2;
    return err < max_err;
}

}  // namespace orbhip
