// Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) for one loop candidate, operation by operation what
// tests/seqref/sim3opt.py does: one Sim3 vertex, the pairs of EdgeSim3ProjectXYZ and
// EdgeInverseSim3ProjectXYZ with g2o's numeric Jacobian, g2o's Levenberg-Marquardt at dimension 7, a pivoted LDLt of the
// 7x7 system, g2o::Sim3 and the two rounds with the classification after each.  Everything is fp64, one rounding per
// operation (the library is built with -ffp-contract=off).  The same text serves a team of lanes on the device and one host
// thread, as orbhip_poseopt_core.h does; its helpers (det_sincos64, po_quat_*, po_cross, po_to_R) are used as they are.
//   - sum<FULL>: the 36 sums over the active pairs (28 of H, 7 of b, the robust chi2).  Pair j of the compacted list belongs
//     to lane j mod kS3oTeam, within a pair e12 comes before e21, a lane adds its pairs in ascending j, the lanes of a
//     wavefront meet in an xor butterfly (offsets 1 .. 32), the wavefronts are added in wavefront order.
//   - first / stride: how the per-pair loops and the 15 estimates of a linearisation are dealt out.
//   - is0 / sync: lane 0 runs the serial state machine over the workspace (LDS on the device), everyone else waits.
// The Levenberg-Marquardt rule, the 7x7 solver and the host replay of the team sum are orbhip_lm_core.h's, at dimension 7.
// Nothing here indexes a private array at run time.
#pragma once
#include "orbhip_poseopt_core.h"

namespace orbhip {

#ifndef ORBHIP_SIM3OPT_TEAM
#define ORBHIP_SIM3OPT_TEAM 256                         // 64 builds the one-wavefront team tools/bench_sim3opt.py measures against
#endif
constexpr int kS3oTeam = ORBHIP_SIM3OPT_TEAM;           // lanes of a team: part of the arithmetic, not of the launch
constexpr int kS3oWave = 64;
constexpr int kS3oSums = 36;
constexpr int kS3oCapMax = 4096;
constexpr double kS3oDelta = 1e-9;                      // base_binary_edge.hpp:147-148
constexpr double kS3oScalar = 1.0 / (2 * kS3oDelta);

// ---- det_exp64: fdlibm's __ieee754_exp with the thresholds written as doubles --------------------------------------------
constexpr double kExpOver = 7.09782712893383973096e+02, kExpUnder = -7.45133219101941108420e+02;
constexpr double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10, kInvLn2 = 1.44269504088896338700e+00;
constexpr double kExpP1 = 1.66666666666666019037e-01, kExpP2 = -2.77777777770155933842e-03, kExpP3 = 6.61375632143793436117e-05,
                 kExpP4 = -1.65339022054652515390e-06, kExpP5 = 4.13813679705723846039e-08;
constexpr double kHalfLn2 = 3.4657359027997264e-01, kThreeHalfLn2 = 1.0397207708399179e+00;
constexpr double kExpTiny = 3.7252902984619140625e-09;  // 2^-28
constexpr double kTwoM1000 = 9.33263618503218878990e-302;

PO_HD double det_exp64(double x)
{
    if (x != x) return x;
    if (x > kExpOver) return __builtin_inf();
    if (x < kExpUnder) return 0.0;
    double hi = 0.0, lo = 0.0;
    int k = 0;
    const double ax = fabs(x);
    if (ax > kHalfLn2) {
        if (ax < kThreeHalfLn2) {
            if (x < 0) { hi = x + kLn2Hi; lo = -kLn2Lo; k = -1; }
            else { hi = x - kLn2Hi; lo = kLn2Lo; k = 1; }
        } else {
            k = (int)(kInvLn2 * x + (x < 0 ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * kLn2Hi;
            lo = t * kLn2Lo;
        }
        x = hi - lo;
    } else if (ax < kExpTiny) {
        return 1.0 + x;
    }
    const double t = x * x;
    const double c = x - t * (kExpP1 + t * (kExpP2 + t * (kExpP3 + t * (kExpP4 + t * kExpP5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    if (k == 1024) return y * 2.0 * ldexp(1.0, 1023);
    if (k >= -1021) return y * ldexp(1.0, k);
    return y * ldexp(1.0, k + 1000) * kTwoM1000;
}

// ---- g2o::Sim3 (sim3.h): S[0..3] = quaternion (x, y, z, w), never normalised, S[4..6] = t, S[7] = s -------------------
// Sim3(toMatrix3d(R), toVector3d(t), s) of the [16] record orbhip_sim3_iterate_device writes: the floats widen to double
PO_HD void s3o_from_sim3(const float *m, double *S)
{
    const double R[9] = {(double)m[0], (double)m[1], (double)m[2], (double)m[3], (double)m[4], (double)m[5],
                         (double)m[6], (double)m[7], (double)m[8]};
    po_quat_from_R(R, S);
    S[4] = (double)m[9]; S[5] = (double)m[10]; S[6] = (double)m[11];
    S[7] = (double)m[12];
}
// Sim3(const Vector7d &update) (:70-142): u = (omega, upsilon, sigma)
PO_HD void s3o_exp(const double *u, double *S)
{
    const double sigma = u[6];
    const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double Om[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    double Om2[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    const double s = det_exp64(sigma);
    const double eps = 0.00001;
    double A, B, Cc, sn = 0.0, cs = 0.0;
    const bool small = theta < eps;
    if (small) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k];
    } else {
        det_sincos64(theta, sn, cs);
        const double a = sn / theta, b = (1.0 - cs) / (theta * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * Om[k]) + b * Om2[k];
    }
    if (fabs(sigma) < eps) {
        Cc = 1.0;
        if (small) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        Cc = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (Cc - ((b - 1.0) * sigma + a * theta) / c) / theta2;          // "* 1. / (theta2)": the product with 1 is exact
        }
    }
    po_quat_from_R(R, S);
    double Wm[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Wm[k] = (A * Om[k] + B * Om2[k]) + Cc * (k % 4 == 0 ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) S[4 + i] = (Wm[3 * i] * u[3] + Wm[3 * i + 1] * u[4]) + Wm[3 * i + 2] * u[5];
    S[7] = s;
}
// operator* (:266-272)
PO_HD void s3o_mul(const double *a, const double *b, double *o)
{
    double r[3];
    po_quat_rot(a, b + 4, r);
    po_quat_mul(a, b, o);
    o[4] = a[7] * r[0] + a[4]; o[5] = a[7] * r[1] + a[5]; o[6] = a[7] * r[2] + a[6];
    o[7] = a[7] * b[7];
}
// inverse (:233-236)
PO_HD void s3o_inverse(const double *S, double *o)
{
    o[0] = -S[0]; o[1] = -S[1]; o[2] = -S[2]; o[3] = S[3];
    const double m = -1. / S[7];
    const double v[3] = {m * S[4], m * S[5], m * S[6]};
    po_quat_rot(o, v, o + 4);
    o[7] = 1. / S[7];
}

// ---- the two edges (types_seven_dof_expmap.h:138-167) ---------------------------------------------------------------
struct S3oCam { double fx, fy, cx, cy; };
// obs - cam_map(project(S.map(X)))
PO_HD void s3o_error(const double *S, const double *X, const double *obs, const S3oCam &cam, double *e)
{
    double r[3];
    po_quat_rot(S, X, r);
    const double m0 = S[7] * r[0] + S[4], m1 = S[7] * r[1] + S[5], m2 = S[7] * r[2] + S[6];
    e[0] = obs[0] - (m0 / m2 * cam.fx + cam.cx);
    e[1] = obs[1] - (m1 / m2 * cam.fy + cam.cy);
}
PO_HD double s3o_chi2(const double *e, double inv)
{
    double chi2 = 0.0;
    chi2 = chi2 + e[0] * (inv * e[0]);
    chi2 = chi2 + e[1] * (inv * e[1]);
    return chi2;
}
// RobustKernelHuber::robustify; returns rho[0]
PO_HD double s3o_huber(double chi2, double delta, double dsqr, double &rho1)
{
    rho1 = 1.0;
    if (chi2 <= dsqr) return chi2;
    const double s = sqrt(chi2);
    rho1 = delta / s;
    return 2 * s * delta - dsqr;
}

struct S3oPair { double P1[3], P2[3], o1[2], o2[2], inv1, inv2; };

// adds the 36 terms of one edge to acc: 28 of H (upper triangle, row by row), 7 of b, rho[0].  E [15][8]: the estimates of
// this linearisation as the edge sees them (2d, 2d + 1: Sim3(+-delta e_d) * estimate, 14: the estimate), for e21 their inverses
PO_HD void s3o_edge_terms(const double (*E)[8], const double *X, const double *obs, double inv, const S3oCam &cam, double delta,
                          double dsqr, double *acc)
{
    double e[2], ep[2], em[2], J0[7], J1[7], rho1;
    s3o_error(E[14], X, obs, cam, e);
    const double rho0 = s3o_huber(s3o_chi2(e, inv), delta, dsqr, rho1);
    acc[35] = acc[35] + rho0;
#pragma unroll
    for (int k = 0; k < 7; ++k) { J0[k] = 0.0; J1[k] = 0.0; }
    // the loop over the columns stays rolled (the estimates come from the workspace one pair at a time); a column found at
    // run time is stored by comparing it with each position in turn
#pragma unroll 1
    for (int d = 0; d < 7; ++d) {
        s3o_error(E[2 * d], X, obs, cam, ep);
        s3o_error(E[2 * d + 1], X, obs, cam, em);
        const double j0 = kS3oScalar * (ep[0] - em[0]), j1 = kS3oScalar * (ep[1] - em[1]);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            J0[k] = k == d ? j0 : J0[k];
            J1[k] = k == d ? j1 : J1[k];
        }
    }
    const double w = rho1 * inv;
    const double we0 = w * e[0], we1 = w * e[1];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = a; b < 7; ++b) {
            double s = 0.0;
            s = s + (J0[a] * w) * J0[b];
            s = s + (J1[a] * w) * J1[b];
            acc[k] = acc[k] + s;
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        double s = 0.0;
        s = s + J0[a] * we0;
        s = s + J1[a] * we1;
        acc[28 + a] = acc[28 + a] + -s;
    }
}
// a trial: rho[0] of both edges at the estimate S and its inverse Si
PO_HD void s3o_pair_chi(const S3oPair &p, const double *S, const double *Si, const S3oCam &cam, double delta, double dsqr, double *acc)
{
    double e[2], rho1;
    s3o_error(S, p.P2, p.o1, cam, e);
    acc[35] = acc[35] + s3o_huber(s3o_chi2(e, p.inv1), delta, dsqr, rho1);
    s3o_error(Si, p.P1, p.o2, cam, e);
    acc[35] = acc[35] + s3o_huber(s3o_chi2(e, p.inv2), delta, dsqr, rho1);
}

// ---- the workspace of one candidate (LDS on the device) ---------------------------------------------------------------
struct S3oWs {
    double part[kS3oTeam / kS3oWave][kS3oSums];   // the wavefront sums on their way to the team sum
    double E[15][8], Ei[15][8];                   // the estimates of a linearisation and their inverses
    double H[49], b[7], x[7], A[49];
    double est[8], einv[8], tried[8], tinv[8], backup[8], est0[8];
    double lam, ni, current, ini, rho;
    int n_bad_lm, qmax, it, its, again, stop;
    int ne, cnt[2];
};

// ---- OptimizationAlgorithmLevenberg::solve at dimension 7, cut where the team has to sum ---------------------------------
PO_HD void s3o_lm_begin(S3oWs &W, const double *s)
{
    int k = 0;
    for (int a = 0; a < 7; ++a)
        for (int b = a; b < 7; ++b) { W.H[a * 7 + b] = s[k]; W.H[b * 7 + a] = s[k]; ++k; }
    for (int a = 0; a < 7; ++a) W.b[a] = s[28 + a];
    lm_begin(W, s[35], W.it == 0 ? 1e-5 * lm_max_diag<7>(W.H) : 0.0);
}
// push, setLambda, solve, oplus; returns ok2.  VertexSim3Expmap::oplusImpl zeroes update[6] in the solver's own vector
PO_HD bool s3o_lm_step(S3oWs &W, bool fix_scale)
{
    for (int k = 0; k < 8; ++k) W.backup[k] = W.est[k];
    for (int k = 0; k < 49; ++k) W.A[k] = W.H[k];
    for (int j = 0; j < 7; ++j) W.A[j * 7 + j] = W.H[j * 7 + j] + W.lam;
    const bool ok2 = ldlt_solve_small<7>(W.A, W.b, W.x);                       // a failure leaves the stale x
    if (fix_scale) W.x[6] = 0.0;
    double u[7], e[8], d[8], o[8], oi[8];
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = W.x[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = W.est[k];
    s3o_exp(u, d);
    s3o_mul(d, e, o);
    s3o_inverse(o, oi);
#pragma unroll
    for (int k = 0; k < 8; ++k) { W.est[k] = o[k]; W.tried[k] = o[k]; W.einv[k] = oi[k]; W.tinv[k] = oi[k]; }
    return ok2;
}
PO_HD void s3o_lm_judge(S3oWs &W, bool ok2, double temp)
{
    if (!lm_gain(W, ok2, temp, lm_scale<7>(W.x, W.b, W.lam)))
        for (int k = 0; k < 8; ++k) W.est[k] = W.backup[k];
    W.again = lm_retry(W);
    if (W.again) return;
    W.its = W.its + 1;
    W.stop = lm_iteration_ok(W) ? 0 : 1;
}

// ---- one candidate --------------------------------------------------------------------------------------------------
// the tables of orbhip_sim3_tables the skip rules read
struct S3oTables {
    const int *slot_point, *n, *obs_start, *obs_kf, *obs_idx;
    const uint8_t *flags;
    int rows, cap, np, cur, match_form;
};
struct S3oCand {
    const orbhip_keypoint *kps_cur, *kps_kf;    // [cap]: the rows of the current key frame and of the candidate
    const int *sp_cur;                          // [cap]: slot_point of the current key frame
    const float *world;                         // [pcap][3]
    const float *T1, *T2;                       // [12]: Tcw of the current key frame and of the candidate
    const float *inv_sigma2;                    // [n_levels]
    const float *sim3;                          // [16]
    int *matched;                               // [cap] in/out
    double *S12;                                // [8]
    float *Scw;                                 // [12] or nullptr
    int *report;                                // [8]
    uint16_t *e_slot, *e_i2;                    // [cap] the compacted pair list: slot of cur, point and slot of the candidate,
    int *e_p2;                                  //       removed flag
    uint8_t *e_out;
    int n_levels, fix_scale;
    S3oCam cam;
    double delta, dsqr, th2;
};

// MapPoint::GetIndexInKeyFrame: the first entry of the point's list that names the row
PO_HD int s3o_index_in_key_frame(const S3oTables &T, int p, int row)
{
    const int o1 = T.obs_start[p + 1];
    for (int o = T.obs_start[p]; o < o1; ++o)
        if (T.obs_kf[o] == row) return T.obs_idx[o];
    return -1;
}
// :1099-1136 for slot i of the current key frame with the entry m of vpMatches1: the candidate's point and its slot
PO_HD bool s3o_keep(const S3oTables &T, int kf, int i, int m, int &p2, int &i2)
{
    if (m < 0) return false;
    p2 = T.match_form == ORBHIP_SIM3_MATCH_SLOTS ? (m < T.cap ? T.slot_point[(size_t)kf * T.cap + m] : -1) : m;
    const int p1 = T.slot_point[(size_t)T.cur * T.cap + i];
    if (!((unsigned)p1 < (unsigned)T.np && (unsigned)p2 < (unsigned)T.np)) return false;
    if (!(T.flags[p1] & ORBHIP_POINT_PRESENT) || !(T.flags[p2] & ORBHIP_POINT_PRESENT)) return false;
    i2 = s3o_index_in_key_frame(T, p2, kf);
    return (unsigned)i2 < (unsigned)T.cap;
}

// one row of a cv::Mat product R X + t: fp64 accumulation, one rounding to float
PO_HD float s3o_row_dot(const float *T, const float *X)
{
    const double d = ((double)T[0] * (double)X[0] + (double)T[1] * (double)X[1]) + (double)T[2] * (double)X[2];
    return (float)(d + (double)T[3]);
}
PO_HD int s3o_level(const S3oCand &F, int octave)
{
    return octave < 0 ? 0 : (octave >= F.n_levels ? F.n_levels - 1 : octave);
}
PO_HD void s3o_load_pair(const S3oCand &F, int j, S3oPair &p)
{
    const int slot = F.e_slot[j], i2 = F.e_i2[j];
    const float *W1 = F.world + (size_t)F.sp_cur[slot] * 3, *W2 = F.world + (size_t)F.e_p2[j] * 3;
    const orbhip_keypoint k1 = F.kps_cur[slot], k2 = F.kps_kf[i2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p.P1[r] = (double)s3o_row_dot(F.T1 + 4 * r, W1);
        p.P2[r] = (double)s3o_row_dot(F.T2 + 4 * r, W2);
    }
    p.o1[0] = (double)k1.x; p.o1[1] = (double)k1.y;
    p.o2[0] = (double)k2.x; p.o2[1] = (double)k2.y;
    p.inv1 = (double)F.inv_sigma2[s3o_level(F, k1.octave)];
    p.inv2 = (double)F.inv_sigma2[s3o_level(F, k2.octave)];
}

// estimate number d of a linearisation (base_binary_edge.hpp:157-173): 2c, 2c + 1 = Sim3(+-delta e_c) * estimate, 14 = the
// estimate; and its inverse.  oplusImpl zeroes update[6] when the scale is fixed
PO_HD void s3o_perturbed(S3oWs &W, int d, bool fix_scale)
{
    double e[8], o[8], oi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = W.est[k];
    if (d < 14) {
        const int c = d >> 1;
        const double v = (d & 1) ? -kS3oDelta : kS3oDelta;
        double u[7], s[8];
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = k == c ? v : 0.0;
        if (fix_scale) u[6] = 0.0;
        s3o_exp(u, s);
        s3o_mul(s, e, o);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = e[k];
    }
    s3o_inverse(o, oi);
#pragma unroll
    for (int k = 0; k < 8; ++k) { W.E[d][k] = o[k]; W.Ei[d][k] = oi[k]; }
}

// SparseOptimizer::optimize(max_it) from W.est; leaves W.est and W.tried (with W.tinv).  W.est was written before a sync.
template <class Team> PO_HD void s3o_optimize(Team &tm, S3oWs &W, const S3oCand &F, int max_it)
{
    for (int it = 0; it < max_it; ++it) {
        for (int d = tm.first(); d < 15; d += tm.stride()) s3o_perturbed(W, d, F.fix_scale != 0);
        tm.sync();
        double s[kS3oSums];
        tm.template sum<true>(W, F, s);
        bool ok2 = false;
        if (tm.is0()) { W.it = it; s3o_lm_begin(W, s); }
        do {
            if (tm.is0()) ok2 = s3o_lm_step(W, F.fix_scale != 0);
            tm.sync();
            tm.template sum<false>(W, F, s);
            if (tm.is0()) s3o_lm_judge(W, ok2, s[35]);
            tm.sync();
        } while (W.again);
        if (W.stop) break;
    }
}

// The check after a round (:1186-1203, :1220-1234) over this lane's pairs; returns how many it removed.  chi2() reads the
// _error of the last computeActiveErrors, i.e. at W.tried, the last TRIED estimate, accepted or not.  The comparison is a
// double against the widened float, strict; a NaN is not greater.  A removed pair has its entry of vpMatches1 nulled.
template <class Team> PO_HD int s3o_classify(Team &tm, const S3oWs &W, const S3oCand &F, int ne)
{
    double tried[8], tinv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { tried[k] = W.tried[k]; tinv[k] = W.tinv[k]; }
    int bad = 0;
    for (int j = tm.first(); j < ne; j += tm.stride()) {
        if (F.e_out[j]) continue;
        S3oPair p;
        s3o_load_pair(F, j, p);
        double e12[2], e21[2];
        s3o_error(tried, p.P2, p.o1, F.cam, e12);
        s3o_error(tinv, p.P1, p.o2, F.cam, e21);
        if (s3o_chi2(e12, p.inv1) > F.th2 || s3o_chi2(e21, p.inv2) > F.th2) {
            F.e_out[j] = 1;
            F.matched[F.e_slot[j]] = -1;
            ++bad;
        }
    }
    return bad;
}

// The function.  F.e_* hold the compacted pairs, W.ne their number, e_out is zero, W.cnt is zero; all of it behind a sync.
template <class Team> PO_HD void s3o_run(Team &tm, S3oWs &W, const S3oCand &F)
{
    const int ne = W.ne;
    if (tm.is0()) {
        double e[8], ei[8];
        s3o_from_sim3(F.sim3, e);
        s3o_inverse(e, ei);
        for (int k = 0; k < 8; ++k) { W.est0[k] = e[k]; W.est[k] = e[k]; W.tried[k] = e[k]; W.einv[k] = ei[k]; W.tinv[k] = ei[k]; }
        for (int k = 0; k < 7; ++k) W.x[k] = 0.0;
        W.its = 0;
        W.again = 0; W.stop = 0;
    }
    tm.sync();
    int n_bad = 0, its1 = 0, its2 = 0, n_in = 0, status = ORBHIP_SIM3OPT_OK;
    if (ne > 0) {
        s3o_optimize(tm, W, F, 5);                                             // :1182
        its1 = W.its;
        const int bad = s3o_classify(tm, W, F, ne);
        tm.add(&W.cnt[0], bad);
        tm.sync();
        n_bad = W.cnt[0];
    }
    if (ne - n_bad < 10) {                                                     // :1211: g2oS12 stays what it was
        status = ORBHIP_SIM3OPT_TOO_FEW;
        if (tm.is0())
            for (int k = 0; k < 8; ++k) F.S12[k] = W.est0[k];
    } else {
        if (tm.is0()) W.its = 0;
        tm.sync();
        s3o_optimize(tm, W, F, n_bad > 0 ? 10 : 5);                            // :1205-1217
        its2 = W.its;
        const int bad = s3o_classify(tm, W, F, ne);
        tm.add(&W.cnt[1], bad);
        tm.sync();
        n_in = ne - n_bad - W.cnt[1];
        if (tm.is0()) {
            for (int k = 0; k < 8; ++k) F.S12[k] = W.est[k];
            if (F.Scw) {                                                       // src/LoopClosing.cc:333-335
                double mw[8], e[8], cw[8], R[9];
                const double R2[9] = {(double)F.T2[0], (double)F.T2[1], (double)F.T2[2], (double)F.T2[4], (double)F.T2[5],
                                      (double)F.T2[6], (double)F.T2[8], (double)F.T2[9], (double)F.T2[10]};
                po_quat_from_R(R2, mw);
                mw[4] = (double)F.T2[3]; mw[5] = (double)F.T2[7]; mw[6] = (double)F.T2[11]; mw[7] = 1.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) e[k] = W.est[k];
                s3o_mul(e, mw, cw);
                po_to_R(cw, R);
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) F.Scw[r * 4 + c] = (float)(cw[7] * R[r * 3 + c]);
                    F.Scw[r * 4 + 3] = (float)cw[4 + r];
                }
            }
        }
    }
    if (tm.is0()) {
        F.report[0] = status; F.report[1] = ne; F.report[2] = n_bad; F.report[3] = n_in;
        F.report[4] = its1; F.report[5] = its2; F.report[6] = 0; F.report[7] = 0;
    }
}

// ---- the host team: one thread that replays the device team's order ----------------------------------------------------
struct S3oHostTeam : HostTeam {
    template <bool FULL> void sum(S3oWs &W, const S3oCand &F, double *s)
    {
        static thread_local double lanes[kS3oTeam][kS3oSums];
        for (int l = 0; l < kS3oTeam; ++l)
            for (int k = 0; k < kS3oSums; ++k) lanes[l][k] = 0.0;
        for (int j = 0; j < W.ne; ++j) {
            if (F.e_out[j]) continue;
            S3oPair p;
            s3o_load_pair(F, j, p);
            double *acc = lanes[j % kS3oTeam];
            if (FULL) {
                s3o_edge_terms(W.E, p.P2, p.o1, p.inv1, F.cam, F.delta, F.dsqr, acc);
                s3o_edge_terms(W.Ei, p.P1, p.o2, p.inv2, F.cam, F.delta, F.dsqr, acc);
            } else {
                s3o_pair_chi(p, W.est, W.einv, F.cam, F.delta, F.dsqr, acc);
            }
        }
        host_team_combine<kS3oTeam, kS3oSums>(lanes, FULL ? 0 : kS3oSums - 1, s, TeamAdd());
    }
};

// compaction on the host: the kept slots i < n[cur] in slot order (:1099-1178)
inline void s3o_host_compact(S3oWs &W, const S3oTables &T, int kf, const S3oCand &F)
{
    int ne = 0;
    const int n1 = T.n[T.cur] < 0 ? 0 : (T.n[T.cur] > T.cap ? T.cap : T.n[T.cur]);
    if ((unsigned)kf < (unsigned)T.rows)
        for (int i = 0; i < n1; ++i) {
            int p2 = -1, i2 = -1;
            if (!s3o_keep(T, kf, i, F.matched[i], p2, i2)) continue;
            F.e_slot[ne] = (uint16_t)i; F.e_p2[ne] = p2; F.e_i2[ne] = (uint16_t)i2; F.e_out[ne] = 0;
            ++ne;
        }
    W.ne = ne;
    W.cnt[0] = W.cnt[1] = 0;
}

}  // namespace orbhip
