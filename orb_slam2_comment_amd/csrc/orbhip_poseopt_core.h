// Optimizer::PoseOptimization (src/Optimizer.cc:239-451) for one frame, operation by operation what tests/seqref/poseopt.py
// does: the two only-pose edges, g2o's Levenberg-Marquardt, a pivoted LDLt of the 6x6 system, SE3Quat,
// the four rounds and the loops of Tracking that follow the call.  Everything is fp64, one rounding per operation (the
// library is built with -ffp-contract=off).  The same text serves a team of lanes on the device and one host thread; what
// differs is the Team the driver is given:
//   - sum<FULL>: the 28 sums over the active edges (21 of H, 6 of b, the robust chi2).  Edge j of the compacted list belongs
//     to lane j mod kPoTeam, a lane adds its edges in ascending j, the lanes of a wavefront meet in an xor butterfly
//     (offsets 1 .. 32), the wavefronts are added in wavefront order.  The host team replays exactly that.
//   - first / stride: how the per-edge loops (classification, epilogue) are dealt out; they carry integers only.
//   - is0 / sync: lane 0 runs the serial state machine over the workspace (LDS on the device), everyone else waits.
// The Levenberg-Marquardt rule, the 6x6 solver and the host replay of the team sum are orbhip_lm_core.h's; what is here
// around them is the function's own: the H and b of the 28 sums, the backup of the estimate, the counters.
// Nothing here indexes a private array at run time.
#pragma once
#include <cmath>
#include <cstdint>

#include "orbhip.h"
#include "orbhip_lm_core.h"

namespace orbhip {

#ifndef ORBHIP_POSEOPT_TEAM
#define ORBHIP_POSEOPT_TEAM 256                         // 64 builds the one-wavefront team tools/bench_poseopt.py measures against
#endif
constexpr int kPoTeam = ORBHIP_POSEOPT_TEAM;            // lanes of a team: part of the arithmetic, not of the launch
constexpr int kPoWave = 64;

// ---- det_sincos64: fdlibm's __kernel_sin / __kernel_cos, a three-part Cody-Waite reduction ----------------------------
constexpr double kS1 = -1.66666666666666324348e-01, kS2 = 8.33333333332248946124e-03, kS3 = -1.98412698298579493134e-04,
                 kS4 = 2.75573137070700676789e-06, kS5 = -2.50507602534068634195e-08, kS6 = 1.58969099521155010221e-10;
constexpr double kC1 = 4.16666666666666019037e-02, kC2 = -1.38888888888741095749e-03, kC3 = 2.48015872894767294178e-05,
                 kC4 = -2.75573143513906633035e-07, kC5 = 2.08757232129817482790e-09, kC6 = -1.13596475577881948265e-11;
constexpr double kInvPio2 = 6.36619772367581382433e-01, kPio2_1 = 1.57079632673412561417e+00,
                 kPio2_1t = 6.07710050650619224932e-11, kPio2_2 = 6.07710050630396597660e-11,
                 kPio2_2t = 2.02226624879595063154e-21, kPio2_3 = 2.02226624871116645580e-21,
                 kPio2_3t = 8.47842766036889956997e-32, kPio4 = 7.85398163397448278999e-01;
constexpr double kSincosRange = 1647099.0;              // 2^20 * pi / 2: fn * kPio2_1 is exact below it

PO_HD double po_kernel_sin(double x, double y)
{
    const double z = x * x, v = z * x;
    const double r = kS2 + z * (kS3 + z * (kS4 + z * (kS5 + z * kS6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * kS1);
}
PO_HD double po_kernel_cos(double x, double y)
{
    const double z = x * x;
    double w = z * z;
    const double r = z * (kC1 + z * (kC2 + z * kC3)) + (w * w) * (kC4 + z * (kC5 + z * kC6));
    const double hz = 0.5 * z;
    w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * y));
}
// |x| <= pi/4: the kernels; up to kSincosRange: three Cody-Waite steps; beyond, or NaN: NaN, NaN
PO_HD void det_sincos64(double x, double &s, double &c)
{
    if (!(fabs(x) <= kSincosRange)) { s = c = __builtin_nan(""); return; }
    if (fabs(x) <= kPio4) { s = po_kernel_sin(x, 0.0); c = po_kernel_cos(x, 0.0); return; }
    const double fn = floor(x * kInvPio2 + 0.5);
    double r = x - fn * kPio2_1;
    double w = fn * kPio2_1t;
    double t = r;
    w = fn * kPio2_2;
    r = t - w;
    w = fn * kPio2_2t - ((t - r) - w);
    t = r;
    w = fn * kPio2_3;
    r = t - w;
    w = fn * kPio2_3t - ((t - r) - w);
    const double y0 = r - w, y1 = (r - y0) - w;
    const double ks = po_kernel_sin(y0, y1), kc = po_kernel_cos(y0, y1);
    const int q = (int)fn & 3;
    if (q == 0) { s = ks; c = kc; }
    else if (q == 1) { s = kc; c = -ks; }
    else if (q == 2) { s = -ks; c = -kc; }
    else { s = -kc; c = ks; }
}

// ---- SE3Quat: p[0..3] = quaternion (x, y, z, w), p[4..6] = translation ------------------------------------------------
PO_HD void po_cross(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
PO_HD void po_quat_case(double rii, double rjj, double rkk, double rkj, double rjk, double rji, double rij, double rki, double rik,
                        double &qi, double &qj, double &qk, double &w)
{
    double t = sqrt(rii - rjj - rkk + 1.0);
    qi = 0.5 * t;
    t = 0.5 / t;
    qj = (rji + rij) * t;
    qk = (rki + rik) * t;
    w = (rkj - rjk) * t;
}
// Eigen's Quaterniond(Matrix3d), R row-major
PO_HD void po_quat_from_R(const double *R, double *q)
{
    double t = (R[0] + R[4]) + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
        return;
    }
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i ? R[4] : R[0])) i = 2;
    if (i == 0) po_quat_case(R[0], R[4], R[8], R[7], R[5], R[3], R[1], R[6], R[2], q[0], q[1], q[2], q[3]);
    else if (i == 1) po_quat_case(R[4], R[8], R[0], R[2], R[6], R[7], R[5], R[1], R[3], q[1], q[2], q[0], q[3]);
    else po_quat_case(R[8], R[0], R[4], R[3], R[1], R[2], R[6], R[5], R[7], q[2], q[0], q[1], q[3]);
}
PO_HD void po_normalize(double *q)
{
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
PO_HD void po_quat_mul(const double *a, const double *b, double *o)
{
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
PO_HD void po_quat_rot(const double *q, const double *v, double *o)
{
    double uv[3], c[3];
    po_cross(q, v, uv);
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    po_cross(q, uv, c);
    o[0] = v[0] + q[3] * uv[0] + c[0];
    o[1] = v[1] + q[3] * uv[1] + c[1];
    o[2] = v[2] + q[3] * uv[2] + c[2];
}
PO_HD void po_to_R(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// Converter::toSE3Quat: the floats widen to double
PO_HD void po_pose_from_Tcw(const float *T, double *p)
{
    const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6],
                         (double)T[8], (double)T[9], (double)T[10]};
    po_quat_from_R(R, p);
    po_normalize(p);
    p[4] = (double)T[3]; p[5] = (double)T[7]; p[6] = (double)T[11];
}
// SE3Quat::exp (se3quat.h:223-257): u = (omega, upsilon)
PO_HD void po_se3_exp(const double *u, double *p)
{
    const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double Om[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    double Om2[9], R[9], V[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    if (theta < 0.00001) {
        // "TODO: CHECK WHETHER THIS IS CORRECT!!!" -- as written
#pragma unroll
        for (int k = 0; k < 9; ++k) { R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k]; V[k] = R[k]; }
    } else {
        double s, c;
        det_sincos64(theta, s, c);
        const double a = s / theta, b = (1.0 - c) / (theta * theta), d = (theta - s) / (theta * theta * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double I = k % 4 == 0 ? 1.0 : 0.0;
            R[k] = (I + a * Om[k]) + b * Om2[k];
            V[k] = (I + b * Om[k]) + d * Om2[k];
        }
    }
    po_quat_from_R(R, p);
    po_normalize(p);
#pragma unroll
    for (int i = 0; i < 3; ++i) p[4 + i] = (V[3 * i] * u[3] + V[3 * i + 1] * u[4]) + V[3 * i + 2] * u[5];
}
// SE3Quat::operator* (:104-110)
PO_HD void po_se3_mul(const double *a, const double *b, double *o)
{
    double r[3];
    po_quat_rot(a, b + 4, r);
    po_quat_mul(a, b, o);
    po_normalize(o);
    o[4] = a[4] + r[0]; o[5] = a[5] + r[1]; o[6] = a[6] + r[2];
}

// ---- edges ---------------------------------------------------------------------------------------------------------
struct PoEdge {
    double X[3], obs[3], inv, delta, dsqr;
    float thr;
    bool stereo;
};
struct PoCam {
    double fx, fy, cx, cy, bf;
    double delta_mono, delta_stereo;        // (float)sqrt(5.991), (float)sqrt(7.815), widened
};

// computeError and chi2; P = the point in the camera frame
PO_HD double po_edge_error(const PoEdge &e, const double *pose, const PoCam &cam, double *err, double *P)
{
    double r[3];
    po_quat_rot(pose, e.X, r);
    P[0] = r[0] + pose[4]; P[1] = r[1] + pose[5]; P[2] = r[2] + pose[6];
    double chi2 = 0.0;
    if (e.stereo) {
        const double invz = (double)(float)(1.0 / P[2]);                      // types_six_dof_expmap.cpp:300: a float
        const double p0 = P[0] * invz * cam.fx + cam.cx, p1 = P[1] * invz * cam.fy + cam.cy;
        err[0] = e.obs[0] - p0;
        err[1] = e.obs[1] - p1;
        err[2] = e.obs[2] - (p0 - cam.bf * invz);
        chi2 = chi2 + err[0] * (e.inv * err[0]);
        chi2 = chi2 + err[1] * (e.inv * err[1]);
        chi2 = chi2 + err[2] * (e.inv * err[2]);
    } else {
        err[0] = e.obs[0] - (P[0] / P[2] * cam.fx + cam.cx);
        err[1] = e.obs[1] - (P[1] / P[2] * cam.fy + cam.cy);
        err[2] = 0.0;
        chi2 = chi2 + err[0] * (e.inv * err[0]);
        chi2 = chi2 + err[1] * (e.inv * err[1]);
    }
    return chi2;
}

// adds the 28 terms of one edge to acc: 21 of H (upper triangle, row by row), 6 of b, rho[0]
template <bool FULL> PO_HD void po_edge_terms(const PoEdge &e, const double *pose, const PoCam &cam, bool kernel, double *acc)
{
    double err[3], P[3];
    const double chi2 = po_edge_error(e, pose, cam, err, P);
    double rho0 = chi2, rho1 = 1.0;
    if (kernel && !(chi2 <= e.dsqr)) {                                        // RobustKernelHuber::robustify
        const double s = sqrt(chi2);
        rho0 = 2 * s * e.delta - e.dsqr;
        rho1 = e.delta / s;
    }
    acc[27] = acc[27] + rho0;
    if (!FULL) return;
    const double x = P[0], y = P[1], invz = 1.0 / P[2], invz_2 = invz * invz, fx = cam.fx, fy = cam.fy, bf = cam.bf;
    double J0[6], J1[6], J2[6];
    J0[0] = x * y * invz_2 * fx; J0[1] = -(1 + (x * x * invz_2)) * fx; J0[2] = y * invz * fx;
    J0[3] = -invz * fx; J0[4] = 0.0; J0[5] = x * invz_2 * fx;
    J1[0] = (1 + y * y * invz_2) * fy; J1[1] = -x * y * invz_2 * fy; J1[2] = -x * invz * fy;
    J1[3] = 0.0; J1[4] = -invz * fy; J1[5] = y * invz_2 * fy;
    J2[0] = J0[0] - bf * y * invz_2; J2[1] = J0[1] + bf * x * invz_2; J2[2] = J0[2];
    J2[3] = J0[3]; J2[4] = 0.0; J2[5] = J0[5] - bf * invz_2;
    const double w = rho1 * e.inv;
    const double we0 = w * err[0], we1 = w * err[1], we2 = w * err[2];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double s = 0.0;
            s = s + (J0[a] * w) * J0[b];
            s = s + (J1[a] * w) * J1[b];
            if (e.stereo) s = s + (J2[a] * w) * J2[b];
            acc[k] = acc[k] + s;
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        s = s + J0[a] * we0;
        s = s + J1[a] * we1;
        if (e.stereo) s = s + J2[a] * we2;
        acc[21 + a] = acc[21 + a] + -s;
    }
}

// ---- the workspace of one frame (LDS on the device) -------------------------------------------------------------------
struct PoWs {
    double part[kPoTeam / kPoWave][28];     // the wavefront sums on their way to the team sum
    double H[36], b[6], x[6], A[36];
    double est[7], tried[7], backup[7], pose0[7];
    double lam, ni, current, ini, rho;
    int n_bad_lm, qmax, it, its_total, again, stop;
    int ne, cnt[3];
};

// ---- OptimizationAlgorithmLevenberg::solve, cut where the team has to sum ----------------------------------------------
// after the sums at the estimate (:75-97)
PO_HD void po_lm_begin(PoWs &W, const double *s)
{
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { W.H[a * 6 + b] = s[k]; W.H[b * 6 + a] = s[k]; ++k; }
    for (int a = 0; a < 6; ++a) W.b[a] = s[21 + a];
    lm_begin(W, s[27], W.it == 0 ? 1e-5 * lm_max_diag<6>(W.H) : 0.0);
}
// push, setLambda, solve, update (:103-121); returns ok2
PO_HD bool po_lm_step(PoWs &W)
{
    for (int k = 0; k < 7; ++k) W.backup[k] = W.est[k];
    for (int k = 0; k < 36; ++k) W.A[k] = W.H[k];
    for (int j = 0; j < 6; ++j) W.A[j * 6 + j] = W.H[j * 6 + j] + W.lam;
    const bool ok2 = ldlt_solve_small<6>(W.A, W.b, W.x);                       // a failure leaves the stale x
    double u[6], e[7], d[7], o[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = W.x[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) e[k] = W.est[k];
    po_se3_exp(u, d);
    po_se3_mul(d, e, o);
#pragma unroll
    for (int k = 0; k < 7; ++k) { W.est[k] = o[k]; W.tried[k] = o[k]; }
    return ok2;
}
// :123-163 with the trial's chi2; sets W.again (another trial) and, when the iteration ends, W.stop (optimize() ends)
PO_HD void po_lm_judge(PoWs &W, bool ok2, double temp)
{
    if (!lm_gain(W, ok2, temp, lm_scale<6>(W.x, W.b, W.lam)))
        for (int k = 0; k < 7; ++k) W.est[k] = W.backup[k];
    W.again = lm_retry(W);
    if (W.again) return;
    W.its_total = W.its_total + 1;
    W.stop = lm_iteration_ok(W) ? 0 : 1;
}

// ---- one frame -----------------------------------------------------------------------------------------------------
struct PoFrame {
    const orbhip_keypoint *kps;             // [cap]
    const float *u_right;                   // [cap] or nullptr
    const float *world;                     // the frame's world row [pcap][3]
    const uint8_t *pflags;                  // [pcap] or nullptr
    const float *inv_sigma2;                // [n_levels]
    float *Tcw;                             // [12]
    int *frame_point;                       // [cap]
    uint8_t *outlier;                       // [cap]
    int *discarded;                         // [cap] or nullptr
    int *report;                            // [8]
    uint16_t *e_slot;                       // [cap] the compacted edge list: slot, point, outlier flag (level 1)
    int *e_pt;
    uint8_t *e_out;
    int n, pcap, n_levels, mode, flags;
    PoCam cam;
};

PO_HD void po_load_edge(const PoFrame &F, int j, PoEdge &e)
{
    const int slot = F.e_slot[j], p = F.e_pt[j];
    const orbhip_keypoint kp = F.kps[slot];
    const float ur = F.u_right ? F.u_right[slot] : -1.f;
    e.stereo = !(ur < 0);                                                      // :286
    e.X[0] = (double)F.world[(size_t)p * 3]; e.X[1] = (double)F.world[(size_t)p * 3 + 1]; e.X[2] = (double)F.world[(size_t)p * 3 + 2];
    e.obs[0] = (double)kp.x; e.obs[1] = (double)kp.y; e.obs[2] = (double)ur;
    const int lv = kp.octave < 0 ? 0 : (kp.octave >= F.n_levels ? F.n_levels - 1 : kp.octave);
    e.inv = (double)F.inv_sigma2[lv];
    e.delta = e.stereo ? F.cam.delta_stereo : F.cam.delta_mono;
    e.dsqr = e.delta * e.delta;
    e.thr = e.stereo ? 7.815f : 5.991f;
}

// SparseOptimizer::optimize(10) from W.est; leaves W.est and W.tried.  W.est was written before a sync.
template <class Team> PO_HD void po_optimize(Team &tm, PoWs &W, const PoFrame &F, bool kernel)
{
    for (int it = 0; it < 10; ++it) {
        double s[28];
        tm.template sum<true>(W, F, kernel, s);
        bool ok2 = false;
        if (tm.is0()) { W.it = it; po_lm_begin(W, s); }
        do {
            if (tm.is0()) ok2 = po_lm_step(W);
            tm.sync();
            tm.template sum<false>(W, F, kernel, s);
            if (tm.is0()) po_lm_judge(W, ok2, s[27]);
            tm.sync();
        } while (W.again);
        if (W.stop) break;
    }
}

// The classification after a round (:382-438) over this lane's edges; returns how many of them it flagged.  An inlier edge
// keeps the _error of the last computeActiveErrors, i.e. at W.tried, the last TRIED estimate, accepted or not; an outlier
// edge is recomputed at W.est (:390).  chi2 is rounded to float, the comparison is strict.
template <class Team> PO_HD int po_classify(Team &tm, const PoWs &W, const PoFrame &F, int ne)
{
    double est[7], tried[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { est[k] = W.est[k]; tried[k] = W.tried[k]; }
    int bad = 0;
    for (int j = tm.first(); j < ne; j += tm.stride()) {
        PoEdge e;
        po_load_edge(F, j, e);
        double err[3], P[3];
        const double chi2 = po_edge_error(e, F.e_out[j] ? est : tried, F.cam, err, P);
        const bool out = (float)chi2 > e.thr;
        F.e_out[j] = out ? 1 : 0;
        bad += out ? 1 : 0;
    }
    return bad;
}

// The function and the loop of Tracking that follows it.  F.e_* hold the compacted edges, W.ne their number, e_out is zero,
// W.cnt is zero; all of it behind a sync.
template <class Team> PO_HD void po_run(Team &tm, PoWs &W, const PoFrame &F)
{
    const int ne = W.ne;
    int status = ORBHIP_POSEOPT_OK, rounds = 0;
    if (ne < 3) {                                                              // :364
        status = ORBHIP_POSEOPT_TOO_FEW;
    } else {
        if (tm.is0()) {
            po_pose_from_Tcw(F.Tcw, W.pose0);
            for (int k = 0; k < 6; ++k) W.x[k] = 0.0;
            W.its_total = 0;
        }
        for (int rnd = 0; rnd < 4; ++rnd) {
            if (tm.is0()) {
                for (int k = 0; k < 7; ++k) { W.est[k] = W.pose0[k]; W.tried[k] = W.pose0[k]; }   // :377
                W.cnt[0] = 0;
            }
            tm.sync();
            po_optimize(tm, W, F, rnd < 3);
            const int bad = po_classify(tm, W, F, ne);
            tm.add(&W.cnt[0], bad);
            ++rounds;
            tm.sync();
            if (ne < 10) { status = ORBHIP_POSEOPT_ONE_ROUND; break; }        // :440
        }
        if (tm.is0()) {
            double q[4], R[9];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = W.est[k];
            po_to_R(q, R);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) F.Tcw[r * 4 + c] = (float)R[r * 3 + c];
                F.Tcw[r * 4 + 3] = (float)W.est[4 + r];
            }
        }
    }
    // mvbOutlier and the loop of Tracking, per edge: every slot it touches has a point
    int ca = 0, cb = 0;
    for (int j = tm.first(); j < ne; j += tm.stride()) {
        const int slot = F.e_slot[j], p = F.e_pt[j];
        const bool out = F.e_out[j] != 0;
        const bool observed = F.pflags && (F.pflags[p] & ORBHIP_POINT_OBSERVED);
        uint8_t byte = out ? 1 : 0;
        if (F.mode != ORBHIP_POSEOPT_PLAIN && F.discarded) F.discarded[slot] = -1;
        if (F.mode == ORBHIP_POSEOPT_DISCARD) {
            if (out) {                                                         // src/Tracking.cc:906-915
                F.frame_point[slot] = -1;
                byte = 0;
                if (F.discarded) F.discarded[slot] = p;
            } else {
                ++ca;
                if (observed) ++cb;
            }
        } else if (F.mode == ORBHIP_POSEOPT_LOCAL_MAP) {
            if (!out) {                                                        // :948-958
                ++cb;
                if ((F.flags & ORBHIP_POSEOPT_ONLY_TRACKING) || observed) ++ca;
            } else if (F.flags & ORBHIP_POSEOPT_STEREO) {                      // :959-960: the byte stays set
                F.frame_point[slot] = -1;
                if (F.discarded) F.discarded[slot] = p;
            }
        }
        F.outlier[slot] = byte;
    }
    tm.add(&W.cnt[1], ca);
    tm.add(&W.cnt[2], cb);
    tm.sync();
    if (tm.is0()) {
        const int n_bad = status == ORBHIP_POSEOPT_TOO_FEW ? 0 : W.cnt[0];
        F.report[0] = status; F.report[1] = ne; F.report[2] = n_bad;
        F.report[3] = status == ORBHIP_POSEOPT_TOO_FEW ? 0 : ne - n_bad;
        F.report[4] = rounds; F.report[5] = status == ORBHIP_POSEOPT_TOO_FEW ? 0 : W.its_total;
        F.report[6] = W.cnt[1]; F.report[7] = W.cnt[2];
    }
}

// ---- the host team: one thread that replays the device team's order ----------------------------------------------------
struct PoHostTeam : HostTeam {
    template <bool FULL> void sum(PoWs &W, const PoFrame &F, bool kernel, double *s)
    {
        static thread_local double lanes[kPoTeam][28];
        for (int l = 0; l < kPoTeam; ++l)
            for (int k = 0; k < 28; ++k) lanes[l][k] = 0.0;
        for (int j = 0; j < W.ne; ++j) {
            if (F.e_out[j]) continue;
            PoEdge e;
            po_load_edge(F, j, e);
            po_edge_terms<FULL>(e, W.est, F.cam, kernel, lanes[j % kPoTeam]);
        }
        host_team_combine<kPoTeam, 28>(lanes, FULL ? 0 : 27, s, TeamAdd());
    }
};

// compaction on the host: the slots i < n with a point, in slot order (:280-360)
inline void po_host_compact(PoWs &W, const PoFrame &F)
{
    int ne = 0;
    for (int i = 0; i < F.n; ++i) {
        const int p = F.frame_point[i];
        if (p < 0 || p >= F.pcap) {
            if (F.mode != ORBHIP_POSEOPT_PLAIN && F.discarded) F.discarded[i] = -1;
            continue;
        }
        F.e_slot[ne] = (uint16_t)i; F.e_pt[ne] = p; F.e_out[ne] = 0;           // :289, :323: the byte is written at the end
        ++ne;
    }
    W.ne = ne;
    W.cnt[0] = W.cnt[1] = W.cnt[2] = 0;
}

}  // namespace orbhip
