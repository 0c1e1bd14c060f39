// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) for one current key frame, operation by operation what
// tests/seqref/lba.py does: the two projection edges with both Jacobians, g2o's Levenberg-Marquardt
// over BlockSolver_6_3 (point blocks, Schur complement, a dense unpivoted LDLt over the free poses, back-substitution),
// the level-1 rule, the final check and the write-back.  Everything is fp64, one rounding per operation (the library is
// built with -ffp-contract=off).  orbhip_poseopt_core.h supplies the SE3 algebra, det_sincos64 and the edge error.
//
// The same text serves the phase kernels of orbhip_lba.hip and one host thread (lba_host_run).  The work is cut into items
// -- an edge, a point, a free pose, a pair of free poses, an element of the update vector -- and into the serial state
// machine one lane runs over LbaState.  Sums that cross lanes are written as a lane part (which items lane l adds, in
// which order) and a combine (xor butterfly over the 64 lanes of a wavefront, offsets 1 .. 32, then the wavefronts in
// order); the host replays both literally.  The orders are functions of the compacted lists and of the constants below
// only, never of a launch geometry:
//   - a point's blocks: its edges are contiguous, added in edge order from 0.0 by one lane;
//   - a pose's blocks and a pair's Schur block: entry k of the pose's edge index belongs to lane k mod 64;
//   - chi2, the largest diagonal and computeScale: item t belongs to lane t mod kLbaTeam (256).
// The Levenberg-Marquardt rule and the host replay of the combine are orbhip_lm_core.h's; lba_lm_judge keeps what is the
// function's own around the rule: the two buffers, the trial counters, the stop byte and the phases.
// Nothing here indexes a private array at run time.
#pragma once
#include "orbhip_poseopt_core.h"

namespace orbhip {

constexpr int kLbaMaxLocal = ORBHIP_LBA_MAX_LOCAL;      // free poses of the dense system
constexpr int kLbaTeam = 256;                           // lanes of the team sums: part of the arithmetic, not of the launch
constexpr int kLbaWave = 64;
constexpr int kLbaRec = 56;                             // doubles of an edge record
// an edge record: what linearisation leaves for the block sums
constexpr int kLbaHll = 0, kLbaBl = 6, kLbaHpp = 9, kLbaBp = 30, kLbaB = 36, kLbaRho = 54, kLbaChi2 = 55;
constexpr int kLbaStereo = 1, kLbaLevel1 = 2;           // bits of e_fl

enum { kLbaDone = 0, kLbaBuild, kLbaTrial, kLbaClassify, kLbaFinal };

struct LbaState {
    int phase, round, it, qmax, ok2, status, cur, tried;
    int n_lkf, n_fkf, n_pts, n_edges, n_free, n_mono, n_stereo, n_level1, n_erase, n_active;
    int its[2], trials[2], poses[2];
    int n_bad_lm, samples, pad;
    double lam, ni, current, ini, rho;
};

struct LbaWs {
    // the tables (include/orbhip.h)
    const int *slot_point, *n;
    const uint8_t *kf_bad;
    const int *obs_start, *obs_kf, *obs_idx;
    const uint8_t *flags;
    const orbhip_keypoint *kps;
    const float *u_right;
    const int *ord_kf, *n_ord;
    float *Tcw, *world;
    int *o_local_kf, *o_fixed_kf, *o_local_point, *o_erase, *o_report;
    const uint8_t *stop;                    // nullable: *pbStopFlag
    const uint8_t *script;                  // host tests: the values successive samples return (the last one repeats)
    int script_n;
    float inv[ORBHIP_MAX_LEVELS];
    PoCam cam;
    int cur, id0_row, rows, cap, np, pcap, n_levels, max_points, max_edges;
    // what global bundle adjustment (orbhip_gba_core.h) sets; all zero is LocalBundleAdjustment
    int single_its;                         // > 0: one round of optimize(single_its), no level-1 rule
    int robust;                             // that round's edges carry Huber kernels
    int max_free;                           // free poses the dense system is sized for (0: kLbaMaxLocal)
    // the workspace
    LbaState *S;
    int *lkf, *fkf, *lpt;                   // [rows], [rows], [max_points]: the three lists
    int *kf_vtx;                            // [rows]: vertex of a row (local list position, then fixed list position) or -1
    int *vtx_row, *vtx_free;                // [rows]: row of a vertex; its free pose or -1
    int *pt_key, *kf_key, *pt_c0;           // [pcap], [rows], [max_points + 1]: setup
    uint8_t *kf_stamp;                      // [rows]: 1 = mnBALocalForKF, 2 = mnBAFixedForKF
    int *e_vtx, *e_idx, *e_pt;              // [max_edges]: the edges in creation order
    uint8_t *e_fl, *e_erase;
    int *pt_e0;                             // [max_points + 1]: a point's edges
    int *kf_e0, *kf_edges;                  // [max_free + 1], [max_edges]: a free pose's edges, ascending
    uint8_t *pt_active, *pose_active;       // [max_points], [max_free]
    double *pose, *pt;                      // [2][rows][7], [2][max_points][3]: the accepted estimate is buffer S->cur
    double *eb;                             // [max_edges][kLbaRec]
    double *Hll, *bl, *Dinv, *db, *xl;      // [max_points][6 | 3 | 6 | 3 | 3]
    double *Hpp, *bp;                       // [max_free][21 | 6]
    double *A, *bs, *xp, *L, *y;            // the Schur system [n][n], [n] each, n = 6 * n_free
};

PO_HD double lba_max2(double a, double b) { return a < b ? b : a; }               // std::max(a, b)

PO_HD size_t lba_pose_at(const LbaWs &W, int buf, int v) { return ((size_t)buf * W.rows + v) * 7; }
PO_HD size_t lba_pt_at(const LbaWs &W, int buf, int i) { return ((size_t)buf * W.max_points + i) * 3; }

// ---- the stop byte --------------------------------------------------------------------------------------------------
PO_HD bool lba_sample(LbaWs &W)
{
    if (!W.stop) return false;
    LbaState &S = *W.S;
    uint8_t v;
    if (W.script) v = W.script[S.samples < W.script_n ? S.samples : W.script_n - 1];
    else v = *(const volatile uint8_t *)W.stop;
    S.samples = S.samples + 1;
    return v != 0;
}

// ---- the serial state machine ---------------------------------------------------------------------------------------
PO_HD int lba_max_free(const LbaWs &W) { return W.max_free ? W.max_free : kLbaMaxLocal; }
PO_HD bool lba_robust(const LbaWs &W) { return W.single_its ? W.robust != 0 : W.S->round == 0; }
PO_HD void lba_round_end(LbaWs &W)
{
    LbaState &S = *W.S;
    if (W.single_its) S.phase = kLbaFinal;
    else if (S.round == 0) {
        if (lba_sample(W)) { S.status = ORBHIP_LBA_ONE_ROUND; S.phase = kLbaFinal; }   // :664
        else S.phase = kLbaClassify;
    } else {
        S.phase = kLbaFinal;
    }
}
// the condition of the loop of SparseOptimizer::optimize (sparse_optimizer.cpp:376): i < iterations && !terminate() && ok
PO_HD void lba_iter_top(LbaWs &W, bool ok)
{
    LbaState &S = *W.S;
    if (S.it >= (W.single_its ? W.single_its : (S.round == 0 ? 5 : 10))) { lba_round_end(W); return; }
    const bool t = lba_sample(W);
    if (t || !ok) { lba_round_end(W); return; }
    S.phase = kLbaBuild;
}
// initializeOptimization + optimize: without an active edge there is no vertex to optimise and optimize() returns at once
PO_HD void lba_round_begin(LbaWs &W, int round)
{
    LbaState &S = *W.S;
    S.round = round; S.it = 0;
    if (S.n_active == 0) { lba_round_end(W); return; }
    lba_iter_top(W, true);
}
// after the setup: :655 and the first round
PO_HD void lba_begin(LbaWs &W)
{
    LbaState &S = *W.S;
    if (S.status == ORBHIP_LBA_CAPACITY) { S.phase = kLbaFinal; return; }
    if (lba_sample(W)) { S.status = ORBHIP_LBA_STOPPED; S.poses[0] = 0; S.phase = kLbaFinal; return; }
    lba_round_begin(W, 0);
}
// OptimizationAlgorithmLevenberg::solve :82-101 with the robust chi2 and the largest diagonal at the estimate
PO_HD void lba_lm_begin(LbaWs &W, double chi, double mx)
{
    lm_begin(*W.S, chi, 1e-5 * mx);
    W.S->phase = kLbaTrial;
}
// :123-163 with the trial's robust chi2 and computeScale
PO_HD void lba_lm_judge(LbaWs &W, double temp, double scale)
{
    LbaState &S = *W.S;
    S.tried = 1 - S.cur;
    // discardTop: the tried estimate stands; pop: the other buffer is overwritten by the next trial
    if (lm_gain(S, S.ok2 != 0, temp, scale)) S.cur = 1 - S.cur;
    S.trials[S.round] = S.trials[S.round] + 1;
    if (lm_retry(S) && !lba_sample(W)) return;                                     // another trial
    S.its[S.round] = S.its[S.round] + 1;
    S.it = S.it + 1;
    lba_iter_top(W, lm_iteration_ok(S));
}

// ---- an edge ----------------------------------------------------------------------------------------------------------
PO_HD void lba_load_edge(const LbaWs &W, int j, int buf, PoEdge &e, double *pose, int &fr)
{
    const int v = W.e_vtx[j], pi = W.e_pt[j], idx = W.e_idx[j];
    const size_t k = (size_t)W.vtx_row[v] * W.cap + idx;
    const orbhip_keypoint kp = W.kps[k];
    e.stereo = (W.e_fl[j] & kLbaStereo) != 0;
    const size_t po = lba_pt_at(W, buf, pi), vo = lba_pose_at(W, buf, v);
    e.X[0] = W.pt[po]; e.X[1] = W.pt[po + 1]; e.X[2] = W.pt[po + 2];
#pragma unroll
    for (int q = 0; q < 7; ++q) pose[q] = W.pose[vo + q];
    e.obs[0] = (double)kp.x; e.obs[1] = (double)kp.y; e.obs[2] = e.stereo ? (double)W.u_right[k] : -1.0;
    const int lv = kp.octave < 0 ? 0 : (kp.octave >= W.n_levels ? W.n_levels - 1 : kp.octave);
    e.inv = (double)W.inv[lv];
    e.delta = e.stereo ? W.cam.delta_stereo : W.cam.delta_mono;
    e.dsqr = e.delta * e.delta;
    e.thr = 0.f;
    fr = W.vtx_free[v];
}

// computeActiveErrors at buffer `buf`: chi2 and the robust chi2 of an active edge
PO_HD void lba_edge_error(const LbaWs &W, int j, int buf)
{
    if (W.e_fl[j] & kLbaLevel1) return;
    PoEdge e;
    double pose[7], err[3], P[3];
    int fr;
    lba_load_edge(W, j, buf, e, pose, fr);
    const double chi2 = po_edge_error(e, pose, W.cam, err, P);
    double rho0 = chi2;
    if (lba_robust(W) && !(chi2 <= e.dsqr)) rho0 = 2 * sqrt(chi2) * e.delta - e.dsqr;
    double *r = W.eb + (size_t)j * kLbaRec;
    r[kLbaRho] = rho0; r[kLbaChi2] = chi2;
}

// computeActiveErrors, linearizeOplus (types_six_dof_expmap.cpp:103-139, :188-234) and constructQuadraticForm
// (base_binary_edge.hpp:55-120) of an active edge at the accepted estimate
PO_HD void lba_edge_linearize(const LbaWs &W, int j)
{
    if (W.e_fl[j] & kLbaLevel1) return;
    PoEdge e;
    double pose[7], err[3], P[3], R[9];
    int fr;
    lba_load_edge(W, j, W.S->cur, e, pose, fr);
    const double chi2 = po_edge_error(e, pose, W.cam, err, P);
    double rho0 = chi2, rho1 = 1.0;
    if (lba_robust(W) && !(chi2 <= e.dsqr)) {                                     // RobustKernelHuber::robustify
        const double s = sqrt(chi2);
        rho0 = 2 * s * e.delta - e.dsqr;
        rho1 = e.delta / s;
    }
    double *r = W.eb + (size_t)j * kLbaRec;
    r[kLbaRho] = rho0; r[kLbaChi2] = chi2;
    po_to_R(pose, R);
    const double x = P[0], y = P[1], z = P[2], z_2 = z * z, fx = W.cam.fx, fy = W.cam.fy, bf = W.cam.bf;
    double Jc0[6], Jc1[6], Jc2[6], Jp0[3], Jp1[3], Jp2[3];
    Jc0[0] = x * y / z_2 * fx; Jc0[1] = -(1 + (x * x / z_2)) * fx; Jc0[2] = y / z * fx;
    Jc0[3] = -1. / z * fx; Jc0[4] = 0.0; Jc0[5] = x / z_2 * fx;
    Jc1[0] = (1 + y * y / z_2) * fy; Jc1[1] = -x * y / z_2 * fy; Jc1[2] = -x / z * fy;
    Jc1[3] = 0.0; Jc1[4] = -1. / z * fy; Jc1[5] = y / z_2 * fy;
    Jc2[0] = Jc0[0] - bf * y / z_2; Jc2[1] = Jc0[1] + bf * x / z_2; Jc2[2] = Jc0[2];
    Jc2[3] = Jc0[3]; Jc2[4] = 0.0; Jc2[5] = Jc0[5] - bf / z_2;
    if (e.stereo) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Jp0[c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
            Jp1[c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
            Jp2[c] = Jp0[c] - bf * R[6 + c] / z_2;
        }
    } else {
        const double m = -1. / z;                                                  // -1./z * tmp * R, left to right
        const double m00 = m * fx, m01 = m * 0.0, m02 = m * (-x / z * fx), m10 = m * 0.0, m11 = m * fy, m12 = m * (-y / z * fy);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Jp0[c] = (m00 * R[c] + m01 * R[3 + c]) + m02 * R[6 + c];
            Jp1[c] = (m10 * R[c] + m11 * R[3 + c]) + m12 * R[6 + c];
            Jp2[c] = 0.0;
        }
    }
    const double w = rho1 * e.inv;                                                 // weightedOmega = rho[1] * omega
    const double o0 = -(e.inv * err[0]) * rho1, o1 = -(e.inv * err[1]) * rho1, o2 = -(e.inv * err[2]) * rho1;   // omega_r
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double s = 0.0;
            s = s + (Jp0[a] * w) * Jp0[b];
            s = s + (Jp1[a] * w) * Jp1[b];
            if (e.stereo) s = s + (Jp2[a] * w) * Jp2[b];
            r[kLbaHll + k] = s;
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
        s = s + Jp0[a] * o0;
        s = s + Jp1[a] * o1;
        if (e.stereo) s = s + Jp2[a] * o2;
        r[kLbaBl + a] = s;
    }
    if (fr < 0) return;                                                            // a fixed pose takes no block
    k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double s = 0.0;
            s = s + (Jc0[a] * w) * Jc0[b];
            s = s + (Jc1[a] * w) * Jc1[b];
            if (e.stereo) s = s + (Jc2[a] * w) * Jc2[b];
            r[kLbaHpp + k] = s;
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        s = s + Jc0[a] * o0;
        s = s + Jc1[a] * o1;
        if (e.stereo) s = s + Jc2[a] * o2;
        r[kLbaBp + a] = s;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)                                                    // B[a][b]: pose row a, point column b
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            s = s + (Jp0[b] * w) * Jc0[a];
            s = s + (Jp1[b] * w) * Jc1[a];
            if (e.stereo) s = s + (Jp2[b] * w) * Jc2[a];
            r[kLbaB + a * 3 + b] = s;
        }
}

// isDepthPositive at buffer `buf`
PO_HD bool lba_depth_positive(const LbaWs &W, int j, int buf)
{
    const int v = W.e_vtx[j];
    const size_t po = lba_pt_at(W, buf, W.e_pt[j]), vo = lba_pose_at(W, buf, v);
    double q[4], X[3], r[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = W.pose[vo + k];
    X[0] = W.pt[po]; X[1] = W.pt[po + 1]; X[2] = W.pt[po + 2];
    po_quat_rot(q, X, r);
    return r[2] + W.pose[vo + 6] > 0.0;
}
// :680 / :696 and :723 / :738: chi2() is the _error of the last computeActiveErrors that had the edge active, compared in
// double, strictly; the depth is taken at the accepted estimate
PO_HD bool lba_edge_bad(const LbaWs &W, int j)
{
    const double chi2 = W.eb[(size_t)j * kLbaRec + kLbaChi2];
    const double thr = (W.e_fl[j] & kLbaStereo) ? 7.815 : 5.991;
    return chi2 > thr || !lba_depth_positive(W, j, W.S->cur);
}

// ---- a point ----------------------------------------------------------------------------------------------------------
PO_HD void lba_point_block(const LbaWs &W, int i)
{
    if (!W.pt_active[i]) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int j = W.pt_e0[i]; j < W.pt_e0[i + 1]; ++j) {
        if (W.e_fl[j] & kLbaLevel1) continue;
        const double *r = W.eb + (size_t)j * kLbaRec;
        s0 = s0 + r[0]; s1 = s1 + r[1]; s2 = s2 + r[2]; s3 = s3 + r[3]; s4 = s4 + r[4]; s5 = s5 + r[5];
        b0 = b0 + r[6]; b1 = b1 + r[7]; b2 = b2 + r[8];
    }
    double *H = W.Hll + (size_t)i * 6, *b = W.bl + (size_t)i * 3;
    H[0] = s0; H[1] = s1; H[2] = s2; H[3] = s3; H[4] = s4; H[5] = s5;
    b[0] = b0; b[1] = b1; b[2] = b2;
}
// Dinv = (Hll + lambda I)^-1 as cofactors over the determinant, db = Dinv b_l (block_solver.hpp:386-395)
PO_HD void lba_point_dinv(const LbaWs &W, int i)
{
    if (!W.pt_active[i]) return;
    const double *H = W.Hll + (size_t)i * 6, *b = W.bl + (size_t)i * 3, lam = W.S->lam;
    const double d00 = H[0] + lam, d01 = H[1], d02 = H[2], d11 = H[3] + lam, d12 = H[4], d22 = H[5] + lam;
    const double c00 = d11 * d22 - d12 * d12, c01 = d02 * d12 - d01 * d22, c02 = d01 * d12 - d02 * d11;
    const double c11 = d00 * d22 - d02 * d02, c12 = d01 * d02 - d00 * d12, c22 = d00 * d11 - d01 * d01;
    const double det = (d00 * c00 + d01 * c01) + d02 * c02;
    double *D = W.Dinv + (size_t)i * 6, *db = W.db + (size_t)i * 3;
    const double i00 = c00 / det, i01 = c01 / det, i02 = c02 / det, i11 = c11 / det, i12 = c12 / det, i22 = c22 / det;
    D[0] = i00; D[1] = i01; D[2] = i02; D[3] = i11; D[4] = i12; D[5] = i22;
    db[0] = (i00 * b[0] + i01 * b[1]) + i02 * b[2];
    db[1] = (i01 * b[0] + i11 * b[1]) + i12 * b[2];
    db[2] = (i02 * b[0] + i12 * b[1]) + i22 * b[2];
}
// :468-481 and the update of the point: x_l = Dinv (b_l - B^T x_p) when the poses were solved, the stale x_l otherwise;
// tried = estimate + x_l.  A point outside the system keeps its bits.
PO_HD void lba_point_update(const LbaWs &W, int i)
{
    const int cur = W.S->cur;
    const size_t src = lba_pt_at(W, cur, i), dst = lba_pt_at(W, 1 - cur, i);
    if (!W.pt_active[i]) {
        W.pt[dst] = W.pt[src]; W.pt[dst + 1] = W.pt[src + 1]; W.pt[dst + 2] = W.pt[src + 2];
        return;
    }
    double *xl = W.xl + (size_t)i * 3;
    if (W.S->ok2) {
        const double *b = W.bl + (size_t)i * 3, *D = W.Dinv + (size_t)i * 6;
        double c0 = b[0], c1 = b[1], c2 = b[2];
        for (int j = W.pt_e0[i]; j < W.pt_e0[i + 1]; ++j) {
            if (W.e_fl[j] & kLbaLevel1) continue;
            const int fr = W.vtx_free[W.e_vtx[j]];
            if (fr < 0) continue;
            const double *B = W.eb + (size_t)j * kLbaRec + kLbaB, *xp = W.xp + fr * 6;
            const double n0 = -xp[0], n1 = -xp[1], n2 = -xp[2], n3 = -xp[3], n4 = -xp[4], n5 = -xp[5];
            c0 = c0 + (((((B[0] * n0 + B[3] * n1) + B[6] * n2) + B[9] * n3) + B[12] * n4) + B[15] * n5);
            c1 = c1 + (((((B[1] * n0 + B[4] * n1) + B[7] * n2) + B[10] * n3) + B[13] * n4) + B[16] * n5);
            c2 = c2 + (((((B[2] * n0 + B[5] * n1) + B[8] * n2) + B[11] * n3) + B[14] * n4) + B[17] * n5);
        }
        xl[0] = (D[0] * c0 + D[1] * c1) + D[2] * c2;
        xl[1] = (D[1] * c0 + D[3] * c1) + D[4] * c2;
        xl[2] = (D[2] * c0 + D[4] * c1) + D[5] * c2;
    }
    W.pt[dst] = W.pt[src] + xl[0]; W.pt[dst + 1] = W.pt[src + 1] + xl[1]; W.pt[dst + 2] = W.pt[src + 2] + xl[2];
}
// the update of a vertex: exp(x) * estimate for a pose of the system, the same bits for every other
PO_HD void lba_vertex_update(const LbaWs &W, int v)
{
    const int cur = W.S->cur, fr = W.vtx_free[v];
    const size_t src = lba_pose_at(W, cur, v), dst = lba_pose_at(W, 1 - cur, v);
    double e[7], u[6], d[7], o[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) e[k] = W.pose[src + k];
    if (fr >= 0 && W.pose_active[fr]) {
#pragma unroll
        for (int k = 0; k < 6; ++k) u[k] = W.xp[fr * 6 + k];
        po_se3_exp(u, d);
        po_se3_mul(d, e, o);
#pragma unroll
        for (int k = 0; k < 7; ++k) W.pose[dst + k] = o[k];
    } else {
#pragma unroll
        for (int k = 0; k < 7; ++k) W.pose[dst + k] = e[k];
    }
}

// ---- a free pose: its blocks, lane part ---------------------------------------------------------------------------------
PO_HD void lba_pose_block_lane(const LbaWs &W, int f, int lane, double *acc)       // acc[27], zeroed
{
    const int e0 = W.kf_e0[f], e1 = W.kf_e0[f + 1];
    for (int k = e0 + lane; k < e1; k += kLbaWave) {
        const int j = W.kf_edges[k];
        if (W.e_fl[j] & kLbaLevel1) continue;
        const double *r = W.eb + (size_t)j * kLbaRec + kLbaHpp;
#pragma unroll
        for (int q = 0; q < 27; ++q) acc[q] = acc[q] + r[q];
    }
}
PO_HD void lba_pose_block_store(const LbaWs &W, int f, const double *sum)
{
    for (int q = 0; q < 21; ++q) W.Hpp[f * 21 + q] = sum[q];
    for (int q = 0; q < 6; ++q) W.bp[f * 6 + q] = sum[21 + q];
}

// ---- a pair of free poses (i1 <= i2): sum over the points both see of B1 Dinv B2^T, and on the diagonal of B1 (Dinv b_l)
PO_HD int lba_upper(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }    // index of (a, b), a <= b, in the packed 21
PO_HD void lba_schur_lane(const LbaWs &W, int i1, int i2, int lane, double *acc)  // acc[42], zeroed
{
    const int e0 = W.kf_e0[i1], e1 = W.kf_e0[i1 + 1];
    for (int k = e0 + lane; k < e1; k += kLbaWave) {
        const int j1 = W.kf_edges[k];
        if (W.e_fl[j1] & kLbaLevel1) continue;
        const int pi = W.e_pt[j1];
        int j2 = -1;
        if (i1 == i2) j2 = j1;
        else
            for (int j = W.pt_e0[pi]; j < W.pt_e0[pi + 1]; ++j)
                if (!(W.e_fl[j] & kLbaLevel1) && W.vtx_free[W.e_vtx[j]] == i2) { j2 = j; break; }
        if (j2 < 0) continue;
        const double *B1 = W.eb + (size_t)j1 * kLbaRec + kLbaB, *B2 = W.eb + (size_t)j2 * kLbaRec + kLbaB;
        const double *D = W.Dinv + (size_t)pi * 6, *db = W.db + (size_t)pi * 3;
        const double d00 = D[0], d01 = D[1], d02 = D[2], d11 = D[3], d12 = D[4], d22 = D[5];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double p0 = B1[a * 3], p1 = B1[a * 3 + 1], p2 = B1[a * 3 + 2];
            const double g0 = (p0 * d00 + p1 * d01) + p2 * d02, g1 = (p0 * d01 + p1 * d11) + p2 * d12,
                         g2 = (p0 * d02 + p1 * d12) + p2 * d22;                    // a row of B1 Dinv
#pragma unroll
            for (int b = 0; b < 6; ++b) acc[a * 6 + b] = acc[a * 6 + b] + ((g0 * B2[b * 3] + g1 * B2[b * 3 + 1]) + g2 * B2[b * 3 + 2]);
            if (i1 == i2) acc[36 + a] = acc[36 + a] + ((p0 * db[0] + p1 * db[1]) + p2 * db[2]);
        }
    }
}
// the lower triangle of the system: the block (i1, i2) mirrored; a pose outside the system is an identity block
PO_HD void lba_schur_store(const LbaWs &W, int i1, int i2, const double *sum)
{
    const int ld = 6 * W.S->n_free;
    const double lam = W.S->lam;
    if (i1 == i2) {
        const bool act = W.pose_active[i1] != 0;
        for (int a = 0; a < 6; ++a) {
            for (int b = 0; b <= a; ++b) {
                double v = a == b ? 1.0 : 0.0;
                if (act) {
                    double h = W.Hpp[i1 * 21 + lba_upper(b, a)];
                    if (a == b) h = h + lam;
                    v = h - sum[b * 6 + a];
                }
                W.A[(size_t)(6 * i1 + a) * ld + 6 * i1 + b] = v;
            }
            W.bs[6 * i1 + a] = act ? W.bp[i1 * 6 + a] - sum[36 + a] : 0.0;
        }
    } else {
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) W.A[(size_t)(6 * i2 + b) * ld + 6 * i1 + a] = 0.0 - sum[a * 6 + b];
    }
}

// ---- the dense system: unpivoted LDLt in index order, ok iff every pivot is > 0; A, L, y are shared by the team --------
template <class Team> PO_HD bool lba_solve(Team &tm, const LbaWs &W)
{
    const int n = 6 * W.S->n_free, ld = n;
    double *A = W.A, *L = W.L, *y = W.y;
    for (int k = 0; k < n; ++k) {
        const double d = A[(size_t)k * ld + k];
        if (!(d > 0)) return false;
        for (int i = k + 1 + tm.tid(); i < n; i += tm.size()) L[i] = A[(size_t)i * ld + k] / d;
        tm.sync();
        for (int i = k + 1 + tm.wave(); i < n; i += tm.waves()) {
            const double l = L[i];
            for (int j = k + 1 + tm.lane(); j <= i; j += tm.lanes()) A[(size_t)i * ld + j] = A[(size_t)i * ld + j] - l * A[(size_t)j * ld + k];
        }
        tm.sync();
        for (int i = k + 1 + tm.tid(); i < n; i += tm.size()) A[(size_t)i * ld + k] = L[i];
        tm.sync();
    }
    for (int i = tm.tid(); i < n; i += tm.size()) y[i] = W.bs[i];
    tm.sync();
    for (int j = 0; j < n; ++j) {                                                  // L y = b, column by column
        const double yj = y[j];
        for (int i = j + 1 + tm.tid(); i < n; i += tm.size()) y[i] = y[i] - A[(size_t)i * ld + j] * yj;
        tm.sync();
    }
    for (int i = tm.tid(); i < n; i += tm.size()) y[i] = y[i] / A[(size_t)i * ld + i];
    tm.sync();
    for (int j = n - 1; j > 0; --j) {                                              // L^T x = y, from the last column
        const double yj = y[j];
        for (int i = tm.tid(); i < j; i += tm.size()) y[i] = y[i] - A[(size_t)j * ld + i] * yj;
        tm.sync();
    }
    for (int i = tm.tid(); i < n; i += tm.size()) W.xp[i] = y[i];
    tm.sync();
    return true;
}

// ---- the team sums: item t of kind K, lane part ---------------------------------------------------------------------------
constexpr int kLbaSumChi = 0, kLbaSumMax = 1, kLbaSumScale = 2;
PO_HD int lba_sum_items(const LbaWs &W, int kind)
{
    return kind == kLbaSumChi ? W.S->n_edges : 6 * W.S->n_free + 3 * W.S->n_pts;
}
PO_HD int lba_diag21(int a) { return a * 6 - a * (a - 1) / 2; }
PO_HD double lba_sum_lane(const LbaWs &W, int kind, int lane)
{
    const int items = lba_sum_items(W, kind), np6 = 6 * W.S->n_free;
    const double lam = W.S->lam;
    double acc = 0.0;
    for (int t = lane; t < items; t += kLbaTeam) {
        if (kind == kLbaSumChi) {
            if (W.e_fl[t] & kLbaLevel1) continue;
            acc = acc + W.eb[(size_t)t * kLbaRec + kLbaRho];
            continue;
        }
        double h, x, b;
        if (t < np6) {
            const int f = t / 6, a = t - f * 6;
            if (!W.pose_active[f]) continue;
            h = W.Hpp[f * 21 + lba_diag21(a)]; x = W.xp[t]; b = W.bp[t];
        } else {
            const int i = (t - np6) / 3, a = (t - np6) - i * 3;
            if (!W.pt_active[i]) continue;
            h = W.Hll[(size_t)i * 6 + (a == 0 ? 0 : (a == 1 ? 3 : 5))]; x = W.xl[(size_t)i * 3 + a]; b = W.bl[(size_t)i * 3 + a];
        }
        if (kind == kLbaSumMax) acc = lba_max2(fabs(h), acc);
        else acc = acc + x * (lam * x + b);
    }
    return acc;
}
struct LbaSumOp {
    int kind;
    PO_HD double operator()(double a, double b) const { return kind == kLbaSumMax ? lba_max2(a, b) : a + b; }
};

// ---- the epilogue ---------------------------------------------------------------------------------------------------------
// Converter::toCvMat(SE3Quat) of a local key frame, the float of a local point (:762-776)
PO_HD void lba_write_pose(const LbaWs &W, int li)
{
    const size_t vo = lba_pose_at(W, W.S->cur, li);
    double q[4], R[9];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = W.pose[vo + k];
    po_to_R(q, R);
    float *T = W.Tcw + (size_t)W.lkf[li] * 12;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)R[r * 3 + c];
        T[r * 4 + 3] = (float)W.pose[vo + 4 + r];
    }
}
PO_HD void lba_write_point(const LbaWs &W, int i)
{
    const size_t po = lba_pt_at(W, W.S->cur, i);
    float *X = W.world + (size_t)W.lpt[i] * 3;
    X[0] = (float)W.pt[po]; X[1] = (float)W.pt[po + 1]; X[2] = (float)W.pt[po + 2];
}
PO_HD void lba_write_report(const LbaWs &W)
{
    const LbaState &S = *W.S;
    int *r = W.o_report;
    r[0] = S.status; r[1] = S.n_lkf; r[2] = S.n_fkf; r[3] = S.n_pts; r[4] = S.n_mono; r[5] = S.n_stereo; r[6] = S.n_level1;
    r[7] = S.n_erase; r[8] = S.its[0]; r[9] = S.trials[0]; r[10] = S.its[1]; r[11] = S.trials[1]; r[12] = S.poses[0];
    r[13] = S.poses[1]; r[14] = 0; r[15] = S.samples;
}
PO_HD bool lba_writes(const LbaState &S) { return S.status == ORBHIP_LBA_OK || S.status == ORBHIP_LBA_ONE_ROUND; }

// ---- the workspace: carved from one allocation, 256-byte pieces; base == nullptr only sizes it ----------------------------
inline size_t lba_carve(LbaWs &W, uint8_t *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t R = (size_t)W.rows, P = (size_t)W.max_points, E = (size_t)W.max_edges, F = (size_t)lba_max_free(W), n = 6 * F;
    W.S = (LbaState *)take(sizeof(LbaState));
    W.lkf = (int *)take(R * 4); W.fkf = (int *)take(R * 4); W.lpt = (int *)take(P * 4);
    W.kf_vtx = (int *)take(R * 4); W.vtx_row = (int *)take(R * 4); W.vtx_free = (int *)take(R * 4);
    W.pt_key = (int *)take((size_t)W.pcap * 4); W.kf_key = (int *)take(R * 4); W.pt_c0 = (int *)take((P + 1) * 4);
    W.kf_stamp = take(R);
    W.e_vtx = (int *)take(E * 4); W.e_idx = (int *)take(E * 4); W.e_pt = (int *)take(E * 4);
    W.e_fl = take(E); W.e_erase = take(E);
    W.pt_e0 = (int *)take((P + 1) * 4);
    W.kf_e0 = (int *)take((F + 1) * 4); W.kf_edges = (int *)take(E * 4);
    W.pt_active = take(P); W.pose_active = take(F);
    W.pose = (double *)take(2 * R * 7 * 8); W.pt = (double *)take(2 * P * 3 * 8);
    W.eb = (double *)take(E * kLbaRec * 8);
    W.Hll = (double *)take(P * 6 * 8); W.bl = (double *)take(P * 3 * 8); W.Dinv = (double *)take(P * 6 * 8);
    W.db = (double *)take(P * 3 * 8); W.xl = (double *)take(P * 3 * 8);
    W.Hpp = (double *)take(F * 21 * 8); W.bp = (double *)take(F * 6 * 8);
    W.A = (double *)take(n * n * 8); W.bs = (double *)take(n * 8); W.xp = (double *)take(n * 8);
    W.L = (double *)take(n * 8); W.y = (double *)take(n * 8);
    return off;
}

// ---- one host thread ------------------------------------------------------------------------------------------------------
struct LbaHostTeam {
    int tid() const { return 0; }
    int size() const { return 1; }
    int wave() const { return 0; }
    int waves() const { return 1; }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() {}
};
inline double lba_host_team_sum(const LbaWs &W, int kind)
{
    double lanes[kLbaTeam][1], total;
    for (int l = 0; l < kLbaTeam; ++l) lanes[l][0] = lba_sum_lane(W, kind, l);
    host_team_combine<kLbaTeam, 1>(lanes, 0, &total, LbaSumOp{kind});
    return total;
}

// the lists, the edges and the first estimates (:456-653), sequentially; sets S.status to CAPACITY where the call refuses
inline void lba_host_setup(LbaWs &W)
{
    LbaState &S = *W.S;
    memset(&S, 0, sizeof(S));
    for (int r = 0; r < W.rows; ++r) { W.kf_stamp[r] = 0; W.kf_vtx[r] = -1; W.vtx_free[r] = -1; }
    for (int p = 0; p < W.pcap; ++p) W.pt_key[p] = 0;
    auto bad = [&](int r) { return W.kf_bad && W.kf_bad[r]; };
    int nl = 0;
    W.lkf[nl++] = W.cur; W.kf_stamp[W.cur] = 1;
    for (int i = 0; i < W.n_ord[W.cur]; ++i) {
        const int r = W.ord_kf[(size_t)W.cur * W.rows + i];
        if (r < 0 || r >= W.rows || W.kf_stamp[r]) continue;
        W.kf_stamp[r] = 1;
        if (!bad(r)) W.lkf[nl++] = r;
    }
    int nfree = 0;
    for (int li = 0; li < nl; ++li) {
        const int r = W.lkf[li];
        W.kf_vtx[r] = li; W.vtx_row[li] = r;
        W.vtx_free[li] = r == W.id0_row ? -1 : nfree++;
    }
    S.n_lkf = nl; S.n_free = nfree;
    int npts = 0;
    for (int li = 0; li < nl; ++li) {
        const int r = W.lkf[li];
        for (int s = 0; s < W.n[r]; ++s) {
            const int p = W.slot_point[(size_t)r * W.cap + s];
            if (p < 0 || p >= W.np || !(W.flags[p] & ORBHIP_POINT_PRESENT) || W.pt_key[p]) continue;
            W.pt_key[p] = 1;
            if (npts < W.max_points) W.lpt[npts] = p;
            ++npts;
        }
    }
    S.n_pts = npts;
    if (nfree > kLbaMaxLocal || npts > W.max_points) { S.status = ORBHIP_LBA_CAPACITY; return; }
    int nf = 0;
    for (int i = 0; i < npts; ++i) {
        const int p = W.lpt[i];
        for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
            const int r = W.obs_kf[o];
            if (r < 0 || r >= W.rows || W.kf_stamp[r]) continue;
            W.kf_stamp[r] = 2;
            if (!bad(r)) {
                W.fkf[nf] = r; W.kf_vtx[r] = nl + nf; W.vtx_row[nl + nf] = r; W.vtx_free[nl + nf] = -1;
                ++nf;
            }
        }
    }
    S.n_fkf = nf;
    int ne = 0, nm = 0, ns = 0;
    for (int i = 0; i < npts; ++i) {
        const int p = W.lpt[i];
        W.pt_e0[i] = ne < W.max_edges ? ne : W.max_edges;
        for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
            const int r = W.obs_kf[o];
            if (r < 0 || r >= W.rows || bad(r) || W.kf_vtx[r] < 0) continue;
            const int idx = W.obs_idx[o];
            const bool stereo = W.u_right && !(W.u_right[(size_t)r * W.cap + idx] < 0);
            if (ne < W.max_edges) {
                W.e_vtx[ne] = W.kf_vtx[r]; W.e_idx[ne] = idx; W.e_pt[ne] = i; W.e_fl[ne] = stereo ? kLbaStereo : 0;
                W.eb[(size_t)ne * kLbaRec + kLbaChi2] = 0.0;
            }
            ++ne;
            if (stereo) ++ns; else ++nm;
        }
    }
    S.n_edges = ne; S.n_mono = nm; S.n_stereo = ns;
    if (ne > W.max_edges) { S.status = ORBHIP_LBA_CAPACITY; return; }
    W.pt_e0[npts] = ne;
    for (int f = 0; f <= nfree; ++f) W.kf_e0[f] = 0;
    for (int j = 0; j < ne; ++j) { const int f = W.vtx_free[W.e_vtx[j]]; if (f >= 0) W.kf_e0[f + 1]++; }
    for (int f = 0; f < nfree; ++f) W.kf_e0[f + 1] += W.kf_e0[f];
    {
        int fill[kLbaMaxLocal];
        for (int f = 0; f < nfree; ++f) fill[f] = W.kf_e0[f];
        for (int j = 0; j < ne; ++j) { const int f = W.vtx_free[W.e_vtx[j]]; if (f >= 0) W.kf_edges[fill[f]++] = j; }
    }
    for (int v = 0; v < nl + nf; ++v) {
        double p[7];
        po_pose_from_Tcw(W.Tcw + (size_t)W.vtx_row[v] * 12, p);
        for (int k = 0; k < 7; ++k) { W.pose[lba_pose_at(W, 0, v) + k] = p[k]; W.pose[lba_pose_at(W, 1, v) + k] = p[k]; }
    }
    for (int i = 0; i < npts; ++i)
        for (int k = 0; k < 3; ++k) {
            const double x = (double)W.world[(size_t)W.lpt[i] * 3 + k];
            W.pt[lba_pt_at(W, 0, i) + k] = x; W.pt[lba_pt_at(W, 1, i) + k] = x;
            W.xl[(size_t)i * 3 + k] = 0.0;
        }
    for (int k = 0; k < 6 * nfree; ++k) W.xp[k] = 0.0;
}
// which vertices the system of a round holds: those with an edge at level 0
inline void lba_host_activity(LbaWs &W, int round)
{
    LbaState &S = *W.S;
    int poses = 0;
    for (int i = 0; i < S.n_pts; ++i) {
        W.pt_active[i] = 0;
        for (int j = W.pt_e0[i]; j < W.pt_e0[i + 1]; ++j) if (!(W.e_fl[j] & kLbaLevel1)) W.pt_active[i] = 1;
    }
    for (int f = 0; f < S.n_free; ++f) {
        W.pose_active[f] = 0;
        for (int k = W.kf_e0[f]; k < W.kf_e0[f + 1]; ++k) if (!(W.e_fl[W.kf_edges[k]] & kLbaLevel1)) W.pose_active[f] = 1;
        poses += W.pose_active[f];
    }
    S.poses[round] = poses;
    S.n_active = S.n_edges - S.n_level1;
}

struct LbaHostTrace {                       // what tests/cpp/lba_host.cpp prints: the estimates when a round ends
    double *est[2], *tried[2];              // [rows][7] + [max_points][3] each, or null
};

inline void lba_host_snapshot(const LbaWs &W, int buf, double *dst)
{
    if (!dst) return;
    const int nv = W.S->n_lkf + W.S->n_fkf;
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < 7; ++k) dst[v * 7 + k] = W.pose[lba_pose_at(W, buf, v) + k];
    for (int i = 0; i < W.S->n_pts; ++i)
        for (int k = 0; k < 3; ++k) dst[(size_t)W.rows * 7 + i * 3 + k] = W.pt[lba_pt_at(W, buf, i) + k];
}

// one linearisation (phase kLbaBuild) and one trial (phase kLbaTrial) on one thread, step by step as the device enqueues them
inline void lba_host_build(LbaWs &W)
{
    LbaState &S = *W.S;
    for (int j = 0; j < S.n_edges; ++j) lba_edge_linearize(W, j);
    for (int i = 0; i < S.n_pts; ++i) lba_point_block(W, i);
    for (int f = 0; f < S.n_free; ++f) {
        double lanes[kLbaWave][27], sum[27];
        for (int l = 0; l < kLbaWave; ++l) { for (int k = 0; k < 27; ++k) lanes[l][k] = 0.0; lba_pose_block_lane(W, f, l, lanes[l]); }
        host_team_combine<kLbaWave, 27>(lanes, 0, sum, TeamAdd());
        lba_pose_block_store(W, f, sum);
    }
    const double chi = lba_host_team_sum(W, kLbaSumChi), mx = S.it == 0 ? lba_host_team_sum(W, kLbaSumMax) : 0.0;
    lba_lm_begin(W, chi, mx);
}
inline void lba_host_trial(LbaWs &W)
{
    LbaState &S = *W.S;
    LbaHostTeam tm;
    for (int i = 0; i < S.n_pts; ++i) lba_point_dinv(W, i);
    for (int i1 = 0; i1 < S.n_free; ++i1)
        for (int i2 = i1; i2 < S.n_free; ++i2) {
            double lanes[kLbaWave][42], sum[42];
            for (int l = 0; l < kLbaWave; ++l) { for (int k = 0; k < 42; ++k) lanes[l][k] = 0.0; lba_schur_lane(W, i1, i2, l, lanes[l]); }
            host_team_combine<kLbaWave, 42>(lanes, 0, sum, TeamAdd());
            lba_schur_store(W, i1, i2, sum);
        }
    S.ok2 = lba_solve(tm, W) ? 1 : 0;
    for (int i = 0; i < S.n_pts; ++i) lba_point_update(W, i);
    for (int v = 0; v < S.n_lkf + S.n_fkf; ++v) lba_vertex_update(W, v);
    for (int j = 0; j < S.n_edges; ++j) lba_edge_error(W, j, 1 - S.cur);
    const double chi = lba_host_team_sum(W, kLbaSumChi), scale = lba_host_team_sum(W, kLbaSumScale);
    lba_lm_judge(W, chi, scale);
}

// the whole function on one thread, phase by phase as the device enqueues it
inline void lba_host_run(LbaWs &W, LbaHostTrace *trace = nullptr)
{
    LbaState &S = *W.S;
    lba_host_setup(W);
    if (S.status != ORBHIP_LBA_CAPACITY) lba_host_activity(W, 0);
    lba_begin(W);
    int snapped = 0;
    auto snap = [&](int round) {
        if (trace && snapped == round) { lba_host_snapshot(W, S.cur, trace->est[round]); lba_host_snapshot(W, S.tried, trace->tried[round]); ++snapped; }
    };
    while (S.phase != kLbaDone) {
        if (S.phase == kLbaBuild) {
            lba_host_build(W);
        } else if (S.phase == kLbaTrial) {
            const int round = S.round;
            lba_host_trial(W);
            if (S.phase == kLbaClassify || S.phase == kLbaFinal) snap(round);
        } else if (S.phase == kLbaClassify) {
            snap(0);
            for (int j = 0; j < S.n_edges; ++j)
                if (lba_edge_bad(W, j)) { W.e_fl[j] |= kLbaLevel1; S.n_level1++; }
            for (int k = 0; k < 6 * S.n_free; ++k) W.xp[k] = 0.0;
            for (int k = 0; k < 3 * S.n_pts; ++k) W.xl[k] = 0.0;
            lba_host_activity(W, 1);
            lba_round_begin(W, 1);
        } else {                                                                   // kLbaFinal
            if (lba_writes(S)) {
                snap(0); snap(1);
                int ne = 0;
                for (int pass = 0; pass < 2; ++pass)
                    for (int j = 0; j < S.n_edges; ++j) {
                        if (((W.e_fl[j] & kLbaStereo) != 0) != (pass == 1) || !lba_edge_bad(W, j)) continue;
                        W.o_erase[ne * 3] = W.vtx_row[W.e_vtx[j]]; W.o_erase[ne * 3 + 1] = W.e_idx[j]; W.o_erase[ne * 3 + 2] = W.lpt[W.e_pt[j]];
                        ++ne;
                    }
                S.n_erase = ne;
                for (int li = 0; li < S.n_lkf; ++li) { W.o_local_kf[li] = W.lkf[li]; lba_write_pose(W, li); }
                for (int k = 0; k < S.n_fkf; ++k) W.o_fixed_kf[k] = W.fkf[k];
                for (int i = 0; i < S.n_pts; ++i) { W.o_local_point[i] = W.lpt[i]; lba_write_point(W, i); }
            }
            lba_write_report(W);
            S.phase = kLbaDone;
        }
    }
}

}  // namespace orbhip
