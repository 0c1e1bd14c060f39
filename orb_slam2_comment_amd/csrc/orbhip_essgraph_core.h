// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:781-1044), operation by operation what tests/seqref/essgraph.py does
// (DESIGN.md section 3): one Sim3 vertex per key frame that is not bad, EdgeSim3 with the identity as information, g2o's
// numeric Jacobian through oplusImpl, Levenberg-Marquardt from lambda 1e-16 over a dense system of 7 unknowns per free
// vertex, the SE3 write-back and the correction of the points.  Everything is fp64, one rounding per operation (the library
// is built with -ffp-contract=off).  orbhip_sim3opt_core.h supplies g2o::Sim3 (s3o_exp, s3o_mul, s3o_inverse), det_exp64
// and, through orbhip_poseopt_core.h, det_sincos64 and the quaternion helpers; det_log64, det_acos64 and Sim3::log are here.
//
// The same text serves the kernels of orbhip_essgraph.hip and one host thread (eg_host_run).  The work is cut into items -- a
// vertex, a bank row's edges, one of the 29 error evaluations of an edge, an element of an edge's blocks, an element of a
// vertex's blocks, an element of the update -- and into the serial state machine one lane runs over EgState.  The orders of
// all sums are functions of the edge list and of kEgTeam only, never of a launch geometry or of the panel width:
//   - an edge's blocks: sums over the 7 error rows, ascending from 0.0;
//   - a vertex's diagonal block and b: its edges in creation order from 0.0; an off-diagonal block belongs to the vertex
//     with the larger free index and receives the edges between the two in creation order, added onto 0.0;
//   - chi2 and computeScale: item t belongs to lane t mod kEgTeam (256), xor butterfly over a wavefront, wavefronts in order;
//   - the factorisation: element (i, j) of the lower triangle receives a - l_ik * c_jk (eg_fnma: one multiply, one
//     subtract) for k ascending, l_ik = c_ik / d_k, ok iff every pivot is > 0; the substitutions as lba_solve has them.
// The Levenberg-Marquardt rule and the host replay of the team combine are orbhip_lm_core.h's; eg_lm_judge keeps the two
// buffers, the counters, fails0 / ORBHIP_EG_SINGULAR and the phases around the rule.
// Nothing here indexes a private array at run time.
#pragma once
#include "orbhip_sim3opt_core.h"

namespace orbhip {

#ifndef ORBHIP_EG_PANEL
#define ORBHIP_EG_PANEL 4                               // poses of a panel of the blocked factorisation: not part of the arithmetic;
                                                        // 4 measured faster than 8 (profiles/essgraph_stage.json)
#endif
constexpr int kEgMaxKf = ORBHIP_EG_MAX_KF;
constexpr int kEgPanel = ORBHIP_EG_PANEL, kEgNb = 7 * kEgPanel;
constexpr int kEgTeam = 256, kEgWave = 64;
constexpr int kEgMinFeat = 100;
constexpr int kEgEvals = 29;                            // 14 estimates of vertex 0, 14 of vertex 1, the estimate itself
constexpr int kEgRec = 162;                             // doubles of an edge record
constexpr int kEgHii = 0, kEgHjj = 49, kEgHij = 98, kEgBi = 147, kEgBj = 154, kEgChi = 161;
enum { kEgLc = 0, kEgTree, kEgLoop, kEgCovis };
enum { kEgDone = 0, kEgBuild, kEgTrial, kEgFinal };
enum { kEgCntIns = 4, kEgCntW, kEgCntNull, kEgCnts };   // after the four kinds

struct EgState {
    int phase, status, it, qmax, ok2, cur, fail, fails0;
    int nv, n_free, n, n_edges, loop_vtx, its, trials, n_pts, n_bad_lm, pad;
    int cnt[kEgCnts + 1];
    double lam, ni, current, ini, rho;
};

struct EgWs {
    // the tables (include/orbhip.h)
    const uint8_t *kf_bad;
    const int *kf_id, *parent, *conn_w, *ord_kf, *ord_w, *n_ord, *loop_start, *loop_kf, *lc_start, *lc_kf;
    const double *corrected, *non_corrected;
    const uint8_t *in_c, *in_nc, *flags;
    const int *ref_kf, *cby, *cref;
    float *Tcw, *world;
    int *o_point_list, *o_report;
    double *o_Scw, *o_Swc;
    int rows, pcap, cur, loop_row, fix_scale, max_edges;
    // the workspace
    EgState *S;
    int *row_vtx;                           // [rows]: vertex of a row or -1
    int *vtx_row, *vtx_free;                // [kEgMaxKf]: row of a vertex; its free index or -1
    int *row_e0;                            // [2][rows + 1]: where a row's edges of pass 0 / 1 start
    double *vScw, *est;                     // [mk][8], [2][mk][8]: the accepted estimate is buffer S->cur
    int *e_i, *e_j;                         // [max_edges]: vertices 0 and 1 of an edge
    double *meas, *D;                       // [max_edges][8]; [14][8]: Sim3(+-delta e_d)
    double *ev, *rec, *chi;                 // [max_edges][29][7], [max_edges][kEgRec], [max_edges]
    int *vf_e0, *vf_edges;                  // [mk + 1], [2 max_edges]: a free vertex's edges, ascending
    double *Hd, *bv, *xp, *y, *A;           // [mk][49], [n], [n], [n], [n][n]
};

PO_HD int eg_mk(const EgWs &W) { return W.rows < kEgMaxKf ? W.rows : kEgMaxKf; }
PO_HD bool eg_bad(const EgWs &W, int r) { return W.kf_bad && W.kf_bad[r]; }
PO_HD double eg_fnma(double a, double l, double c) { const double p = l * c; return a - p; }

// ---- det_log64: fdlibm's __ieee754_log with the word tests written as doubles ---------------------------------------------
constexpr double kLg1 = 6.666666666666735130e-01, kLg2 = 3.999999999940941908e-01, kLg3 = 2.857142874366239149e-01,
                 kLg4 = 2.222219843214978396e-01, kLg5 = 1.818357216161805012e-01, kLg6 = 1.531383769920937332e-01,
                 kLg7 = 1.479819860511658591e-01;
constexpr double kLogSplit = 1.4142112731933594;        // 1 + 0x6a09c / 2^20: mantissas from here on are halved
constexpr double kLogMidLo = 1.3799991607666016, kLogMidHi = 1.4200000762939453;
constexpr double kLogTiny = 9.5367431640625e-07;        // 2^-20
constexpr double kTwo54 = 18014398509481984.0, kDblMin = 2.2250738585072014e-308;

PO_HD double det_log64(double x)
{
    if (x != x) return x;
    if (x < 0) return __builtin_nan("");
    if (x == 0) return -__builtin_inf();
    if (x == __builtin_inf()) return x;
    int k = 0, e = 0;
    if (x < kDblMin) { x = x * kTwo54; k = -54; }
    double m = frexp(x, &e);
    m = m * 2.0;
    k = k + (e - 1);
    const bool mid = kLogMidLo <= m && m < kLogMidHi;
    if (m >= kLogSplit) { m = m * 0.5; k = k + 1; }
    const double f = m - 1.0, dk = (double)k;
    if (fabs(f) < kLogTiny) {
        if (f == 0) return k == 0 ? 0.0 : dk * kLn2Hi + dk * kLn2Lo;
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        return k == 0 ? f - R : dk * kLn2Hi - ((R - dk * kLn2Lo) - f);
    }
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (kLg2 + w * (kLg4 + w * kLg6)), t2 = z * (kLg1 + w * (kLg3 + w * (kLg5 + w * kLg7)));
    const double R = t2 + t1;
    if (mid) {
        const double hfsq = 0.5 * f * f;
        return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * kLn2Hi - ((hfsq - (s * (hfsq + R) + dk * kLn2Lo)) - f);
    }
    return k == 0 ? f - s * (f - R) : dk * kLn2Hi - ((s * (f - R) - dk * kLn2Lo) - f);
}

// ---- det_acos64: fdlibm's __ieee754_acos ------------------------------------------------------------------------------------
constexpr double kAcPio2Hi = 1.57079632679489655800e+00, kAcPio2Lo = 6.12323399573676603587e-17, kAcPi = 3.14159265358979311600e+00;
constexpr double kPS0 = 1.66666666666666657415e-01, kPS1 = -3.25565818622400915405e-01, kPS2 = 2.01212532134862925881e-01,
                 kPS3 = -4.00555345006794114027e-02, kPS4 = 7.91534994289814532176e-04, kPS5 = 3.47933107596021167570e-05;
constexpr double kQS1 = -2.40339491173441421878e+00, kQS2 = 2.02094576023350569471e+00, kQS3 = -6.88283971605453293030e-01,
                 kQS4 = 7.70381505559019352791e-02;
constexpr double kAcosTiny = 6.938893903907228e-18;     // 2^-57

PO_HD double eg_acos_r(double z)
{
    const double p = z * (kPS0 + z * (kPS1 + z * (kPS2 + z * (kPS3 + z * (kPS4 + z * kPS5)))));
    const double q = 1.0 + z * (kQS1 + z * (kQS2 + z * (kQS3 + z * kQS4)));
    return p / q;
}
PO_HD double eg_clear_low_word(double x)
{
    unsigned long long u;
    __builtin_memcpy(&u, &x, 8);
    u &= 0xffffffff00000000ull;
    __builtin_memcpy(&x, &u, 8);
    return x;
}
PO_HD double det_acos64(double x)
{
    if (x != x) return x;
    const double ax = fabs(x);
    if (ax >= 1.0) {
        if (ax == 1.0) return x > 0 ? 0.0 : kAcPi + 2.0 * kAcPio2Lo;
        return __builtin_nan("");
    }
    if (ax < 0.5) {
        if (ax <= kAcosTiny) return kAcPio2Hi + kAcPio2Lo;
        const double r = eg_acos_r(x * x);
        return kAcPio2Hi - (x - (kAcPio2Lo - x * r));
    }
    if (x < 0) {
        const double z = (1.0 + x) * 0.5, r = eg_acos_r(z), s = sqrt(z), w = r * s - kAcPio2Lo;
        return kAcPi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5, s = sqrt(z), df = eg_clear_low_word(s);
    const double c = (z - df * df) / (s + df), r = eg_acos_r(z), w = r * s + c;
    return 2.0 * (df + w);
}

// ---- Sim3::log (sim3.h:148-230) ---------------------------------------------------------------------------------------------
PO_HD void eg_swap4(double *a, double *b)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) { const double t = a[c]; a[c] = b[c]; b[c] = t; }
}
// W.lu().solve(t): partial pivoting, the largest |a| of the column, the first of equals
PO_HD void eg_lu3_solve(const double *Wm, const double *t, double *x)
{
    double r0[4] = {Wm[0], Wm[1], Wm[2], t[0]}, r1[4] = {Wm[3], Wm[4], Wm[5], t[1]}, r2[4] = {Wm[6], Wm[7], Wm[8], t[2]};
    int p = 0;
    if (fabs(r1[0]) > fabs(r0[0])) p = 1;
    if (fabs(r2[0]) > fabs(p == 1 ? r1[0] : r0[0])) p = 2;
    if (p == 1) eg_swap4(r0, r1);
    if (p == 2) eg_swap4(r0, r2);
    {
        const double l1 = r1[0] / r0[0], l2 = r2[0] / r0[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) { r1[j] = r1[j] - l1 * r0[j]; r2[j] = r2[j] - l2 * r0[j]; }
    }
    if (fabs(r2[1]) > fabs(r1[1])) eg_swap4(r1, r2);
    {
        const double l = r2[1] / r1[1];
        r2[2] = r2[2] - l * r1[2]; r2[3] = r2[3] - l * r1[3];
    }
    x[2] = r2[3] / r2[2];
    x[1] = (r1[3] - r1[2] * x[2]) / r1[1];
    x[0] = ((r0[3] - r0[1] * x[1]) - r0[2] * x[2]) / r0[0];
}
PO_HD void eg_sim3_log(const double *S, double *o)
{
    const double s = S[7], sigma = det_log64(s);
    double R[9];
    po_to_R(S, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    const bool near = d > 1 - eps;
    double om[3], A, B, Cc, theta = 0.0, theta2 = 0.0, sn = 0.0, cs = 0.0;
    if (near) {
        om[0] = 0.5 * dR[0]; om[1] = 0.5 * dR[1]; om[2] = 0.5 * dR[2];
    } else {
        theta = det_acos64(d);
        theta2 = theta * theta;
        const double f = theta / (2 * sqrt(1 - d * d));
        om[0] = f * dR[0]; om[1] = f * dR[1]; om[2] = f * dR[2];
        det_sincos64(theta, sn, cs);
    }
    if (fabs(sigma) < eps) {
        Cc = 1.0;
        if (near) { A = 1. / 2.; B = 1. / 6.; }
        else { A = (1 - cs) / theta2; B = (theta - sn) / (theta2 * theta); }
    } else {
        Cc = (s - 1) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (Cc - ((b - 1) * sigma + a * theta) / c) / theta2;              // "* 1. / (theta2)": the product with 1 is exact
        }
    }
    const double Om[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    double Om2[9], Wm[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
#pragma unroll
    for (int k = 0; k < 9; ++k) Wm[k] = (A * Om[k] + B * Om2[k]) + Cc * (k % 4 == 0 ? 1.0 : 0.0);
    o[0] = om[0]; o[1] = om[1]; o[2] = om[2];
    eg_lu3_solve(Wm, S + 4, o + 3);
    o[6] = sigma;
}
// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): log(C * v1 * v2^-1)
PO_HD void eg_edge_error(const double *meas, const double *Si, const double *Sj, double *err)
{
    double a[8], ji[8], b[8];
    s3o_mul(meas, Si, a);
    s3o_inverse(Sj, ji);
    s3o_mul(a, ji, b);
    eg_sim3_log(b, err);
}
PO_HD double eg_chi2(const double *e)
{
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) c = c + e[k] * e[k];
    return c;
}
PO_HD void eg_load8(const double *p, double *o)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = p[k];
}
PO_HD void eg_store8(double *p, const double *o)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = o[k];
}
PO_HD size_t eg_est_at(const EgWs &W, int buf, int v) { return ((size_t)buf * eg_mk(W) + v) * 8; }

// ---- a vertex ---------------------------------------------------------------------------------------------------------------
// :809-844: the corrected Sim3 where marked, otherwise Sim3(toMatrix3d(R), toVector3d(t), 1.0) of the float pose
PO_HD void eg_vertex_init(const EgWs &W, int v)
{
    const int r = W.vtx_row[v];
    double S[8];
    if (W.in_c[r]) eg_load8(W.corrected + (size_t)r * 8, S);
    else {
        const float *T = W.Tcw + (size_t)r * 12;
        const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8],
                             (double)T[9], (double)T[10]};
        po_quat_from_R(R, S);
        S[4] = (double)T[3]; S[5] = (double)T[7]; S[6] = (double)T[11]; S[7] = 1.0;
    }
    eg_store8(W.vScw + (size_t)v * 8, S);
    eg_store8(W.est + eg_est_at(W, 0, v), S);
    eg_store8(W.est + eg_est_at(W, 1, v), S);
}
PO_HD void eg_perturb_init(const EgWs &W, int q)               // q < 14: Sim3(+-delta e_d), d = q / 2
{
    double u[7], S[8];
    const int d = q >> 1;
    const double v = (q & 1) ? -kS3oDelta : kS3oDelta;
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = k == d ? v : 0.0;
    if (W.fix_scale) u[6] = 0.0;                               // VertexSim3Expmap::oplusImpl
    s3o_exp(u, S);
    eg_store8(W.D + q * 8, S);
}

// ---- a bank row's edges (:852-983) ----------------------------------------------------------------------------------------------
// Sjw of a "normal" edge: the non-corrected Sim3 where marked, else vScw
PO_HD void eg_row_sim3(const EgWs &W, int r, double *S)
{
    if (W.in_nc[r]) eg_load8(W.non_corrected + (size_t)r * 8, S);
    else eg_load8(W.vScw + (size_t)W.row_vtx[r] * 8, S);
}
// whether the loop-connection pass creates the edge i -> j
PO_HD bool eg_lc_created(const EgWs &W, int i, int j)
{
    if (eg_bad(W, i) || j < 0 || j >= W.rows || eg_bad(W, j) || i == j) return false;
    return !((i != W.cur || j != W.loop_row) && W.conn_w[(size_t)i * W.rows + j] < kEgMinFeat);
}
PO_HD bool eg_lc_lists(const EgWs &W, int i, int j)
{
    for (int o = W.lc_start[i]; o < W.lc_start[i + 1]; ++o)
        if (W.lc_kf[o] == j) return true;
    return false;
}
// sInsertedEdges.count of the pair
PO_HD bool eg_inserted(const EgWs &W, int a, int b)
{
    return (eg_lc_lists(W, a, b) && eg_lc_created(W, a, b)) || (eg_lc_lists(W, b, a) && eg_lc_created(W, b, a));
}
PO_HD void eg_put_edge(const EgWs &W, int at, int i, int j, const double *Sjw, const double *Swi)
{
    if (at >= W.max_edges) return;
    double m[8];
    s3o_mul(Sjw, Swi, m);
    W.e_i[at] = W.row_vtx[i]; W.e_j[at] = W.row_vtx[j];
    eg_store8(W.meas + (size_t)at * 8, m);
}
// The edges row r creates in pass 0 (loop connections) or pass 1 (spanning tree, old loop edges, covisibility), in the
// reference's order; written from `base` when write is set, counted into cnt [kEgCnts] otherwise.  Returns their number.
PO_HD int eg_row_edges(const EgWs &W, int r, int pass, int base, bool write, int *cnt)
{
    int ne = 0;
    double Swi[8], Sjw[8], t[8];
    if (pass == 0) {
        const int o0 = W.lc_start[r], o1 = W.lc_start[r + 1];
        if (o1 <= o0) return 0;
        if (write && !eg_bad(W, r)) { eg_load8(W.vScw + (size_t)W.row_vtx[r] * 8, t); s3o_inverse(t, Swi); }
        for (int o = o0; o < o1; ++o) {
            const int j = W.lc_kf[o];
            if (eg_bad(W, r) || j < 0 || j >= W.rows || eg_bad(W, j) || j == r) { if (!write) cnt[kEgCntNull]++; continue; }
            if (!eg_lc_created(W, r, j)) { if (!write) cnt[kEgCntW]++; continue; }
            if (write) { eg_load8(W.vScw + (size_t)W.row_vtx[j] * 8, Sjw); eg_put_edge(W, base + ne, r, j, Sjw, Swi); }
            else cnt[kEgLc]++;
            ++ne;
        }
        return ne;
    }
    if (eg_bad(W, r)) return 0;
    if (write) { eg_row_sim3(W, r, t); s3o_inverse(t, Swi); }
    const int p = W.parent[r];
    if (p >= 0) {
        if (p >= W.rows || eg_bad(W, p) || p == r) { if (!write) cnt[kEgCntNull]++; }
        else {
            if (write) { eg_row_sim3(W, p, Sjw); eg_put_edge(W, base + ne, r, p, Sjw, Swi); }
            else cnt[kEgTree]++;
            ++ne;
        }
    }
    const int l0 = W.loop_start[r], l1 = W.loop_start[r + 1];
    for (int o = l0; o < l1; ++o) {
        const int l = W.loop_kf[o];
        if (l < 0 || l >= W.rows || l == r) { if (!write) cnt[kEgCntNull]++; continue; }
        if (!(W.kf_id[l] < W.kf_id[r])) continue;
        if (eg_bad(W, l)) { if (!write) cnt[kEgCntNull]++; continue; }
        if (write) { eg_row_sim3(W, l, Sjw); eg_put_edge(W, base + ne, r, l, Sjw, Swi); }
        else cnt[kEgLoop]++;
        ++ne;
    }
    // KeyFrame::GetCovisiblesByWeight(100) as src/KeyFrame.cc:184-199 has it: nothing when no weight is below 100
    int no = W.n_ord[r], k100 = 0;
    no = no < 0 ? 0 : (no > W.rows ? W.rows : no);
    while (k100 < no && W.ord_w[(size_t)r * W.rows + k100] >= kEgMinFeat) ++k100;
    if (k100 == no) k100 = 0;
    for (int q = 0; q < k100; ++q) {
        const int n = W.ord_kf[(size_t)r * W.rows + q];
        if (n < 0 || n >= W.rows || n == r) continue;
        if (n == p || (W.parent[n] == r && !eg_bad(W, n))) continue;
        bool in_loops = false;
        for (int o = l0; o < l1; ++o) in_loops = in_loops || W.loop_kf[o] == n;
        if (in_loops || eg_bad(W, n) || !(W.kf_id[n] < W.kf_id[r])) continue;
        if (eg_inserted(W, r, n)) { if (!write) cnt[kEgCntIns]++; continue; }
        if (write) { eg_row_sim3(W, n, Sjw); eg_put_edge(W, base + ne, r, n, Sjw, Swi); }
        else cnt[kEgCovis]++;
        ++ne;
    }
    return ne;
}

// ---- an edge ------------------------------------------------------------------------------------------------------------------
// evaluation q of a linearisation (base_binary_edge.hpp:152-198): q < 14 perturbs vertex 0, q < 28 vertex 1, 28 is the
// estimate; a fixed vertex is skipped
PO_HD void eg_edge_eval(const EgWs &W, int e, int q)
{
    const int vi = W.e_i[e], vj = W.e_j[e], cur = W.S->cur;
    if ((q < 14 && W.vtx_free[vi] < 0) || (q >= 14 && q < 28 && W.vtx_free[vj] < 0)) return;
    double m[8], Si[8], Sj[8], Dq[8], P[8], err[7];
    eg_load8(W.meas + (size_t)e * 8, m);
    eg_load8(W.est + eg_est_at(W, cur, vi), Si);
    eg_load8(W.est + eg_est_at(W, cur, vj), Sj);
    if (q < 14) { eg_load8(W.D + q * 8, Dq); s3o_mul(Dq, Si, P); eg_edge_error(m, P, Sj, err); }
    else if (q < 28) { eg_load8(W.D + (q - 14) * 8, Dq); s3o_mul(Dq, Sj, P); eg_edge_error(m, Si, P, err); }
    else eg_edge_error(m, Si, Sj, err);
    double *o = W.ev + ((size_t)e * kEgEvals + q) * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) o[k] = err[k];
}
// entry (row k, column a) of the numeric Jacobian of end `end`
PO_HD double eg_jac(const double *ev, int end, int k, int a)
{
    return kS3oScalar * (ev[(end * 14 + 2 * a) * 7 + k] - ev[(end * 14 + 2 * a + 1) * 7 + k]);
}
// element t of the edge record (constructQuadraticForm, base_binary_edge.hpp:55-120, omega = I)
PO_HD void eg_edge_block(const EgWs &W, int e, int t)
{
    const double *ev = W.ev + (size_t)e * kEgEvals * 7;
    const bool fi = W.vtx_free[W.e_i[e]] >= 0, fj = W.vtx_free[W.e_j[e]] >= 0;
    double s = 0.0;
    if (t < kEgBi) {
        const int which = t / 49, ab = t - which * 49, a = ab / 7, b = ab - a * 7;
        const int ea = which == 1 ? 1 : 0, eb = which == 0 ? 0 : 1;
        if ((ea == 0 ? fi : fj) && (eb == 0 ? fi : fj))
            for (int k = 0; k < 7; ++k) s = s + eg_jac(ev, ea, k, a) * eg_jac(ev, eb, k, b);
    } else if (t < kEgChi) {
        const int end = t < kEgBj ? 0 : 1, a = t - (end ? kEgBj : kEgBi);
        if (end == 0 ? fi : fj)
            for (int k = 0; k < 7; ++k) s = s + eg_jac(ev, end, k, a) * -ev[28 * 7 + k];
    } else {
        s = eg_chi2(ev + 28 * 7);
    }
    W.rec[(size_t)e * kEgRec + t] = s;
}
// computeActiveErrors at the tried estimate
PO_HD void eg_trial_chi(const EgWs &W, int e)
{
    const int buf = 1 - W.S->cur;
    double m[8], Si[8], Sj[8], err[7];
    eg_load8(W.meas + (size_t)e * 8, m);
    eg_load8(W.est + eg_est_at(W, buf, W.e_i[e]), Si);
    eg_load8(W.est + eg_est_at(W, buf, W.e_j[e]), Sj);
    eg_edge_error(m, Si, Sj, err);
    W.chi[e] = eg_chi2(err);
}

// ---- a free vertex ------------------------------------------------------------------------------------------------------------
// element t < 49 of its diagonal block, t < 56 of its b: its edges in creation order
PO_HD void eg_vertex_block(const EgWs &W, int f, int v, int t)
{
    double s = 0.0;
    for (int k = W.vf_e0[f]; k < W.vf_e0[f + 1]; ++k) {
        const int e = W.vf_edges[k];
        const bool first = W.e_i[e] == v;
        const double *r = W.rec + (size_t)e * kEgRec;
        s = s + (t < 49 ? r[(first ? kEgHii : kEgHjj) + t] : r[(first ? kEgBi : kEgBj) + (t - 49)]);
    }
    if (t < 49) W.Hd[(size_t)f * 49 + t] = s;
    else W.bv[7 * f + (t - 49)] = s;
}
// its rows of the system at the current lambda: the diagonal block (lower triangle), the blocks left of it (A was zeroed),
// and its part of the right-hand side
PO_HD void eg_vertex_scatter(const EgWs &W, int f, int v, int t)
{
    const size_t ld = (size_t)W.S->n;
    if (t >= 49) { W.y[7 * f + (t - 49)] = W.bv[7 * f + (t - 49)]; return; }
    const int a = t / 7, b = t - a * 7;
    if (b <= a) {
        const double h = W.Hd[(size_t)f * 49 + t];
        W.A[(size_t)(7 * f + a) * ld + 7 * f + b] = a == b ? h + W.S->lam : h;
    }
    for (int k = W.vf_e0[f]; k < W.vf_e0[f + 1]; ++k) {
        const int e = W.vf_edges[k];
        const bool first = W.e_i[e] == v;
        const int g = W.vtx_free[first ? W.e_j[e] : W.e_i[e]];
        if (g < 0 || g >= f) continue;
        const double *r = W.rec + (size_t)e * kEgRec + kEgHij;
        double *dst = W.A + (size_t)(7 * f + a) * ld + 7 * g + b;
        *dst = *dst + (first ? r[a * 7 + b] : r[b * 7 + a]);
    }
}
// the update of a vertex: exp(x) * estimate for a free vertex, the same bits for the fixed one.  oplusImpl zeroes the scale
// entry in the solver's own vector.
PO_HD void eg_vertex_update(const EgWs &W, int v)
{
    const int cur = W.S->cur, f = W.vtx_free[v];
    double e[8], o[8];
    eg_load8(W.est + eg_est_at(W, cur, v), e);
    if (f >= 0) {
        double u[7], d[8];
        if (W.fix_scale) W.xp[7 * f + 6] = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = W.xp[7 * f + k];
        s3o_exp(u, d);
        s3o_mul(d, e, o);
        eg_store8(W.est + eg_est_at(W, 1 - cur, v), o);
    } else {
        eg_store8(W.est + eg_est_at(W, 1 - cur, v), e);
    }
}

// ---- the team sums ----------------------------------------------------------------------------------------------------------
constexpr int kEgSumLin = 0, kEgSumTrial = 1, kEgSumScale = 2;
PO_HD double eg_sum_lane(const EgWs &W, int kind, int lane)
{
    const int items = kind == kEgSumScale ? W.S->n : W.S->n_edges;
    const double lam = W.S->lam;
    double acc = 0.0;
    for (int t = lane; t < items; t += kEgTeam) {
        if (kind == kEgSumLin) acc = acc + W.rec[(size_t)t * kEgRec + kEgChi];
        else if (kind == kEgSumTrial) acc = acc + W.chi[t];
        else { const double x = W.xp[t]; acc = acc + x * (lam * x + W.bv[t]); }
    }
    return acc;
}

// ---- the serial state machine (optimization_algorithm_levenberg.cpp with setUserLambdaInit(1e-16)) -----------------------------
PO_HD void eg_begin(EgWs &W)
{
    EgState &S = *W.S;
    if (S.status == ORBHIP_EG_CAPACITY) { S.phase = kEgFinal; return; }
    S.phase = (S.n_edges > 0 && S.n > 0) ? kEgBuild : kEgFinal;
}
PO_HD void eg_lm_begin(EgWs &W, double chi)
{
    EgState &S = *W.S;
    if (S.it == 0) S.fails0 = 0;
    lm_begin(S, chi, 1e-16);
    S.phase = kEgTrial;
}
PO_HD void eg_lm_judge(EgWs &W, double temp, double scale)
{
    EgState &S = *W.S;
    if (!S.ok2 && S.it == 0) S.fails0 = S.fails0 + 1;
    // discardTop: the tried estimate stands; pop: the other buffer is overwritten by the next trial
    if (lm_gain(S, S.ok2 != 0, temp, scale)) S.cur = 1 - S.cur;
    S.trials = S.trials + 1;
    S.fail = 0;
    if (lm_retry(S)) return;                                                       // another trial
    S.its = S.its + 1;
    if (S.it == 0 && S.fails0 == S.qmax) S.status = ORBHIP_EG_SINGULAR;
    S.it = S.it + 1;
    S.phase = (lm_iteration_ok(S) && S.it < 20) ? kEgBuild : kEgFinal;
}

// ---- the epilogue (:991-1043) ---------------------------------------------------------------------------------------------------
PO_HD void eg_write_pose(const EgWs &W, int v)
{
    const int r = W.vtx_row[v];
    double S[8], Si[8], R[9];
    eg_load8(W.est + eg_est_at(W, W.S->cur, v), S);
    s3o_inverse(S, Si);
    eg_store8(W.o_Swc + (size_t)r * 8, Si);
    eg_load8(W.vScw + (size_t)v * 8, Si);
    eg_store8(W.o_Scw + (size_t)r * 8, Si);
    po_to_R(S, R);
    const double m = 1. / S[7];
    float *T = W.Tcw + (size_t)r * 12;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[a * 4 + c] = (float)R[a * 3 + c];
        T[a * 4 + 3] = (float)(S[4 + a] * m);
    }
}
PO_HD void eg_sim3_map(const double *S, const double *X, double *o)
{
    double r[3];
    po_quat_rot(S, X, r);
    o[0] = S[7] * r[0] + S[4]; o[1] = S[7] * r[1] + S[5]; o[2] = S[7] * r[2] + S[6];
}
// a present point: correctedSwr.map(Srw.map(P)); a reference row that is bad or out of range holds default Sim3s both ways
PO_HD void eg_write_point(const EgWs &W, int p)
{
    const int r = W.cby[p] == W.cur ? W.cref[p] : W.ref_kf[p];
    if (r < 0 || r >= W.rows || eg_bad(W, r)) return;
    const int v = W.row_vtx[r];
    double Srw[8], S[8], Swr[8], a[3], b[3];
    float *Xf = W.world + (size_t)p * 3;
    const double X[3] = {(double)Xf[0], (double)Xf[1], (double)Xf[2]};
    eg_load8(W.vScw + (size_t)v * 8, Srw);
    eg_load8(W.est + eg_est_at(W, W.S->cur, v), S);
    s3o_inverse(S, Swr);
    eg_sim3_map(Srw, X, a);
    eg_sim3_map(Swr, a, b);
    Xf[0] = (float)b[0]; Xf[1] = (float)b[1]; Xf[2] = (float)b[2];
}
PO_HD void eg_write_report(const EgWs &W)
{
    const EgState &S = *W.S;
    int *r = W.o_report;
    r[0] = S.status; r[1] = S.nv; r[2] = S.cnt[kEgLc]; r[3] = S.cnt[kEgTree]; r[4] = S.cnt[kEgLoop]; r[5] = S.cnt[kEgCovis];
    r[6] = S.cnt[kEgCntIns]; r[7] = S.cnt[kEgCntW]; r[8] = S.its; r[9] = S.trials; r[10] = S.n; r[11] = S.n_pts;
    r[12] = S.cnt[kEgCntNull]; r[13] = 0; r[14] = 0; r[15] = 0;
}

// ---- the workspace: carved from one allocation, 256-byte pieces; base == nullptr only sizes it ----------------------------
inline size_t eg_carve(EgWs &W, uint8_t *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t R = (size_t)W.rows, K = (size_t)eg_mk(W), E = (size_t)W.max_edges, n = 7 * K;
    W.S = (EgState *)take(sizeof(EgState));
    W.row_vtx = (int *)take(R * 4); W.vtx_row = (int *)take(K * 4); W.vtx_free = (int *)take(K * 4);
    W.row_e0 = (int *)take(2 * (R + 1) * 4);
    W.vScw = (double *)take(K * 64); W.est = (double *)take(2 * K * 64);
    W.e_i = (int *)take(E * 4); W.e_j = (int *)take(E * 4);
    W.meas = (double *)take(E * 64); W.D = (double *)take(14 * 64);
    W.ev = (double *)take(E * kEgEvals * 7 * 8); W.rec = (double *)take(E * kEgRec * 8); W.chi = (double *)take(E * 8);
    W.vf_e0 = (int *)take((K + 1) * 4); W.vf_edges = (int *)take(2 * E * 4);
    W.Hd = (double *)take(K * 49 * 8); W.bv = (double *)take(n * 8); W.xp = (double *)take(n * 8); W.y = (double *)take(n * 8);
    W.A = (double *)take(n * n * 8);
    return off;
}

// ---- one host thread ------------------------------------------------------------------------------------------------------
inline double eg_host_team_sum(const EgWs &W, int kind)
{
    double lanes[kEgTeam][1], total;
    for (int l = 0; l < kEgTeam; ++l) lanes[l][0] = eg_sum_lane(W, kind, l);
    host_team_combine<kEgTeam, 1>(lanes, 0, &total, TeamAdd());
    return total;
}
// the vertices and the edges (:809-983), sequentially
inline void eg_host_setup(EgWs &W)
{
    EgState &S = *W.S;
    memset(&S, 0, sizeof(S));
    int nv = 0;
    for (int r = 0; r < W.rows; ++r) {
        W.row_vtx[r] = -1;
        if (eg_bad(W, r)) continue;
        if (nv < kEgMaxKf) { W.row_vtx[r] = nv; W.vtx_row[nv] = r; }
        ++nv;
    }
    S.nv = nv; S.loop_vtx = -1;
    if (nv > kEgMaxKf) { S.status = ORBHIP_EG_CAPACITY; return; }
    int nf = 0;
    for (int v = 0; v < nv; ++v) {
        if (W.vtx_row[v] == W.loop_row) { W.vtx_free[v] = -1; S.loop_vtx = v; }
        else W.vtx_free[v] = nf++;
        eg_vertex_init(W, v);
    }
    S.n_free = nf; S.n = 7 * nf;
    for (int q = 0; q < 14; ++q) eg_perturb_init(W, q);
    int ne = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int r = 0; r < W.rows; ++r) {
            eg_row_edges(W, r, pass, 0, false, S.cnt);
            ne += eg_row_edges(W, r, pass, ne, true, S.cnt);
        }
    S.n_edges = ne;
    if (ne > W.max_edges) { S.status = ORBHIP_EG_CAPACITY; return; }
    for (int f = 0; f <= nf; ++f) W.vf_e0[f] = 0;
    int k = 0;
    for (int v = 0; v < nv; ++v) {
        const int f = W.vtx_free[v];
        if (f < 0) continue;
        W.vf_e0[f] = k;
        for (int e = 0; e < ne; ++e)
            if (W.e_i[e] == v || W.e_j[e] == v) W.vf_edges[k++] = e;
        W.vf_e0[f + 1] = k;
    }
    for (int t = 0; t < S.n; ++t) W.xp[t] = 0.0;
}
// the unpivoted LDLt of lba_solve on one thread, the scaled column kept below the diagonal
inline bool eg_host_solve(const EgWs &W)
{
    const int n = W.S->n;
    const size_t ld = (size_t)n;
    double *A = W.A, *y = W.y;
    for (int k = 0; k < n; ++k) {
        const double d = A[k * ld + k];
        if (!(d > 0)) return false;
        for (int i = k + 1; i < n; ++i) {
            const double l = A[i * ld + k] / d;
            for (int j = k + 1; j <= i; ++j) A[i * ld + j] = eg_fnma(A[i * ld + j], l, A[j * ld + k]);
        }
        for (int i = k + 1; i < n; ++i) A[i * ld + k] = A[i * ld + k] / d;
    }
    for (int j = 0; j < n; ++j)
        for (int i = j + 1; i < n; ++i) y[i] = eg_fnma(y[i], A[i * ld + j], y[j]);
    for (int i = 0; i < n; ++i) y[i] = y[i] / A[i * ld + i];
    for (int j = n - 1; j > 0; --j)
        for (int i = 0; i < j; ++i) y[i] = eg_fnma(y[i], A[j * ld + i], y[j]);
    return true;
}
// the list of the present points in index order, and their correction
inline void eg_host_points(EgWs &W)
{
    int np = 0;
    for (int p = 0; p < W.pcap; ++p) {
        if (!(W.flags[p] & ORBHIP_POINT_PRESENT)) continue;
        W.o_point_list[np++] = p;
        eg_write_point(W, p);
    }
    W.S->n_pts = np;
}

struct EgHostTrace {                        // what tests/cpp/essgraph_host.cpp dumps: the tried estimates of every trial
    double *tried;                          // [max_trials][mk][8] or null
    int max_trials, n_trials;
};

// the whole function on one thread, phase by phase as the device enqueues it
inline void eg_host_run(EgWs &W, EgHostTrace *trace = nullptr)
{
    EgState &S = *W.S;
    eg_host_setup(W);
    eg_begin(W);
    while (S.phase != kEgDone) {
        if (S.phase == kEgBuild) {
            for (int e = 0; e < S.n_edges; ++e)
                for (int q = 0; q < kEgEvals; ++q) eg_edge_eval(W, e, q);
            for (int e = 0; e < S.n_edges; ++e)
                for (int t = 0; t < kEgRec; ++t) eg_edge_block(W, e, t);
            for (int v = 0; v < S.nv; ++v)
                if (W.vtx_free[v] >= 0)
                    for (int t = 0; t < 56; ++t) eg_vertex_block(W, W.vtx_free[v], v, t);
            eg_lm_begin(W, eg_host_team_sum(W, kEgSumLin));
        } else if (S.phase == kEgTrial) {
            const size_t nn = (size_t)S.n * S.n;
            for (size_t k = 0; k < nn; ++k) W.A[k] = 0.0;
            for (int v = 0; v < S.nv; ++v)
                if (W.vtx_free[v] >= 0)
                    for (int t = 0; t < 56; ++t) eg_vertex_scatter(W, W.vtx_free[v], v, t);
            S.ok2 = eg_host_solve(W) ? 1 : 0;
            if (S.ok2) for (int t = 0; t < S.n; ++t) W.xp[t] = W.y[t];
            for (int v = 0; v < S.nv; ++v) eg_vertex_update(W, v);
            if (trace && trace->tried && trace->n_trials < trace->max_trials) {
                for (int v = 0; v < S.nv; ++v)
                    eg_load8(W.est + eg_est_at(W, 1 - S.cur, v), trace->tried + ((size_t)trace->n_trials * eg_mk(W) + v) * 8);
                trace->n_trials++;
            }
            for (int e = 0; e < S.n_edges; ++e) eg_trial_chi(W, e);
            const double chi = eg_host_team_sum(W, kEgSumTrial), scale = eg_host_team_sum(W, kEgSumScale);
            eg_lm_judge(W, chi, scale);
        } else {                                                                   // kEgFinal
            if (S.status != ORBHIP_EG_CAPACITY) {
                for (int v = 0; v < S.nv; ++v) eg_write_pose(W, v);
                eg_host_points(W);
            }
            eg_write_report(W);
            S.phase = kEgDone;
        }
    }
}

}  // namespace orbhip
