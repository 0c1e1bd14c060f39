// Optimizer::BundleAdjustment (src/Optimizer.cc:49-237; GlobalBundleAdjustemnt :41-46 is the call with null lists) and the map
// update of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:676-737), operation by operation what
// tests/seqref/gba.py does.  The edges, the blocks, the Schur complement, the Levenberg-Marquardt state
// machine and the team sums are orbhip_lba_core.h's (the rule itself and the combine: orbhip_lm_core.h), run as one round of
// optimize(iterations) (LbaWs::single_its); this file adds what differs: the vertices and edges of a whole map, the write-back
// of the two modes, and the apply step.
//
// The same text serves the kernels of orbhip_gba.hip and one host thread (gba_host_run, gba_apply_host).
//   - vertices: the listed rows that are not bad, in list order; the free poses of the reduced system are these with the rows of
//     kf_id == 0 left out, in the same order;
//   - points: the listed points that are PRESENT and have at least one edge, in list order; a point's edges are its
//     observations in table order whose row is not bad, has kf_id <= maxKFid and is a vertex;
//   - float products of the apply step: fp32, per row, left to right (gba_mul44, gba_inverse).
#pragma once
#include "orbhip_lba_core.h"

namespace orbhip {

constexpr int kGbaMaxKf = ORBHIP_GBA_MAX_KF;
constexpr int kGbaPanel = 4, kGbaNb = 6 * kGbaPanel;    // poses, columns of a panel of the blocked factorisation

struct GbaCount {
    int max_kfid, n_removed, n_skipped, n_null, n_listed, pad[3];
};

struct GbaWs {
    LbaWs L;                                // tables, scalars, the state record and the workspace of the optimisation
    const int *kf_id;                       // [rows]: mnId
    const int *kf_list, *pt_list;           // [nkf], [npt] or null: every row / every point index
    int nkf, npt, mode;
    float *TcwGBA, *posGBA;                 // ORBHIP_GBA_STAGED: [rows][12], [pcap][3]
    uint8_t *kf_mark, *pt_mark;             // ORBHIP_GBA_STAGED: [rows], [pcap]
    int *o_point_list, *o_report;           // ORBHIP_GBA_IN_PLACE: [max_points]; [16]
    // the workspace beyond LbaWs
    GbaCount *C;
    int *e_free;                            // [max_edges]: the free pose of an edge or -1
    uint8_t *cov;                           // [max_free][max_free]: (i1, i2), i1 <= i2, share a point
};

PO_HD int gba_nkf(const GbaWs &G) { return G.kf_list ? G.nkf : G.L.rows; }
PO_HD int gba_npt(const GbaWs &G) { return G.pt_list ? G.npt : G.L.np; }
PO_HD int gba_kf_at(const GbaWs &G, int i) { return G.kf_list ? G.kf_list[i] : i; }
PO_HD int gba_pt_at(const GbaWs &G, int i) { return G.pt_list ? G.pt_list[i] : i; }
PO_HD bool gba_row_good(const GbaWs &G, int r) { return r >= 0 && r < G.L.rows && !(G.L.kf_bad && G.L.kf_bad[r]); }
PO_HD bool gba_point_listed(const GbaWs &G, int p) { return p >= 0 && p < G.L.np && (G.L.flags[p] & ORBHIP_POINT_PRESENT); }

// An observation of a listed point: 0 an edge, 1 skipped by the bad / maxKFid rule (:109), 2 a null vertex (the row is in the
// map and old enough but is not listed)
PO_HD int gba_obs_kind(const GbaWs &G, int o, int max_kfid)
{
    const int r = G.L.obs_kf[o];
    if (!gba_row_good(G, r) || G.kf_id[r] > max_kfid) return 1;
    return G.L.kf_vtx[r] < 0 ? 2 : 0;
}
PO_HD bool gba_obs_stereo(const GbaWs &G, int o)
{
    const LbaWs &W = G.L;
    return W.u_right && !(W.u_right[(size_t)W.obs_kf[o] * W.cap + W.obs_idx[o]] < 0);
}
PO_HD void gba_edge_write(const GbaWs &G, int j, int o, int i)
{
    const LbaWs &W = G.L;
    const int v = W.kf_vtx[W.obs_kf[o]];
    W.e_vtx[j] = v; W.e_idx[j] = W.obs_idx[o]; W.e_pt[j] = i; W.e_fl[j] = gba_obs_stereo(G, o) ? kLbaStereo : 0;
    W.eb[(size_t)j * kLbaRec + kLbaChi2] = 0.0;
    G.e_free[j] = W.vtx_free[v];
}
PO_HD void gba_point_init(const GbaWs &G, int i, int p)
{
    const LbaWs &W = G.L;
    W.lpt[i] = p; W.pt_active[i] = 1;
    for (int k = 0; k < 3; ++k) {
        const double x = (double)W.world[(size_t)p * 3 + k];
        W.pt[lba_pt_at(W, 0, i) + k] = x; W.pt[lba_pt_at(W, 1, i) + k] = x;
        W.xl[(size_t)i * 3 + k] = 0.0;
    }
}
PO_HD void gba_vertex_init(const GbaWs &G, int v)
{
    const LbaWs &W = G.L;
    double q[7];
    po_pose_from_Tcw(W.Tcw + (size_t)W.vtx_row[v] * 12, q);
    for (int k = 0; k < 7; ++k) { W.pose[lba_pose_at(W, 0, v) + k] = q[k]; W.pose[lba_pose_at(W, 1, v) + k] = q[k]; }
}

// after the setup: initializeOptimization and the first look at the loop condition of optimize()
PO_HD void gba_begin(GbaWs &G)
{
    LbaWs &W = G.L;
    LbaState &S = *W.S;
    if (S.status == ORBHIP_GBA_CAPACITY) { S.phase = kLbaFinal; return; }
    S.round = 0; S.it = 0; S.ok2 = 1;
    if (S.n_active == 0) { S.phase = kLbaFinal; return; }                          // no vertex to optimise: optimize() returns at once
    lba_iter_top(W, true);
    if (S.phase == kLbaFinal) S.status = ORBHIP_GBA_STOPPED;                       // the stop byte was set on entry
}

// ---- the write-back (:193-235) ------------------------------------------------------------------------------------------------
PO_HD bool gba_writes(const LbaState &S) { return S.status != ORBHIP_GBA_CAPACITY; }
PO_HD void gba_write_pose(const GbaWs &G, int v)
{
    const LbaWs &W = G.L;
    const size_t vo = lba_pose_at(W, W.S->cur, v);
    double q[4], R[9];
    for (int k = 0; k < 4; ++k) q[k] = W.pose[vo + k];
    po_to_R(q, R);
    const int row = W.vtx_row[v];
    float *T = (G.mode == ORBHIP_GBA_STAGED ? G.TcwGBA : W.Tcw) + (size_t)row * 12;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)R[r * 3 + c];
        T[r * 4 + 3] = (float)W.pose[vo + 4 + r];
    }
    if (G.mode == ORBHIP_GBA_STAGED) G.kf_mark[row] = 1;
}
PO_HD void gba_write_point(const GbaWs &G, int i)
{
    const LbaWs &W = G.L;
    const size_t po = lba_pt_at(W, W.S->cur, i);
    const int p = W.lpt[i];
    float *X = (G.mode == ORBHIP_GBA_STAGED ? G.posGBA : W.world) + (size_t)p * 3;
    X[0] = (float)W.pt[po]; X[1] = (float)W.pt[po + 1]; X[2] = (float)W.pt[po + 2];
    if (G.mode == ORBHIP_GBA_STAGED) G.pt_mark[p] = 1;
    else G.o_point_list[i] = p;
}
PO_HD void gba_write_report(const GbaWs &G)
{
    const LbaState &S = *G.L.S;
    const GbaCount &C = *G.C;
    int *r = G.o_report;
    r[0] = S.status; r[1] = S.n_lkf; r[2] = S.n_free; r[3] = S.n_pts; r[4] = C.n_removed; r[5] = S.n_mono; r[6] = S.n_stereo;
    r[7] = C.n_skipped; r[8] = C.n_null; r[9] = S.its[0]; r[10] = S.trials[0]; r[11] = 6 * S.n_free; r[12] = C.n_listed;
    r[13] = 0; r[14] = 0; r[15] = S.samples;
}

// ---- the workspace: LbaWs's, then three more pieces ------------------------------------------------------------------------------
inline size_t gba_carve(GbaWs &G, uint8_t *base)
{
    LbaWs &W = G.L;
    W.max_free = W.rows < kGbaMaxKf ? (W.rows < 1 ? 1 : W.rows) : kGbaMaxKf;
    size_t off = lba_carve(W, base);
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    G.C = (GbaCount *)take(sizeof(GbaCount));
    G.e_free = (int *)take((size_t)W.max_edges * 4);
    G.cov = take((size_t)W.max_free * W.max_free);
    return off;
}

// ---- one host thread ---------------------------------------------------------------------------------------------------------
inline void gba_host_setup(GbaWs &G)
{
    LbaWs &W = G.L;
    LbaState &S = *W.S;
    GbaCount &C = *G.C;
    memset(&S, 0, sizeof(S));
    memset(&C, 0, sizeof(C));
    for (int r = 0; r < W.rows; ++r) { W.kf_vtx[r] = -1; W.vtx_free[r] = -1; }
    int nv = 0, nfree = 0, max_kfid = 0;
    for (int i = 0; i < gba_nkf(G); ++i) {
        const int r = gba_kf_at(G, i);
        if (!gba_row_good(G, r)) continue;
        if (nv < W.rows && nv < kGbaMaxKf) {
            W.lkf[nv] = r; W.vtx_row[nv] = r; W.kf_vtx[r] = nv;
            W.vtx_free[nv] = G.kf_id[r] == 0 ? -1 : nfree++;
        }
        if (G.kf_id[r] > max_kfid) max_kfid = G.kf_id[r];
        ++nv;
    }
    S.n_lkf = nv; S.n_free = nfree; C.max_kfid = max_kfid;
    if (nv > kGbaMaxKf) { S.n_free = 0; S.status = ORBHIP_GBA_CAPACITY; return; }
    int npts = 0, ne = 0, nm = 0, ns = 0;
    for (int i = 0; i < gba_npt(G); ++i) {
        const int p = gba_pt_at(G, i);
        if (!gba_point_listed(G, p)) continue;
        const int e0 = ne;
        for (int o = W.obs_start[p]; o < W.obs_start[p + 1]; ++o) {
            const int kind = gba_obs_kind(G, o, max_kfid);
            if (kind == 1) { C.n_skipped++; continue; }
            if (kind == 2) { C.n_null++; continue; }
            if (ne < W.max_edges && npts < W.max_points) gba_edge_write(G, ne, o, npts);
            if (gba_obs_stereo(G, o)) ++ns; else ++nm;
            ++ne;
        }
        if (ne == e0) { C.n_removed++; continue; }                                 // vbNotIncludedMP
        if (npts < W.max_points) { W.pt_e0[npts] = e0 < W.max_edges ? e0 : W.max_edges; gba_point_init(G, npts, p); }
        ++npts;
    }
    S.n_pts = npts; S.n_edges = ne; S.n_mono = nm; S.n_stereo = ns;
    if (npts > W.max_points || ne > W.max_edges) { S.status = ORBHIP_GBA_CAPACITY; return; }
    W.pt_e0[npts] = ne;
    for (int f = 0; f <= nfree; ++f) W.kf_e0[f] = 0;
    for (int j = 0; j < ne; ++j) if (G.e_free[j] >= 0) W.kf_e0[G.e_free[j] + 1]++;
    int poses = 0;
    for (int f = 0; f < nfree; ++f) { W.pose_active[f] = W.kf_e0[f + 1] > 0 ? 1 : 0; poses += W.pose_active[f]; W.kf_e0[f + 1] += W.kf_e0[f]; }
    for (int f = 0; f < nfree; ++f) {                                              // each free pose's edges, ascending
        int k = W.kf_e0[f];
        for (int j = 0; j < ne; ++j) if (G.e_free[j] == f) W.kf_edges[k++] = j;
    }
    for (int v = 0; v < nv; ++v) gba_vertex_init(G, v);
    for (int k = 0; k < 6 * nfree; ++k) W.xp[k] = 0.0;
    S.n_active = ne; S.poses[0] = poses;
}

inline void gba_host_run(GbaWs &G)
{
    LbaWs &W = G.L;
    LbaState &S = *W.S;
    gba_host_setup(G);
    gba_begin(G);
    while (S.phase != kLbaDone) {
        if (S.phase == kLbaBuild) lba_host_build(W);
        else if (S.phase == kLbaTrial) lba_host_trial(W);
        else {                                                                     // kLbaFinal
            if (gba_writes(S)) {
                for (int v = 0; v < S.n_lkf; ++v) gba_write_pose(G, v);
                for (int i = 0; i < S.n_pts; ++i) gba_write_point(G, i);
                G.C->n_listed = G.mode == ORBHIP_GBA_IN_PLACE ? S.n_pts : 0;
            }
            gba_write_report(G);
            S.phase = kLbaDone;
        }
    }
}

// ---- the apply step (src/LoopClosing.cc:676-737) --------------------------------------------------------------------------------
struct GbaApply {
    const int *origins, *parent;            // [n_origins], [rows]
    const uint8_t *kf_bad;                  // [rows] or null
    uint8_t *kf_mark;                       // [rows], in/out
    float *TcwGBA, *Tcw, *TcwBef;           // [rows][12]: in/out, in/out, out
    const uint8_t *pt_mark, *flags;         // [pcap]
    const float *posGBA;                    // [pcap][3]
    const int *ref_kf;                      // [pcap]
    float *world;                           // [pcap][3], in/out
    int *o_report;                          // [8]
    int n_origins, rows, pcap;
    // the workspace
    int *queue;                             // [rows]: lpKFtoCheck; an entry past `rows` could never be popped
    uint8_t *visited;                       // [rows]: TcwBefGBA of the row is written
    int *cnt;                               // [8]: the report while it is counted
};
inline size_t gba_apply_carve(GbaApply &A, uint8_t *base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    A.queue = (int *)take((size_t)A.rows * 4); A.visited = take((size_t)A.rows); A.cnt = (int *)take(8 * 4);
    return off;
}

// KeyFrame::SetPose: Rwc = Rcw^T, Ow = -Rwc * tcw, per row ((-a0 x + -a1 y) + -a2 z) in fp32
PO_HD void gba_inverse(const float *T, float *Twc)
{
    for (int r = 0; r < 3; ++r) {
        const float a0 = T[r], a1 = T[4 + r], a2 = T[8 + r];
        Twc[r * 4] = a0; Twc[r * 4 + 1] = a1; Twc[r * 4 + 2] = a2;
        Twc[r * 4 + 3] = ((-a0) * T[3] + (-a1) * T[7]) + (-a2) * T[11];
    }
}
// a 4x4 cv::Mat product of two [R | t; 0 0 0 1]: element (i, j) = ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) + a_i3 b_3j in fp32 with
// the last row of b as it stands (0 0 0 1); the last row of the product is 0 0 0 1 exactly and is not stored
PO_HD void gba_mul44(const float *a, const float *b, float *c)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            const float b3 = j == 3 ? 1.f : 0.f;
            c[i * 4 + j] = ((a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j]) + a[i * 4 + 2] * b[8 + j]) + a[i * 4 + 3] * b3;
        }
}
PO_HD bool gba_apply_row_good(const GbaApply &A, int r) { return r >= 0 && r < A.rows && !(A.kf_bad && A.kf_bad[r]); }
// an origin the walk starts from: in the map and holding a TcwGBA
PO_HD bool gba_apply_origin(const GbaApply &A, int r) { return gba_apply_row_good(A, r) && A.kf_mark[r] != 0; }
// a child c of the popped row k whose mark is clear: pChild->mTcwGBA = (pChild->GetPose() * Twc) * pKF->mTcwGBA
PO_HD void gba_apply_child(const GbaApply &A, int k, int c, const float *Twc)
{
    float Tcc[12], out[12];
    gba_mul44(A.Tcw + (size_t)c * 12, Twc, Tcc);
    gba_mul44(Tcc, A.TcwGBA + (size_t)k * 12, out);
    for (int q = 0; q < 12; ++q) A.TcwGBA[(size_t)c * 12 + q] = out[q];
    A.kf_mark[c] = 1;
}
// pKF->mTcwBefGBA = pKF->GetPose(); pKF->SetPose(pKF->mTcwGBA)
PO_HD void gba_apply_set_pose(const GbaApply &A, int k)
{
    for (int q = 0; q < 12; ++q) { A.TcwBef[(size_t)k * 12 + q] = A.Tcw[(size_t)k * 12 + q]; A.Tcw[(size_t)k * 12 + q] = A.TcwGBA[(size_t)k * 12 + q]; }
    A.visited[k] = 1;
}
// a point (:705-737): 0 not present, 1 set from posGBA, 2 moved through its reference row, 3 left
PO_HD int gba_apply_point(const GbaApply &A, int p)
{
    if (!(A.flags[p] & ORBHIP_POINT_PRESENT)) return 0;
    float *X = A.world + (size_t)p * 3;
    if (A.pt_mark[p]) {
        X[0] = A.posGBA[(size_t)p * 3]; X[1] = A.posGBA[(size_t)p * 3 + 1]; X[2] = A.posGBA[(size_t)p * 3 + 2];
        return 1;
    }
    const int r = A.ref_kf[p];
    if (r < 0 || r >= A.rows || !A.kf_mark[r] || !A.visited[r]) return 3;
    const float *B = A.TcwBef + (size_t)r * 12;
    float Xc[3], Twc[12];
    for (int i = 0; i < 3; ++i) Xc[i] = ((B[i * 4] * X[0] + B[i * 4 + 1] * X[1]) + B[i * 4 + 2] * X[2]) + B[i * 4 + 3];
    gba_inverse(A.Tcw + (size_t)r * 12, Twc);
    float o[3];
    for (int i = 0; i < 3; ++i) o[i] = ((Twc[i * 4] * Xc[0] + Twc[i * 4 + 1] * Xc[1]) + Twc[i * 4 + 2] * Xc[2]) + Twc[i * 4 + 3];
    X[0] = o[0]; X[1] = o[1]; X[2] = o[2];
    return 2;
}

inline void gba_apply_host(GbaApply &A)
{
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < A.rows; ++r) A.visited[r] = 0;
    int head = 0, tail = 0;
    for (int i = 0; i < A.n_origins; ++i)
        if (gba_apply_origin(A, A.origins[i]) && tail < A.rows) A.queue[tail++] = A.origins[i];
    while (head < tail) {                                                          // at most `rows` pops: the queue holds no more
        const int k = A.queue[head++];
        float Twc[12];
        gba_inverse(A.Tcw + (size_t)k * 12, Twc);
        for (int c = 0; c < A.rows; ++c) {
            if (A.parent[c] != k || !gba_apply_row_good(A, c)) continue;
            if (!A.kf_mark[c]) { gba_apply_child(A, k, c, Twc); cnt[1]++; }
            if (tail < A.rows) A.queue[tail++] = c;
        }
        gba_apply_set_pose(A, k);
        cnt[0]++;
    }
    for (int p = 0; p < A.pcap; ++p) {
        const int kind = gba_apply_point(A, p);
        if (kind) { cnt[5]++; cnt[1 + kind]++; }
    }
    for (int k = 0; k < 8; ++k) A.o_report[k] = cnt[k];
}

}  // namespace orbhip
