// Sim3 optimisation on the device: Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) for the current key frame and C
// loop candidates (include/orbhip.h, section "Sim3 optimisation").  gfx950 only, wave64.  The arithmetic is
// tests/seqref/sim3opt.py operation by operation; the function itself is orbhip_sim3opt_core.h,
// which the host can replay bit for bit.
//
// One launch on the caller's stream:
//   k_optimize_sim3   one workgroup of kS3oTeam lanes per candidate: the skip rules per slot of the current key frame and the
//                     ordered compaction of the kept slots (scan per wavefront, wavefront totals through LDS), two rounds
//                     of Levenberg-Marquardt with the check after each, the nulled matches, S12, Scw and the report.
//                     Pair j belongs to lane j mod kS3oTeam; the 15 estimates of a linearisation and their inverses are
//                     computed once, by 15 lanes, into LDS and read from there by every pair; the 36 sums take an xor
//                     butterfly per wavefront and an LDS pass over the wavefront sums; lane 0 runs the serial part (7x7
//                     LDLt, exp, composition, the LM state) over LDS.  The pair list lives in LDS, pair data is re-read
//                     from L2.  No float atomics, no scratch.
#include "orbhip_internal.h"
#include "orbhip_sim3opt_core.h"
#include "orbhip_team_dev.h"

namespace orbhip {
namespace {

struct S3oDevTeam : DevTeam<kS3oTeam> {
    template <bool FULL> __device__ __forceinline__ void sum(S3oWs &W, const S3oCand &F, double *s)
    {
        double est[8], einv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { est[k] = W.est[k]; einv[k] = W.einv[k]; }
#pragma unroll
        for (int k = 0; k < kS3oSums; ++k) s[k] = 0.0;
        const int ne = W.ne;
        for (int j = tid; j < ne; j += kS3oTeam) {
            if (F.e_out[j]) continue;
            S3oPair p;
            s3o_load_pair(F, j, p);
            if (FULL) {
                s3o_edge_terms(W.E, p.P2, p.o1, p.inv1, F.cam, F.delta, F.dsqr, s);
                s3o_edge_terms(W.Ei, p.P1, p.o2, p.inv2, F.cam, F.delta, F.dsqr, s);
            } else {
                s3o_pair_chi(p, est, einv, F.cam, F.delta, F.dsqr, s);
            }
        }
        team_combine<kS3oTeam, FULL ? 0 : kS3oSums - 1, kS3oSums>(s, W.part, tid);
    }
};

__global__ __launch_bounds__(kS3oTeam) void k_optimize_sim3(S3oArgs A)
{
    __shared__ S3oWs W;
    __shared__ uint16_t s_slot[kS3oCapMax];
    __shared__ uint16_t s_i2[kS3oCapMax];
    __shared__ int s_p2[kS3oCapMax];
    __shared__ uint8_t s_out[kS3oCapMax];
    __shared__ float s_inv[ORBHIP_MAX_LEVELS];
    __shared__ int s_w[kS3oTeam / kS3oWave];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (kS3oWave - 1), wv = tid / kS3oWave;
    int *report = A.report + (size_t)c * 8;
    if (A.select && !A.select[c]) {                                            // uniform over the workgroup
        if (tid == 0) report[0] = ORBHIP_SIM3OPT_SKIPPED;
        return;
    }
    const S3oTables &T = A.T;
    const int kf = A.kf_index[c], cur = T.cur;
    const bool kf_ok = (unsigned)kf < (unsigned)T.rows;
    const int n1 = min(max(T.n[cur], 0), T.cap);
    const size_t row = (size_t)c * T.cap, kfo = kf_ok ? (size_t)kf * T.cap : 0;
    S3oCand F;
    F.kps_cur = A.kps + (size_t)cur * T.cap;
    F.kps_kf = A.kps + kfo;
    F.sp_cur = T.slot_point + (size_t)cur * T.cap;
    F.world = A.world;
    F.T1 = A.Tcw + (size_t)cur * 12;
    F.T2 = A.Tcw + (kf_ok ? (size_t)kf * 12 : 0);
    F.inv_sigma2 = s_inv;
    F.sim3 = A.sim3 + (size_t)c * 16;
    F.matched = A.matched12 + row;
    F.S12 = A.S12 + (size_t)c * 8;
    F.Scw = A.Scw ? A.Scw + (size_t)c * 12 : nullptr;
    F.report = report;
    F.e_slot = s_slot; F.e_i2 = s_i2; F.e_p2 = s_p2; F.e_out = s_out;
    F.n_levels = min(max(A.n_levels, 1), ORBHIP_MAX_LEVELS); F.fix_scale = A.fix_scale;
    F.cam = A.cam; F.delta = A.delta; F.dsqr = A.delta * A.delta; F.th2 = A.th2;
    if (tid < ORBHIP_MAX_LEVELS) s_inv[tid] = A.inv[tid];
    // the kept slots i < n[cur], in slot order (:1099-1178)
    int running = 0;
    for (int b = 0; b < n1; b += kS3oTeam) {
        const int i = b + tid;
        int p2 = -1, i2 = -1;
        const bool keep = i < n1 && kf_ok && s3o_keep(T, kf, i, F.matched[i], p2, i2);
        const int incl = wave_incl_scan_add(keep ? 1 : 0);
        if (lane == kS3oWave - 1) s_w[wv] = incl;
        __syncthreads();
        int off = running, all = 0;
        for (int w = 0; w < kS3oTeam / kS3oWave; ++w) {
            if (w < wv) off += s_w[w];
            all += s_w[w];
        }
        if (keep) {
            const int k = off + incl - 1;
            s_slot[k] = (uint16_t)i; s_p2[k] = p2; s_i2[k] = (uint16_t)i2; s_out[k] = 0;
        }
        running += all;
        __syncthreads();
    }
    if (tid == 0) { W.ne = running; W.cnt[0] = 0; W.cnt[1] = 0; }
    __syncthreads();
    S3oDevTeam tm{tid};
    s3o_run(tm, W, F);
}

}  // namespace

int launch_optimize_sim3(hipStream_t stream, S3oArgs A)
{
    if (A.C <= 0) return ORBHIP_OK;
    hipLaunchKernelGGL(k_optimize_sim3, dim3(A.C), dim3(kS3oTeam), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
