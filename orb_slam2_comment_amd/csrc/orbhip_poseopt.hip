// Pose optimisation on the device: Optimizer::PoseOptimization (src/Optimizer.cc:239-451) and the loops of Tracking that
// follow it (include/orbhip.h, section "pose optimisation").  gfx950 only, wave64.  The arithmetic is
// tests/seqref/poseopt.py operation by operation; the function itself is orbhip_poseopt_core.h,
// which the host can replay bit for bit.
//
// One launch on the caller's stream:
//   k_pose_optimization   one workgroup of kPoTeam lanes per frame: the slots with a point compacted in slot order (scan per
//                         wavefront, wavefront totals through LDS), four rounds of Levenberg-Marquardt, the classification
//                         after each, mvbOutlier, the epilogue of the mode and the report.  Edge j belongs to lane
//                         j mod kPoTeam; the 28 sums take an xor butterfly per wavefront and an LDS pass over the four
//                         wavefront sums; lane 0 runs the serial part (6x6 LDLt, exp, composition, the LM state) over LDS.
//                         The edge list lives in LDS, edge data is re-read from L2.  No float atomics, no scratch.
#include "orbhip_internal.h"
#include "orbhip_poseopt_core.h"
#include "orbhip_team_dev.h"

namespace orbhip {
namespace {

struct PoDevTeam : DevTeam<kPoTeam> {
    template <bool FULL> __device__ __forceinline__ void sum(PoWs &W, const PoFrame &F, bool kernel, double *s)
    {
        double pose[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) pose[k] = W.est[k];
#pragma unroll
        for (int k = 0; k < 28; ++k) s[k] = 0.0;
        const int ne = W.ne;
        for (int j = tid; j < ne; j += kPoTeam) {
            if (F.e_out[j]) continue;
            PoEdge e;
            po_load_edge(F, j, e);
            po_edge_terms<FULL>(e, pose, F.cam, kernel, s);
        }
        team_combine<kPoTeam, FULL ? 0 : 27, 28>(s, W.part, tid);
    }
};

__global__ __launch_bounds__(kPoTeam) void k_pose_optimization(PoArgs A)
{
    __shared__ PoWs W;
    __shared__ uint16_t s_slot[kPoCapMax];
    __shared__ int s_pt[kPoCapMax];
    __shared__ uint8_t s_out[kPoCapMax];
    __shared__ float s_inv[ORBHIP_MAX_LEVELS];
    __shared__ int s_w[kPoTeam / kPoWave];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (kPoWave - 1), wv = tid / kPoWave;
    const int n = min(max(A.n[f], 0), A.cap);
    const int row = A.world_row ? A.world_row[f] : 0;
    const bool row_ok = (unsigned)row < (unsigned)A.wrows;
    const size_t fo = (size_t)f * A.cap, ro = row_ok ? (size_t)row * A.pcap : 0;
    PoFrame F;
    F.kps = A.kps + fo;
    F.u_right = A.u_right ? A.u_right + fo : nullptr;
    F.world = A.world + ro * 3;
    F.pflags = A.point_flags ? A.point_flags + ro : nullptr;
    F.inv_sigma2 = s_inv;
    F.Tcw = A.Tcw + (size_t)f * 12;
    F.frame_point = A.frame_point + fo;
    F.outlier = A.outlier + fo;
    F.discarded = A.discarded ? A.discarded + fo : nullptr;
    F.report = A.report + (size_t)f * 8;
    F.e_slot = s_slot; F.e_pt = s_pt; F.e_out = s_out;
    F.n = n; F.pcap = A.pcap; F.n_levels = min(max(A.n_levels, 1), ORBHIP_MAX_LEVELS); F.mode = A.mode; F.flags = A.flags;
    F.cam = A.cam;
    if (tid < ORBHIP_MAX_LEVELS) s_inv[tid] = A.inv[tid];
    // the slots i < n with a point, in slot order (:280-360)
    int running = 0;
    for (int b = 0; b < n; b += kPoTeam) {
        const int i = b + tid;
        int p = -1;
        if (i < n) {
            p = F.frame_point[i];
        }
        const bool keep = row_ok && (unsigned)p < (unsigned)A.pcap;
        // a slot without an edge is written here, a slot with one by the lane that owns the edge, once
        if (i < n && !keep && A.mode != ORBHIP_POSEOPT_PLAIN && F.discarded) F.discarded[i] = -1;
        const int incl = wave_incl_scan_add(keep ? 1 : 0);
        if (lane == kPoWave - 1) s_w[wv] = incl;
        __syncthreads();
        int off = running, all = 0;
        for (int w = 0; w < kPoTeam / kPoWave; ++w) {
            if (w < wv) off += s_w[w];
            all += s_w[w];
        }
        if (keep) {
            const int k = off + incl - 1;
            s_slot[k] = (uint16_t)i; s_pt[k] = p; s_out[k] = 0;               // :289, :323: the byte is written at the end
        }
        running += all;
        __syncthreads();
    }
    if (tid == 0) { W.ne = running; W.cnt[0] = 0; W.cnt[1] = 0; W.cnt[2] = 0; }
    __syncthreads();
    PoDevTeam tm{tid};
    po_run(tm, W, F);
}

}  // namespace

int launch_pose_optimization(hipStream_t stream, PoArgs A)
{
    if (A.frames <= 0) return ORBHIP_OK;
    hipLaunchKernelGGL(k_pose_optimization, dim3(A.frames), dim3(kPoTeam), 0, stream, A);
    ORBHIP_HIP_CHECK(hipGetLastError());
    return ORBHIP_OK;
}

}  // namespace orbhip
