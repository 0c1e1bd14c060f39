// Host build of orbhip_poseopt_core.h: one thread replays what a device team does, so its outputs must equal those of
// tests/seqref/poseopt.py bit for bit (tests/test_poseopt_cpu.py builds this with g++ -ffp-contract=off and runs it).
//   poseopt_host run|classify <in> <out> [fill]   the optional trailing argument is the byte (0 .. 255, default 0) the workspace holds before the run: the team's record PoWs (its two
//                                    emitted estimates start at zero all the same) and the edge lists e_slot, e_pt, e_out
//   poseopt_host run <in> <out>      in:  int32 header {frames, cap, wrows, pcap, has u_right, has world_row, has point_flags,
//                                         has discarded, n_levels, mode, flags}, float cam[5] = fx, fy, cx, cy, bf,
//                                         float inv_level_sigma2[n_levels], then kps, n, [u_right], world, [point_flags],
//                                         [world_row], Tcw, frame_point, outlier, [discarded] as the C ABI lays them out
//                                    out: Tcw, frame_point, outlier, [discarded], report, then the estimate and the last
//                                         tried estimate of the last frame's last round as 2 x 7 doubles (quaternion x y z w, t)
//   poseopt_host classify <in> <out> in:  as for run, followed by double est[7], tried[7] and uint8 e_out[cap]: the
//                                         classification after a round (po_classify) of frame 0 with that state
//                                    out: uint8 e_out[cap], int32 flagged, int32 edges
//   poseopt_host sincos <in> <out>   in: doubles; out: (sin, cos) pairs of det_sincos64
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip_poseopt_core.h"

using namespace orbhip;

static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

struct Cursor {
    std::vector<unsigned char> &v;
    size_t off;
    // a copy: the arrays follow each other without padding, so they are not aligned inside the file
    template <class T> std::vector<T> take(size_t count)
    {
        const size_t bytes = count * sizeof(T);
        if (off + bytes > v.size()) { fprintf(stderr, "input too short\n"); exit(2); }
        std::vector<T> r(count);
        if (bytes) memcpy(r.data(), v.data() + off, bytes);
        off += bytes;
        return r;
    }
};

template <class T> static void emit(FILE *f, const T *p, size_t count)
{
    if (fwrite(p, sizeof(T), count, f) != count) { perror("write"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc != 4 && argc != 5) { fprintf(stderr, "usage: poseopt_host run|classify|sincos <in> <out> [fill]\n"); return 2; }
    const uint8_t fill = argc == 5 ? (uint8_t)strtol(argv[4], nullptr, 0) : 0;
    std::vector<unsigned char> in = slurp(argv[2]);
    FILE *out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 2; }
    if (argv[1][0] == 's') {
        const size_t cnt = in.size() / sizeof(double);
        const double *x = reinterpret_cast<const double *>(in.data());
        std::vector<double> r(2 * cnt);
        for (size_t i = 0; i < cnt; ++i) det_sincos64(x[i], r[2 * i], r[2 * i + 1]);
        emit(out, r.data(), r.size());
        fclose(out);
        return 0;
    }
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(11);
    const int frames = h[0], cap = h[1], wrows = h[2], pcap = h[3], n_levels = h[8], mode = h[9], flags = h[10];
    if (frames < 0 || cap < 1 || cap > 4096 || wrows < 1 || pcap < 1 || n_levels < 1 || n_levels > ORBHIP_MAX_LEVELS) return 2;
    const std::vector<float> cam = c.take<float>(5), inv = c.take<float>(n_levels);
    const size_t Fn = frames, FC = Fn * cap, WP = (size_t)wrows * pcap;
    const std::vector<orbhip_keypoint> kps_v = c.take<orbhip_keypoint>(FC);
    const std::vector<int32_t> n = c.take<int32_t>(Fn);
    const std::vector<float> ur_v = c.take<float>(h[4] ? FC : 0), world = c.take<float>(WP * 3);
    const std::vector<uint8_t> pf_v = c.take<uint8_t>(h[6] ? WP : 0);
    const std::vector<int32_t> row_v = c.take<int32_t>(h[5] ? Fn : 0);
    std::vector<float> Tcw = c.take<float>(Fn * 12);
    std::vector<int32_t> fp = c.take<int32_t>(FC);
    std::vector<uint8_t> outl = c.take<uint8_t>(FC);
    std::vector<int32_t> dis_v = c.take<int32_t>(h[7] ? FC : 0);
    const bool classify = argv[1][0] == 'c';
    const std::vector<double> poses = c.take<double>(classify ? 14 : 0);
    const std::vector<uint8_t> flags_in = c.take<uint8_t>(classify ? (size_t)cap : 0);
    const orbhip_keypoint *kps = kps_v.data();
    const float *ur = h[4] ? ur_v.data() : nullptr;
    const uint8_t *pf = h[6] ? pf_v.data() : nullptr;
    const int32_t *row = h[5] ? row_v.data() : nullptr;
    int32_t *dis = h[7] ? dis_v.data() : nullptr;
    std::vector<int32_t> report(Fn * 8, 0);
    std::vector<uint16_t> e_slot(cap);
    std::vector<int> e_pt(cap);
    std::vector<uint8_t> e_out(cap, fill);
    memset(e_slot.data(), fill, e_slot.size() * sizeof(uint16_t));
    memset(e_pt.data(), fill, e_pt.size() * sizeof(int));
    static PoWs W;
    memset(&W, fill, sizeof(W));
    for (int k = 0; k < 7; ++k) W.est[k] = W.tried[k] = 0.0;
    for (int f = 0; f < frames; ++f) {
        const int r = row ? row[f] : 0;
        if (r < 0 || r >= wrows || n[f] < 0 || n[f] > cap) return 2;
        PoFrame F;
        F.kps = kps + (size_t)f * cap;
        F.u_right = ur ? ur + (size_t)f * cap : nullptr;
        F.world = world.data() + (size_t)r * pcap * 3;
        F.pflags = pf ? pf + (size_t)r * pcap : nullptr;
        F.inv_sigma2 = inv.data();
        F.Tcw = Tcw.data() + (size_t)f * 12;
        F.frame_point = fp.data() + (size_t)f * cap;
        F.outlier = outl.data() + (size_t)f * cap;
        F.discarded = dis ? dis + (size_t)f * cap : nullptr;
        F.report = report.data() + (size_t)f * 8;
        F.e_slot = e_slot.data(); F.e_pt = e_pt.data(); F.e_out = e_out.data();
        F.n = n[f]; F.pcap = pcap; F.n_levels = n_levels; F.mode = mode; F.flags = flags;
        F.cam.fx = (double)cam[0]; F.cam.fy = (double)cam[1]; F.cam.cx = (double)cam[2]; F.cam.cy = (double)cam[3];
        F.cam.bf = (double)cam[4];
        F.cam.delta_mono = (double)(float)std::sqrt(5.991);
        F.cam.delta_stereo = (double)(float)std::sqrt(7.815);
        po_host_compact(W, F);
        PoHostTeam tm;
        if (classify) {
            for (int k = 0; k < 7; ++k) { W.est[k] = poses[k]; W.tried[k] = poses[7 + k]; }
            for (int j = 0; j < W.ne; ++j) e_out[j] = flags_in[j];
            const int32_t counts[2] = {po_classify(tm, W, F, W.ne), W.ne};
            emit(out, e_out.data(), (size_t)cap);
            emit(out, counts, 2);
            fclose(out);
            return 0;
        }
        po_run(tm, W, F);
    }
    emit(out, Tcw.data(), Fn * 12);
    emit(out, fp.data(), FC);
    emit(out, outl.data(), FC);
    if (dis) emit(out, dis, FC);
    emit(out, report.data(), report.size());
    emit(out, W.est, 7);
    emit(out, W.tried, 7);
    fclose(out);
    return 0;
}
