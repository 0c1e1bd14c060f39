// Host build of orbhip_lba_core.h: one thread replays what the phase kernels do, so its outputs must equal those of
// tests/seqref/lba.py bit for bit (tests/test_lba_cpu.py builds this with g++ -ffp-contract=off and runs it).
//   lba_host <in> <out> [fill]   the optional trailing argument is the byte (0 .. 255, default 0) the workspace holds before the run
//                         in:   int32 header[16] = {cur, id0_row, rows, cap, np, pcap, n_levels, max_points, max_edges,
//                              has kf_bad, has u_right, has stop, script length, 0, 0, 0}, float cam[5] = fx, fy, cx, cy, bf,
//                              float inv_level_sigma2[n_levels], then slot_point, n, [kf_bad], obs_start, obs_kf, obs_idx,
//                              flags, kps, [u_right], ord_kf, n_ord, Tcw, world as the C ABI lays them out, uint8
//                              script[script length] (the values successive samples of the stop byte return, the last one
//                              repeats), and the caller's local_kf, fixed_kf, local_point, erase, report
//                         out: Tcw, world, local_kf, fixed_kf, local_point, erase, report, then for round 1 and round 2 the
//                              estimate and the last tried estimate when the round ended, each [rows][7] + [max_points][3]
//                              doubles (vertices in list order, local then fixed; points in list order; zero beyond)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip_lba_core.h"

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
    if (count && fwrite(p, sizeof(T), count, f) != count) { perror("write"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: lba_host <in> <out> [fill]\n"); return 2; }
    const uint8_t fill = argc == 4 ? (uint8_t)strtol(argv[3], nullptr, 0) : 0;
    std::vector<unsigned char> in = slurp(argv[1]);
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(16);
    const int rows = h[2], cap = h[3], np = h[4], pcap = h[5], n_levels = h[6], max_points = h[7], max_edges = h[8];
    if (rows < 1 || rows > 4096 || cap < 1 || cap > 4096 || np < 0 || np > pcap || n_levels < 1 || n_levels > ORBHIP_MAX_LEVELS ||
        max_points < 1 || max_edges < 1 || h[0] < 0 || h[0] >= rows || h[1] < -1 || h[1] >= rows || h[12] < 0 || (h[11] && h[12] < 1))
        return 2;
    const size_t R = rows, RC = R * cap, P = pcap;
    const std::vector<float> cam = c.take<float>(5), inv = c.take<float>(n_levels);
    const std::vector<int32_t> slot_point = c.take<int32_t>(RC), n = c.take<int32_t>(R);
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(h[9] ? R : 0);
    const std::vector<int32_t> obs_start = c.take<int32_t>((size_t)np + 1);
    const size_t total = (size_t)obs_start[np];
    const std::vector<int32_t> obs_kf = c.take<int32_t>(total), obs_idx = c.take<int32_t>(total);
    const std::vector<uint8_t> flags = c.take<uint8_t>(P);
    const std::vector<orbhip_keypoint> kps = c.take<orbhip_keypoint>(RC);
    const std::vector<float> u_right = c.take<float>(h[10] ? RC : 0);
    const std::vector<int32_t> ord_kf = c.take<int32_t>(R * R), n_ord = c.take<int32_t>(R);
    std::vector<float> Tcw = c.take<float>(R * 12), world = c.take<float>(P * 3);
    const std::vector<uint8_t> script = c.take<uint8_t>((size_t)h[12]);
    std::vector<int32_t> local_kf = c.take<int32_t>(R), fixed_kf = c.take<int32_t>(R), local_point = c.take<int32_t>((size_t)max_points);
    std::vector<int32_t> erase = c.take<int32_t>((size_t)max_edges * 3), report = c.take<int32_t>(16);

    LbaWs W;
    memset(&W, 0, sizeof(W));
    W.slot_point = slot_point.data(); W.n = n.data(); W.kf_bad = h[9] ? kf_bad.data() : nullptr;
    W.obs_start = obs_start.data(); W.obs_kf = obs_kf.data(); W.obs_idx = obs_idx.data(); W.flags = flags.data();
    W.kps = kps.data(); W.u_right = h[10] ? u_right.data() : nullptr; W.ord_kf = ord_kf.data(); W.n_ord = n_ord.data();
    W.Tcw = Tcw.data(); W.world = world.data();
    W.o_local_kf = local_kf.data(); W.o_fixed_kf = fixed_kf.data(); W.o_local_point = local_point.data();
    W.o_erase = erase.data(); W.o_report = report.data();
    W.stop = h[11] ? script.data() : nullptr; W.script = h[11] ? script.data() : nullptr; W.script_n = h[12];
    for (int l = 0; l < ORBHIP_MAX_LEVELS; ++l) W.inv[l] = l < n_levels ? inv[l] : 0.f;
    W.cam.fx = (double)cam[0]; W.cam.fy = (double)cam[1]; W.cam.cx = (double)cam[2]; W.cam.cy = (double)cam[3]; W.cam.bf = (double)cam[4];
    W.cam.delta_mono = (double)(float)std::sqrt(5.991);
    W.cam.delta_stereo = (double)(float)std::sqrt(7.815);
    W.cur = h[0]; W.id0_row = h[1]; W.rows = rows; W.cap = cap; W.np = np; W.pcap = pcap; W.n_levels = n_levels;
    W.max_points = max_points; W.max_edges = max_edges;
    std::vector<uint8_t> ws(lba_carve(W, nullptr) + 256, fill);
    lba_carve(W, ws.data() + (256 - (size_t)ws.data() % 256) % 256);
    const size_t snap = R * 7 + (size_t)max_points * 3;
    std::vector<double> tr(4 * snap, 0.0);
    LbaHostTrace trace;
    trace.est[0] = tr.data(); trace.tried[0] = tr.data() + snap; trace.est[1] = tr.data() + 2 * snap; trace.tried[1] = tr.data() + 3 * snap;
    lba_host_run(W, &trace);

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    emit(out, Tcw.data(), Tcw.size()); emit(out, world.data(), world.size());
    emit(out, local_kf.data(), local_kf.size()); emit(out, fixed_kf.data(), fixed_kf.size());
    emit(out, local_point.data(), local_point.size()); emit(out, erase.data(), erase.size()); emit(out, report.data(), report.size());
    emit(out, tr.data(), tr.size());
    fclose(out);
    return 0;
}
