// Host build of orbhip_gba_core.h: one thread replays what the kernels do, so its outputs must equal those of
// tests/seqref/gba.py bit for bit (tests/test_gba_cpu.py builds this with g++ -ffp-contract=off and runs it).
//   gba_host ba|apply <in> <out> [fill]   the optional trailing argument is the byte (0 .. 255, default 0) the workspace holds before the run
//   gba_host ba <in> <out>      in:  int32 header[24] = {rows, cap, np, pcap, n_levels, max_points, max_edges, has kf_bad,
//                                    has u_right, has stop, script length, has kf_list, nkf, has pt_list, npt, iterations, robust,
//                                    mode, 0...}, float cam[5] = fx, fy, cx, cy, bf, float inv_level_sigma2[n_levels], then
//                                    [kf_bad], kf_id, obs_start, obs_kf, obs_idx, flags, kps, [u_right], Tcw, world as the C ABI
//                                    lays them out, uint8 script[script length], kf_list [nkf], pt_list [npt], and the caller's
//                                    TcwGBA, posGBA, kf_mark, pt_mark, point_list [max_points], report [16]
//                               out: Tcw, world, TcwGBA, posGBA, kf_mark, pt_mark, point_list, report
//   gba_host apply <in> <out>   in:  int32 header[8] = {rows, pcap, n_origins, has kf_bad, 0...}, origins, parent, [kf_bad],
//                                    kf_mark, TcwGBA, Tcw, pt_mark, posGBA, flags, ref_kf, world, TcwBefGBA, report [8]
//                               out: kf_mark, TcwGBA, Tcw, world, TcwBefGBA, report
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip_gba_core.h"

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

template <class T> static void emit(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("write"); exit(2); }
}

static uint8_t *aligned(std::vector<uint8_t> &ws) { return ws.data() + (256 - (size_t)ws.data() % 256) % 256; }

static int run_ba(Cursor &c, FILE *out, uint8_t fill, bool state)
{
    const std::vector<int32_t> h = c.take<int32_t>(24);
    const int rows = h[0], cap = h[1], np = h[2], pcap = h[3], n_levels = h[4], max_points = h[5], max_edges = h[6];
    if (rows < 0 || rows > 4096 || cap < 1 || cap > 4096 || np < 0 || np > pcap || n_levels < 1 || n_levels > ORBHIP_MAX_LEVELS ||
        max_points < 1 || max_edges < 1 || h[10] < 0 || (h[9] && h[10] < 1) || h[12] < 0 || h[12] > rows || h[14] < 0 || h[14] > pcap ||
        h[15] < 1)
        return 2;
    const size_t R = rows, RC = R * cap, P = pcap;
    const std::vector<float> cam = c.take<float>(5), inv = c.take<float>(n_levels);
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(h[7] ? R : 0);
    const std::vector<int32_t> kf_id = c.take<int32_t>(R), obs_start = c.take<int32_t>((size_t)np + 1);
    const size_t total = (size_t)obs_start[np];
    const std::vector<int32_t> obs_kf = c.take<int32_t>(total), obs_idx = c.take<int32_t>(total);
    const std::vector<uint8_t> flags = c.take<uint8_t>(P);
    const std::vector<orbhip_keypoint> kps = c.take<orbhip_keypoint>(RC);
    const std::vector<float> u_right = c.take<float>(h[8] ? RC : 0);
    std::vector<float> Tcw = c.take<float>(R * 12), world = c.take<float>(P * 3);
    const std::vector<uint8_t> script = c.take<uint8_t>((size_t)h[10]);
    const std::vector<int32_t> kf_list = c.take<int32_t>(h[11] ? (size_t)h[12] : 0), pt_list = c.take<int32_t>(h[13] ? (size_t)h[14] : 0);
    std::vector<float> TcwGBA = c.take<float>(R * 12), posGBA = c.take<float>(P * 3);
    std::vector<uint8_t> kf_mark = c.take<uint8_t>(R), pt_mark = c.take<uint8_t>(P);
    std::vector<int32_t> point_list = c.take<int32_t>((size_t)max_points), report = c.take<int32_t>(16);
    const int32_t none = 0;

    GbaWs G;
    memset(&G, 0, sizeof(G));
    LbaWs &W = G.L;
    W.kf_bad = h[7] ? kf_bad.data() : nullptr; W.obs_start = obs_start.data(); W.obs_kf = obs_kf.data(); W.obs_idx = obs_idx.data();
    W.flags = flags.data(); W.kps = kps.data(); W.u_right = h[8] ? u_right.data() : nullptr; W.Tcw = Tcw.data(); W.world = world.data();
    W.stop = h[9] ? script.data() : nullptr; W.script = h[9] ? script.data() : nullptr; W.script_n = h[10];
    for (int l = 0; l < ORBHIP_MAX_LEVELS; ++l) W.inv[l] = l < n_levels ? inv[l] : 0.f;
    W.cam.fx = (double)cam[0]; W.cam.fy = (double)cam[1]; W.cam.cx = (double)cam[2]; W.cam.cy = (double)cam[3]; W.cam.bf = (double)cam[4];
    W.cam.delta_mono = (double)(float)std::sqrt(5.99);
    W.cam.delta_stereo = (double)(float)std::sqrt(7.815);
    W.id0_row = -1; W.rows = rows; W.cap = cap; W.np = np; W.pcap = pcap; W.n_levels = n_levels; W.max_points = max_points; W.max_edges = max_edges;
    W.single_its = h[15]; W.robust = h[16] ? 1 : 0;
    G.kf_id = kf_id.data();
    G.kf_list = h[11] ? (kf_list.empty() ? &none : kf_list.data()) : nullptr; G.nkf = h[12];
    G.pt_list = h[13] ? (pt_list.empty() ? &none : pt_list.data()) : nullptr; G.npt = h[14];
    G.mode = h[17];
    G.TcwGBA = TcwGBA.data(); G.posGBA = posGBA.data(); G.kf_mark = kf_mark.data(); G.pt_mark = pt_mark.data();
    G.o_point_list = point_list.data(); G.o_report = report.data();
    std::vector<uint8_t> ws(gba_carve(G, nullptr) + 256, fill);
    gba_carve(G, aligned(ws));
    gba_host_run(G);
    emit(out, Tcw); emit(out, world); emit(out, TcwGBA); emit(out, posGBA); emit(out, kf_mark); emit(out, pt_mark); emit(out, point_list);
    emit(out, report);
    if (state) emit(out, std::vector<double>{W.S->lam, W.S->rho, W.S->current});   // where the last trial left Levenberg-Marquardt
    return 0;
}

static int run_apply(Cursor &c, FILE *out, uint8_t fill)
{
    const std::vector<int32_t> h = c.take<int32_t>(8);
    const int rows = h[0], pcap = h[1], n_origins = h[2];
    if (rows < 1 || rows > 4096 || pcap < 0 || n_origins < 0) return 2;
    const size_t R = rows, P = pcap;
    const std::vector<int32_t> origins = c.take<int32_t>((size_t)n_origins), parent = c.take<int32_t>(R);
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(h[3] ? R : 0);
    std::vector<uint8_t> kf_mark = c.take<uint8_t>(R);
    std::vector<float> TcwGBA = c.take<float>(R * 12), Tcw = c.take<float>(R * 12);
    const std::vector<uint8_t> pt_mark = c.take<uint8_t>(P);
    const std::vector<float> posGBA = c.take<float>(P * 3);
    const std::vector<uint8_t> flags = c.take<uint8_t>(P);
    const std::vector<int32_t> ref_kf = c.take<int32_t>(P);
    std::vector<float> world = c.take<float>(P * 3), bef = c.take<float>(R * 12);
    std::vector<int32_t> report = c.take<int32_t>(8);
    GbaApply A;
    memset(&A, 0, sizeof(A));
    A.origins = origins.data(); A.parent = parent.data(); A.kf_bad = h[3] ? kf_bad.data() : nullptr; A.kf_mark = kf_mark.data();
    A.TcwGBA = TcwGBA.data(); A.Tcw = Tcw.data(); A.TcwBef = bef.data(); A.pt_mark = pt_mark.data(); A.flags = flags.data();
    A.posGBA = posGBA.data(); A.ref_kf = ref_kf.data(); A.world = world.data(); A.o_report = report.data();
    A.n_origins = n_origins; A.rows = rows; A.pcap = pcap;
    std::vector<uint8_t> ws(gba_apply_carve(A, nullptr) + 256, fill);
    gba_apply_carve(A, aligned(ws));
    gba_apply_host(A);
    emit(out, kf_mark); emit(out, TcwGBA); emit(out, Tcw); emit(out, world); emit(out, bef); emit(out, report);
    return 0;
}

int main(int argc, char **argv)
{
    if ((argc < 4 || argc > 6) || (strcmp(argv[1], "ba") && strcmp(argv[1], "apply"))) {
        fprintf(stderr, "usage: gba_host ba|apply <in> <out> [fill [state]]\n");
        return 2;
    }
    const uint8_t fill = argc >= 5 ? (uint8_t)strtol(argv[4], nullptr, 0) : 0;
    std::vector<unsigned char> in = slurp(argv[2]);
    Cursor c{in, 0};
    FILE *out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 2; }
    const int rc = strcmp(argv[1], "ba") ? run_apply(c, out, fill) : run_ba(c, out, fill, argc == 6 && !strcmp(argv[5], "state"));
    fclose(out);
    return rc;
}
