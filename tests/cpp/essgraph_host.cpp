// Host build of orbhip_essgraph_core.h: one thread replays what the kernels do, so its outputs must equal those of
// tests/seqref/essgraph.py bit for bit (tests/test_essgraph_cpu.py builds this with g++ -ffp-contract=off and runs it, also
// under -fsanitize=address,undefined).
//   essgraph_host <in> <out> [fill]   the optional trailing argument is the byte (0 .. 255, default 0) the workspace holds before the run
//                              in:   int32 header[16] = {rows, pcap, cur, loop_row, fix_scale, max_edges, entries of loop_kf,
//                                   entries of lc_kf, max trials to dump, 0 ...}, then kf_bad, kf_id, parent, conn_w, ord_kf,
//                                   ord_w, n_ord, loop_start, loop_kf, lc_start, lc_kf, corrected, non_corrected,
//                                   in_corrected, in_non_corrected, flags, ref_kf, corrected_by_kf, corrected_ref, Tcw, world
//                                   as the C ABI lays them out, and the caller's point_list, Scw_out, Swc_out, report
//                              out: Tcw, world, point_list, Scw_out, Swc_out, report, int32 trials dumped, and per trial the
//                                   tried estimate of every vertex in row order, [8] doubles each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip.h"
#include "orbhip_essgraph_core.h"

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
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: essgraph_host <in> <out> [fill]\n"); return 2; }
    const uint8_t fill = argc == 4 ? (uint8_t)strtol(argv[3], nullptr, 0) : 0;
    std::vector<unsigned char> in = slurp(argv[1]);
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(16);
    const int rows = h[0], pcap = h[1], max_edges = h[5], n_loop = h[6], n_lc = h[7], max_trials = h[8];
    if (rows < 1 || rows > 4096 || pcap < 0 || max_edges < 1 || n_loop < 0 || n_lc < 0 || max_trials < 0 || h[2] < 0 || h[2] >= rows ||
        h[3] < 0 || h[3] >= rows)
        return 2;
    const size_t R = rows, P = pcap;
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(R);
    const std::vector<int32_t> kf_id = c.take<int32_t>(R), parent = c.take<int32_t>(R), conn_w = c.take<int32_t>(R * R);
    const std::vector<int32_t> ord_kf = c.take<int32_t>(R * R), ord_w = c.take<int32_t>(R * R), n_ord = c.take<int32_t>(R);
    const std::vector<int32_t> loop_start = c.take<int32_t>(R + 1), loop_kf = c.take<int32_t>((size_t)n_loop);
    const std::vector<int32_t> lc_start = c.take<int32_t>(R + 1), lc_kf = c.take<int32_t>((size_t)n_lc);
    const std::vector<double> corrected = c.take<double>(R * 8), non_corrected = c.take<double>(R * 8);
    const std::vector<uint8_t> in_c = c.take<uint8_t>(R), in_nc = c.take<uint8_t>(R), flags = c.take<uint8_t>(P);
    const std::vector<int32_t> ref_kf = c.take<int32_t>(P), cby = c.take<int32_t>(P), cref = c.take<int32_t>(P);
    std::vector<float> Tcw = c.take<float>(R * 12), world = c.take<float>(P * 3);
    std::vector<int32_t> point_list = c.take<int32_t>(P);
    std::vector<double> Scw = c.take<double>(R * 8), Swc = c.take<double>(R * 8);
    std::vector<int32_t> report = c.take<int32_t>(16);
    if (loop_start[rows] != n_loop || lc_start[rows] != n_lc) return 2;

    EgWs W;
    memset(&W, 0, sizeof(W));
    W.kf_bad = kf_bad.data(); W.kf_id = kf_id.data(); W.parent = parent.data(); W.conn_w = conn_w.data(); W.ord_kf = ord_kf.data();
    W.ord_w = ord_w.data(); W.n_ord = n_ord.data(); W.loop_start = loop_start.data(); W.loop_kf = loop_kf.data();
    W.lc_start = lc_start.data(); W.lc_kf = lc_kf.data(); W.corrected = corrected.data(); W.non_corrected = non_corrected.data();
    W.in_c = in_c.data(); W.in_nc = in_nc.data(); W.flags = flags.data(); W.ref_kf = ref_kf.data(); W.cby = cby.data();
    W.cref = cref.data(); W.Tcw = Tcw.data(); W.world = world.data(); W.o_point_list = point_list.data();
    W.o_Scw = Scw.data(); W.o_Swc = Swc.data(); W.o_report = report.data();
    W.rows = rows; W.pcap = pcap; W.cur = h[2]; W.loop_row = h[3]; W.fix_scale = h[4]; W.max_edges = max_edges;
    std::vector<uint8_t> ws(eg_carve(W, nullptr) + 256, fill);
    eg_carve(W, ws.data() + (256 - (size_t)ws.data() % 256) % 256);
    std::vector<double> tried((size_t)max_trials * eg_mk(W) * 8 + 1, 0.0);
    EgHostTrace trace;
    trace.tried = tried.data(); trace.max_trials = max_trials; trace.n_trials = 0;
    eg_host_run(W, &trace);

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    emit(out, Tcw.data(), Tcw.size()); emit(out, world.data(), world.size()); emit(out, point_list.data(), point_list.size());
    emit(out, Scw.data(), Scw.size()); emit(out, Swc.data(), Swc.size()); emit(out, report.data(), report.size());
    const int32_t nt = trace.n_trials, nv = W.S->status == ORBHIP_EG_CAPACITY ? 0 : W.S->nv;
    emit(out, &nt, 1);
    for (int t = 0; t < nt; ++t) emit(out, tried.data() + (size_t)t * eg_mk(W) * 8, (size_t)nv * 8);
    fclose(out);
    return 0;
}
