// orbhip::Optimizer::OptimizeEssentialGraph and OptimizeEssentialGraphDevice (include/orbhip/Optimizer.hpp) on one case of
// tests/test_essgraph_cpu.py.  Built with g++ against liborbhip.so and the HIP runtime (device memory for the device form).
//   essgraph_smoke <in> <out>   in:  the input of tests/cpp/essgraph_host.cpp
//                               out: host mirror: int32 status, report[16], Tcw, world, the corrected points as int32 length +
//                                    entries, vScw and vCorrectedSwc [rows][8]; device form: Tcw, world, point_list [pcap],
//                                    Scw, Swc [rows][8], report [16] as the call left the caller's arrays
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip/Optimizer.hpp"

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

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); return 3; } } while (0)

template <class T> static int upload(const std::vector<T> &v, void **d)
{
    *d = nullptr;
    HIP_OK(hipMalloc(d, v.size() * sizeof(T) + 16));
    if (!v.empty()) HIP_OK(hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
template <class T> static int download(std::vector<T> &v, const void *d)
{
    if (!v.empty()) HIP_OK(hipMemcpy(v.data(), d, v.size() * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

static std::vector<double> flat(const std::vector<orbhip::Sim3> &v)
{
    std::vector<double> o;
    for (size_t r = 0; r < v.size(); ++r) {
        for (int i = 0; i < 4; ++i) o.push_back(v[r].r[i]);
        for (int i = 0; i < 3; ++i) o.push_back(v[r].t[i]);
        o.push_back(v[r].s);
    }
    return o;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: essgraph_smoke <in> <out>\n"); return 2; }
    std::vector<unsigned char> in = slurp(argv[1]);
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(16);
    const int rows = h[0], pcap = h[1], cur = h[2], loop_row = h[3], fix_scale = h[4], max_edges = h[5];
    const size_t R = rows, P = pcap;
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(R);
    const std::vector<int32_t> kf_id = c.take<int32_t>(R), parent = c.take<int32_t>(R), conn_w = c.take<int32_t>(R * R);
    const std::vector<int32_t> ord_kf = c.take<int32_t>(R * R), ord_w = c.take<int32_t>(R * R), n_ord = c.take<int32_t>(R);
    const std::vector<int32_t> loop_start = c.take<int32_t>(R + 1);
    std::vector<int32_t> loop_kf = c.take<int32_t>((size_t)h[6]);
    const std::vector<int32_t> lc_start = c.take<int32_t>(R + 1);
    std::vector<int32_t> lc_kf = c.take<int32_t>((size_t)h[7]);
    const std::vector<double> corrected = c.take<double>(R * 8), non_corrected = c.take<double>(R * 8);
    const std::vector<uint8_t> in_c = c.take<uint8_t>(R), in_nc = c.take<uint8_t>(R), flags = c.take<uint8_t>(P);
    const std::vector<int32_t> ref_kf = c.take<int32_t>(P), cby = c.take<int32_t>(P), cref = c.take<int32_t>(P);
    const std::vector<float> Tcw0 = c.take<float>(R * 12), world0 = c.take<float>(P * 3);
    std::vector<int32_t> point_list = c.take<int32_t>(P);
    std::vector<double> Scw = c.take<double>(R * 8), Swc = c.take<double>(R * 8);
    std::vector<int32_t> report = c.take<int32_t>(16);
    if (loop_kf.empty()) loop_kf.push_back(0);
    if (lc_kf.empty()) lc_kf.push_back(0);

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        // the host mirror
        std::vector<float> Tcw(Tcw0), world(world0);
        orbhip_eg_tables t;
        t.kf_bad = kf_bad.data(); t.kf_id = kf_id.data(); t.parent = parent.data(); t.conn_w = conn_w.data(); t.ord_kf = ord_kf.data();
        t.ord_w = ord_w.data(); t.n_ord = n_ord.data(); t.loop_start = loop_start.data(); t.loop_kf = loop_kf.data();
        t.lc_start = lc_start.data(); t.lc_kf = lc_kf.data(); t.corrected = corrected.data(); t.non_corrected = non_corrected.data();
        t.in_corrected = in_c.data(); t.in_non_corrected = in_nc.data(); t.flags = flags.data(); t.ref_kf = ref_kf.data();
        t.corrected_by_kf = cby.data(); t.corrected_ref = cref.data(); t.Tcw = Tcw.data(); t.world = world.data();
        orbhip::EssentialGraph eg;
        const int status = orbhip::Optimizer::OptimizeEssentialGraph(matcher, rows, pcap, t, loop_row, cur, fix_scale != 0, max_edges, eg);
        emit(out, std::vector<int32_t>(1, status));
        emit(out, std::vector<int32_t>(eg.report, eg.report + 16));
        emit(out, Tcw); emit(out, world);
        emit(out, std::vector<int32_t>(1, (int32_t)eg.vpCorrectedPoints.size()));
        emit(out, eg.vpCorrectedPoints);
        emit(out, flat(eg.vScw)); emit(out, flat(eg.vCorrectedSwc));
        printf("status %d vertices %d edges %d points %zu\n", status, eg.report[1], eg.report[2] + eg.report[3] + eg.report[4] + eg.report[5],
               eg.vpCorrectedPoints.size());
        // the device form
        void *d[25];
        if (upload(kf_bad, &d[0]) || upload(kf_id, &d[1]) || upload(parent, &d[2]) || upload(conn_w, &d[3]) || upload(ord_kf, &d[4]) ||
            upload(ord_w, &d[5]) || upload(n_ord, &d[6]) || upload(loop_start, &d[7]) || upload(loop_kf, &d[8]) || upload(lc_start, &d[9]) ||
            upload(lc_kf, &d[10]) || upload(corrected, &d[11]) || upload(non_corrected, &d[12]) || upload(in_c, &d[13]) ||
            upload(in_nc, &d[14]) || upload(flags, &d[15]) || upload(ref_kf, &d[16]) || upload(cby, &d[17]) || upload(cref, &d[18]) ||
            upload(Tcw0, &d[19]) || upload(world0, &d[20]) || upload(point_list, &d[21]) || upload(Scw, &d[22]) || upload(Swc, &d[23]) ||
            upload(report, &d[24]))
            return 3;
        orbhip_eg_tables dt;
        dt.kf_bad = d[0]; dt.kf_id = d[1]; dt.parent = d[2]; dt.conn_w = d[3]; dt.ord_kf = d[4]; dt.ord_w = d[5]; dt.n_ord = d[6];
        dt.loop_start = d[7]; dt.loop_kf = d[8]; dt.lc_start = d[9]; dt.lc_kf = d[10]; dt.corrected = d[11]; dt.non_corrected = d[12];
        dt.in_corrected = d[13]; dt.in_non_corrected = d[14]; dt.flags = d[15]; dt.ref_kf = d[16]; dt.corrected_by_kf = d[17];
        dt.corrected_ref = d[18]; dt.Tcw = d[19]; dt.world = d[20];
        orbhip_eg_out dout;
        dout.point_list = d[21]; dout.Scw = d[22]; dout.Swc = d[23]; dout.report = d[24];
        orbhip::Optimizer::OptimizeEssentialGraphDevice(matcher, cur, loop_row, rows, pcap, dt, fix_scale != 0, max_edges, dout);
        orbhip::check(orbhip_matcher_sync(matcher.handle()), "orbhip_matcher_sync");
        std::vector<float> Tcw2(Tcw0), world2(world0);
        if (download(Tcw2, d[19]) || download(world2, d[20]) || download(point_list, d[21]) || download(Scw, d[22]) || download(Swc, d[23]) ||
            download(report, d[24]))
            return 3;
        emit(out, Tcw2); emit(out, world2); emit(out, point_list); emit(out, Scw); emit(out, Swc); emit(out, report);
        for (int i = 0; i < 25; ++i) (void)hipFree(d[i]);
    } catch (const orbhip::Error &e) {
        fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 1;
    }
    fclose(out);
    return 0;
}
