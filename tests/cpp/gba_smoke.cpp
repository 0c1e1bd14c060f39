// orbhip::Optimizer::BundleAdjustment and BundleAdjustmentDevice (include/orbhip/Optimizer.hpp) on one case of
// tests/test_gba_cpu.py.  Built with g++ against liborbhip.so and the HIP runtime (device memory for the device form).
//   gba_smoke <in> <out>   in:  the input of `gba_host ba` (tests/cpp/gba_host.cpp; the script is ignored: stop is null)
//                          out: host mirror: int32 status, report[16], Tcw, world, TcwGBA, posGBA, kfMark, ptMark, then
//                               vpUpdatedPoints as int32 length + entries; device form: Tcw, world, TcwGBA, posGBA, kf_mark,
//                               pt_mark, point_list [max_points], report [16] as the call left the caller's arrays, then the two
//                               counters
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

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: gba_smoke <in> <out>\n"); return 2; }
    std::vector<unsigned char> in = slurp(argv[1]);
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(24);
    const int rows = h[0], cap = h[1], np = h[2], pcap = h[3], n_levels = h[4], max_points = h[5], max_edges = h[6];
    const int iterations = h[15], robust = h[16], mode = h[17];
    const size_t R = rows, RC = R * cap, P = pcap;
    const std::vector<float> camv = c.take<float>(5), inv = c.take<float>(n_levels);
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(h[7] ? R : 0);
    const std::vector<int32_t> kf_id = c.take<int32_t>(R), obs_start = c.take<int32_t>((size_t)np + 1);
    const size_t total = (size_t)obs_start[np];
    const std::vector<int32_t> obs_kf = c.take<int32_t>(total), obs_idx = c.take<int32_t>(total);
    const std::vector<uint8_t> flags = c.take<uint8_t>(P);
    const std::vector<orbhip_keypoint> kps = c.take<orbhip_keypoint>(RC);
    const std::vector<float> u_right = c.take<float>(h[8] ? RC : 0);
    const std::vector<float> Tcw0 = c.take<float>(R * 12), world0 = c.take<float>(P * 3);
    c.take<uint8_t>((size_t)h[10]);
    const std::vector<int32_t> kf_list = c.take<int32_t>(h[11] ? (size_t)h[12] : 0), pt_list = c.take<int32_t>(h[13] ? (size_t)h[14] : 0);
    std::vector<float> TcwGBA = c.take<float>(R * 12), posGBA = c.take<float>(P * 3);
    std::vector<uint8_t> kf_mark = c.take<uint8_t>(R), pt_mark = c.take<uint8_t>(P);
    std::vector<int32_t> point_list = c.take<int32_t>((size_t)max_points), report = c.take<int32_t>(16);

    orbhip_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3]; cam.mbf = camv[4];
    cam.max_x = 1241.f; cam.max_y = 376.f; cam.n_levels = n_levels;
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        // the host mirror
        std::vector<float> Tcw(Tcw0), world(world0);
        orbhip_gba_tables t;
        t.kf_bad = h[7] ? kf_bad.data() : nullptr; t.kf_id = kf_id.data(); t.obs_start = obs_start.data(); t.obs_kf = obs_kf.data();
        t.obs_idx = obs_idx.data(); t.flags = flags.data(); t.kps = kps.data(); t.u_right = h[8] ? u_right.data() : nullptr;
        t.Tcw = Tcw.data(); t.world = world.data();
        orbhip::GlobalBA ba;
        const int status = orbhip::Optimizer::BundleAdjustment(matcher, cam, rows, cap, np, pcap, t, h[11] ? &kf_list : nullptr,
                                                               h[13] ? &pt_list : nullptr, inv, iterations, nullptr,
                                                               mode == ORBHIP_GBA_STAGED ? 7ul : 0ul, robust != 0, max_points, max_edges, ba);
        emit(out, std::vector<int32_t>(1, status));
        emit(out, std::vector<int32_t>(ba.report, ba.report + 16));
        emit(out, Tcw); emit(out, world); emit(out, ba.TcwGBA); emit(out, ba.posGBA); emit(out, ba.kfMark); emit(out, ba.ptMark);
        emit(out, std::vector<int32_t>(1, (int32_t)ba.vpUpdatedPoints.size()));
        emit(out, ba.vpUpdatedPoints);
        printf("status %d vertices %d free %d points %d iterations %d trials %d\n", status, ba.report[1], ba.report[2], ba.report[3],
               ba.report[9], ba.report[10]);
        // the device form
        void *d[18];
        if (upload(kf_bad, &d[0]) || upload(kf_id, &d[1]) || upload(obs_start, &d[2]) || upload(obs_kf, &d[3]) || upload(obs_idx, &d[4]) ||
            upload(flags, &d[5]) || upload(kps, &d[6]) || upload(u_right, &d[7]) || upload(Tcw0, &d[8]) || upload(world0, &d[9]) ||
            upload(kf_list, &d[10]) || upload(pt_list, &d[11]) || upload(TcwGBA, &d[12]) || upload(posGBA, &d[13]) ||
            upload(kf_mark, &d[14]) || upload(pt_mark, &d[15]) || upload(point_list, &d[16]) || upload(report, &d[17]))
            return 3;
        orbhip_gba_tables dt;
        dt.kf_bad = h[7] ? d[0] : nullptr; dt.kf_id = d[1]; dt.obs_start = d[2]; dt.obs_kf = d[3]; dt.obs_idx = d[4]; dt.flags = d[5];
        dt.kps = d[6]; dt.u_right = h[8] ? d[7] : nullptr; dt.Tcw = d[8]; dt.world = d[9];
        orbhip_gba_out dout;
        dout.TcwGBA = d[12]; dout.posGBA = d[13]; dout.kf_mark = d[14]; dout.pt_mark = d[15]; dout.point_list = d[16]; dout.report = d[17];
        orbhip::Optimizer::BundleAdjustmentDevice(matcher, cam, rows, cap, np, pcap, dt, inv, h[11] ? d[10] : nullptr, h[12],
                                                  h[13] ? d[11] : nullptr, h[14], iterations, robust != 0, mode, max_points, max_edges,
                                                  nullptr, dout);
        std::vector<float> Tcw2(Tcw0), world2(world0);
        if (download(Tcw2, d[8]) || download(world2, d[9]) || download(TcwGBA, d[12]) || download(posGBA, d[13]) || download(kf_mark, d[14]) ||
            download(pt_mark, d[15]) || download(point_list, d[16]) || download(report, d[17]))
            return 3;
        emit(out, Tcw2); emit(out, world2); emit(out, TcwGBA); emit(out, posGBA); emit(out, kf_mark); emit(out, pt_mark); emit(out, point_list);
        emit(out, report);
        std::vector<int32_t> counters(2, 0);
        orbhip::check(orbhip_global_bundle_adjustment_counters(matcher.handle(), counters.data()), "orbhip_global_bundle_adjustment_counters");
        emit(out, counters);
        for (int i = 0; i < 18; ++i) (void)hipFree(d[i]);
    } catch (const orbhip::Error &e) {
        fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 1;
    }
    fclose(out);
    return 0;
}
