// orbhip::Optimizer::LocalBundleAdjustment and LocalBundleAdjustmentDevice (include/orbhip/Optimizer.hpp) on one case of
// tests/test_lba_cpu.py.  Built with g++ against liborbhip.so and the HIP runtime (device memory for the device form).
//   lba_smoke <in> <out>   in:  the input of tests/cpp/lba_host.cpp (the script is ignored: stop is null)
//                          out: host mirror: int32 status, report[16], Tcw, world, then the four lists each as int32 length +
//                               entries; device form: Tcw, world, local_kf [rows], fixed_kf [rows], local_point [max_points],
//                               erase [max_edges][3], report [16] as the call left the caller's arrays
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
static void emit_list(FILE *f, const std::vector<int32_t> &v)
{
    const std::vector<int32_t> n(1, (int32_t)v.size());
    emit(f, n);
    emit(f, v);
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
    if (argc != 3) { fprintf(stderr, "usage: lba_smoke <in> <out>\n"); return 2; }
    std::vector<unsigned char> in = slurp(argv[1]);
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(16);
    const int cur = h[0], id0 = h[1], rows = h[2], cap = h[3], np = h[4], pcap = h[5], n_levels = h[6], max_points = h[7], max_edges = h[8];
    const size_t R = rows, RC = R * cap, P = pcap;
    const std::vector<float> camv = c.take<float>(5), inv = c.take<float>(n_levels);
    const std::vector<int32_t> slot_point = c.take<int32_t>(RC), n = c.take<int32_t>(R);
    const std::vector<uint8_t> kf_bad = c.take<uint8_t>(h[9] ? R : 0);
    const std::vector<int32_t> obs_start = c.take<int32_t>((size_t)np + 1);
    const size_t total = (size_t)obs_start[np];
    const std::vector<int32_t> obs_kf = c.take<int32_t>(total), obs_idx = c.take<int32_t>(total);
    const std::vector<uint8_t> flags = c.take<uint8_t>(P);
    const std::vector<orbhip_keypoint> kps = c.take<orbhip_keypoint>(RC);
    const std::vector<float> u_right = c.take<float>(h[10] ? RC : 0);
    const std::vector<int32_t> ord_kf = c.take<int32_t>(R * R), n_ord = c.take<int32_t>(R);
    const std::vector<float> Tcw0 = c.take<float>(R * 12), world0 = c.take<float>(P * 3);
    c.take<uint8_t>((size_t)h[12]);
    std::vector<int32_t> local_kf = c.take<int32_t>(R), fixed_kf = c.take<int32_t>(R), local_point = c.take<int32_t>((size_t)max_points);
    std::vector<int32_t> erase = c.take<int32_t>((size_t)max_edges * 3), report = c.take<int32_t>(16);

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
        orbhip_lba_tables t;
        t.slot_point = slot_point.data(); t.n = n.data(); t.kf_bad = h[9] ? kf_bad.data() : nullptr; t.obs_start = obs_start.data();
        t.obs_kf = obs_kf.data(); t.obs_idx = obs_idx.data(); t.flags = flags.data(); t.kps = kps.data();
        t.u_right = h[10] ? u_right.data() : nullptr; t.ord_kf = ord_kf.data(); t.n_ord = n_ord.data(); t.Tcw = Tcw.data(); t.world = world.data();
        orbhip::LocalBA ba;
        const bool stop = false;
        const int status = orbhip::Optimizer::LocalBundleAdjustment(matcher, cam, rows, cap, np, pcap, t, cur, id0, inv, max_points, max_edges,
                                                                    &stop, ba);
        emit(out, std::vector<int32_t>(1, status));
        emit(out, std::vector<int32_t>(ba.report, ba.report + 16));
        emit(out, Tcw); emit(out, world);
        emit_list(out, ba.lLocalKeyFrames); emit_list(out, ba.lFixedCameras); emit_list(out, ba.lLocalMapPoints); emit_list(out, ba.vToErase);
        printf("status %d local %zu fixed %zu points %zu erase %zu\n", status, ba.lLocalKeyFrames.size(), ba.lFixedCameras.size(),
               ba.lLocalMapPoints.size(), ba.vToErase.size() / 3);
        // the device form
        void *d[18];
        if (upload(slot_point, &d[0]) || upload(n, &d[1]) || upload(kf_bad, &d[2]) || upload(obs_start, &d[3]) || upload(obs_kf, &d[4]) ||
            upload(obs_idx, &d[5]) || upload(flags, &d[6]) || upload(kps, &d[7]) || upload(u_right, &d[8]) || upload(ord_kf, &d[9]) ||
            upload(n_ord, &d[10]) || upload(Tcw0, &d[11]) || upload(world0, &d[12]) || upload(local_kf, &d[13]) || upload(fixed_kf, &d[14]) ||
            upload(local_point, &d[15]) || upload(erase, &d[16]) || upload(report, &d[17]))
            return 3;
        orbhip_lba_tables dt;
        dt.slot_point = d[0]; dt.n = d[1]; dt.kf_bad = h[9] ? d[2] : nullptr; dt.obs_start = d[3]; dt.obs_kf = d[4]; dt.obs_idx = d[5];
        dt.flags = d[6]; dt.kps = d[7]; dt.u_right = h[10] ? d[8] : nullptr; dt.ord_kf = d[9]; dt.n_ord = d[10]; dt.Tcw = d[11]; dt.world = d[12];
        orbhip_lba_out dout;
        dout.local_kf = d[13]; dout.fixed_kf = d[14]; dout.local_point = d[15]; dout.erase = d[16]; dout.report = d[17];
        orbhip::Optimizer::LocalBundleAdjustmentDevice(matcher, cur, id0, cam, rows, cap, np, pcap, dt, inv, max_points, max_edges, nullptr, dout);
        orbhip::check(orbhip_matcher_sync(matcher.handle()), "orbhip_matcher_sync");
        std::vector<float> Tcw2(Tcw0), world2(world0);
        if (download(Tcw2, d[11]) || download(world2, d[12]) || download(local_kf, d[13]) || download(fixed_kf, d[14]) ||
            download(local_point, d[15]) || download(erase, d[16]) || download(report, d[17]))
            return 3;
        emit(out, Tcw2); emit(out, world2); emit(out, local_kf); emit(out, fixed_kf); emit(out, local_point); emit(out, erase); emit(out, report);
        for (int i = 0; i < 18; ++i) (void)hipFree(d[i]);
    } catch (const orbhip::Error &e) {
        fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 1;
    }
    fclose(out);
    return 0;
}
