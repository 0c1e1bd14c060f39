// The C++ mirror of PnPsolver (include/orbhip/PnPsolver.hpp) the way Tracking::Relocalization drives it
// (src/Tracking.cc:1400-1425): one solver per candidate, iterate(5) again and again until bNoMore (at most maxCalls times).
// Reads "n np pcap C nLevels drawRows minInliers maxIts maxCalls" as int32 and fx fy cx cy epsilon th2 as float, then x[n],
// y[n], octave[n], flags[pcap], world[pcap][3], matches[C][n], levelSigma2[nLevels], draws[C][drawRows][4]; writes, per
// candidate, the number of calls and per call report[8], Tcw[12] (zeros where nothing was returned) and vbInliers[n] (zeros
// likewise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip/PnPsolver.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: pnp_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[9];
    float k[6];
    if (std::fread(hdr, 4, 9, f) != 9 || std::fread(k, 4, 6, f) != 6) return 3;
    const size_t n = (size_t)hdr[0], pcap = (size_t)hdr[2], C = (size_t)hdr[3], drawRows = (size_t)hdr[5];
    const int np = hdr[1], nLevels = hdr[4], minInliers = hdr[6], maxIts = hdr[7], maxCalls = hdr[8];
    std::vector<float> x, y, world, sigma2;
    std::vector<int32_t> octave, matches, draws;
    std::vector<uint8_t> flags;
    if (!rd(f, x, n) || !rd(f, y, n) || !rd(f, octave, n) || !rd(f, flags, pcap) || !rd(f, world, pcap * 3) || !rd(f, matches, C * n) ||
        !rd(f, sigma2, (size_t)nLevels) || !rd(f, draws, C * drawRows * 4))
        return 3;
    std::fclose(f);
    std::vector<orbhip_keypoint> kps(n);
    if (n) std::memset(kps.data(), 0, n * sizeof(orbhip_keypoint));
    for (size_t i = 0; i < n; ++i) { kps[i].x = x[i]; kps[i].y = y[i]; kps[i].octave = octave[i]; }
    orbhip_pnp_map map;
    map.flags = flags.data(); map.world = world.data(); map.slot_point = nullptr;
    std::vector<float> sf((size_t)nLevels, 1.f);
    const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(k[0], k[1], k[2], k[3], 0.f, 0.f, 0.f, 1241.f, 0.f, 376.f, sf, 0.f);
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        for (size_t c = 0; c < C; ++c) {
            const std::vector<int32_t> mt(matches.begin() + c * n, matches.begin() + (c + 1) * n);
            orbhip::PnPsolver solver(matcher, cam, kps, np, (int)pcap, map, mt, sigma2);
            solver.SetRansacParameters(0.99, minInliers, maxIts, 4, k[4], k[5]);
            solver.SetDraws(std::vector<int32_t>(draws.begin() + c * drawRows * 4, draws.begin() + (c + 1) * drawRows * 4));
            std::vector<int32_t> reports;
            std::vector<float> poses;
            std::vector<uint8_t> marks;
            bool bNoMore = false;
            int calls = 0, returned = 0;
            while (!bNoMore && calls < maxCalls) {
                std::vector<bool> vbInliers;
                int nInliers = 0;
                const bool got = solver.iterate(5, bNoMore, vbInliers, nInliers);
                if (nInliers != solver.Report()[6] || (got && vbInliers.size() != n) || (!got && !vbInliers.empty())) return 6;
                reports.insert(reports.end(), solver.Report(), solver.Report() + 8);
                for (int i = 0; i < 12; ++i) poses.push_back(got ? solver.GetTcw()[i] : 0.f);
                for (size_t i = 0; i < n; ++i) marks.push_back(got && vbInliers[i] ? 1 : 0);
                returned += got;
                ++calls;
            }
            const int32_t ncalls = calls;
            std::fwrite(&ncalls, 4, 1, o);
            std::fwrite(reports.data(), 4, reports.size(), o);
            std::fwrite(poses.data(), 4, poses.size(), o);
            std::fwrite(marks.data(), 1, marks.size(), o);
            std::printf("candidate %zu N %d limit %d calls %d returned %d\n", c, solver.Report()[1], solver.Report()[2], calls, returned);
        }
        std::fclose(o);
        // a sample size other than four: refused
        if (C) {
            const std::vector<int32_t> mt(matches.begin(), matches.begin() + n);
            orbhip::PnPsolver bad(matcher, cam, kps, np, (int)pcap, map, mt, sigma2);
            bad.SetRansacParameters(0.99, minInliers, maxIts, 5, k[4], k[5]);
            bad.SetDraws(std::vector<int32_t>(draws.begin(), draws.begin() + drawRows * 4));
            std::vector<bool> v;
            int ni;
            try { bad.find(v, ni); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        }
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
