// The C++ mirror of Optimizer::OptimizeSim3 (include/orbhip/Optimizer.hpp) the way LoopClosing::ComputeSim3 calls it
// (src/LoopClosing.cc:325-335): once per candidate on the Sim3 the solver returned.  Reads "rows cap np pcap cur C fixScale
// matchForm nLevels obsTotal" as int32 and fx fy cx cy th2 as float, then slotPoint[rows][cap], n[rows], obsStart[np+1],
// obsKf[obsTotal], obsIdx[obsTotal], flags[pcap], world[pcap][3], Tcw[rows][12], x[rows][cap], y[rows][cap], octave[rows][cap],
// kfIndex[C], matched12[C][cap], invLevelSigma2[nLevels], sim3[C][16]; writes, per candidate, the return value, report[8],
// g2oS12 as 8 doubles, Scw[12] (zeros on the early return) and vpMatches1[cap].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip/Optimizer.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: sim3opt_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[10];
    float k[5];
    if (std::fread(hdr, 4, 10, f) != 10 || std::fread(k, 4, 5, f) != 5) return 3;
    const size_t rows = (size_t)hdr[0], cap = (size_t)hdr[1], np = (size_t)hdr[2], pcap = (size_t)hdr[3], C = (size_t)hdr[5];
    const int cur = hdr[4], fixScale = hdr[6], matchForm = hdr[7], nLevels = hdr[8];
    const size_t obsTotal = (size_t)hdr[9];
    std::vector<int32_t> slotPoint, n, obsStart, obsKf, obsIdx, octave, kfIndex, matched;
    std::vector<uint8_t> flags;
    std::vector<float> world, Tcw, x, y, inv, sim3;
    if (!rd(f, slotPoint, rows * cap) || !rd(f, n, rows) || !rd(f, obsStart, np + 1) || !rd(f, obsKf, obsTotal) || !rd(f, obsIdx, obsTotal) ||
        !rd(f, flags, pcap) || !rd(f, world, pcap * 3) || !rd(f, Tcw, rows * 12) || !rd(f, x, rows * cap) || !rd(f, y, rows * cap) ||
        !rd(f, octave, rows * cap) || !rd(f, kfIndex, C) || !rd(f, matched, C * cap) || !rd(f, inv, (size_t)nLevels) || !rd(f, sim3, C * 16))
        return 3;
    std::fclose(f);
    std::vector<orbhip_keypoint> kps(rows * cap);
    std::memset(kps.data(), 0, kps.size() * sizeof(orbhip_keypoint));
    for (size_t i = 0; i < rows * cap; ++i) { kps[i].x = x[i]; kps[i].y = y[i]; kps[i].octave = octave[i]; }
    orbhip_sim3_tables t;
    t.slot_point = slotPoint.data(); t.obs_start = obsStart.data(); t.obs_kf = obsKf.data(); t.obs_idx = obsIdx.data();
    t.flags = flags.data(); t.world = world.data(); t.Tcw = Tcw.data(); t.kps = kps.data(); t.n = n.data();
    std::vector<float> sf((size_t)nLevels, 1.f);
    const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(k[0], k[1], k[2], k[3], 0.f, 0.f, 0.f, 640.f, 0.f, 480.f, sf, 0.f);
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        for (size_t c = 0; c < C; ++c) {
            std::vector<int32_t> vpMatches1(matched.begin() + c * cap, matched.begin() + (c + 1) * cap);
            orbhip::Sim3 gScm;
            float Scw[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int32_t report[8];
            const int32_t nInliers = orbhip::Optimizer::OptimizeSim3(matcher, cam, (int)rows, (int)cap, (int)np, (int)pcap, t, cur, kfIndex[c],
                                                                     vpMatches1, matchForm, inv, sim3.data() + c * 16, gScm, k[4],
                                                                     fixScale != 0, Scw, report);
            if (nInliers != report[3]) return 6;
            const double S12[8] = {gScm.r[0], gScm.r[1], gScm.r[2], gScm.r[3], gScm.t[0], gScm.t[1], gScm.t[2], gScm.s};
            std::fwrite(&nInliers, 4, 1, o);
            std::fwrite(report, 4, 8, o);
            std::fwrite(S12, 8, 8, o);
            std::fwrite(Scw, 4, 12, o);
            std::fwrite(vpMatches1.data(), 4, cap, o);
            std::printf("candidate %zu row %d pairs %d bad %d inliers %d match %d\n", c, kfIndex[c], report[1], report[2], nInliers,
                        nInliers >= 20 ? 1 : 0);                                // src/LoopClosing.cc:329
        }
        std::fclose(o);
        // a candidate outside the bank, a th2 of zero and a capacity over the limit: refused
        if (C) {
            std::vector<int32_t> m12(matched.begin(), matched.begin() + cap);
            orbhip::Sim3 g;
            try { orbhip::Optimizer::OptimizeSim3(matcher, cam, (int)rows, (int)cap, (int)np, (int)pcap, t, cur, (int)rows, m12, matchForm, inv, sim3.data(), g, k[4], false); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
            try { orbhip::Optimizer::OptimizeSim3(matcher, cam, (int)rows, (int)cap, (int)np, (int)pcap, t, cur, kfIndex[0], m12, matchForm, inv, sim3.data(), g, 0.f, false); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
            try { orbhip::Optimizer::OptimizeSim3(matcher, cam, (int)rows, 4097, (int)np, (int)pcap, t, cur, kfIndex[0], m12, matchForm, inv, sim3.data(), g, k[4], false); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_CAPACITY) return 6; }
        }
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
