// The C++ mirror of Sim3Solver (include/orbhip/Sim3Solver.hpp) the way LoopClosing::ComputeSim3 drives it
// (src/LoopClosing.cc:238-342): one solver per candidate, iterate(5) again and again until bNoMore.  Reads
// "rows cap np pcap cur C minInliers maxIts fixScale matchForm nLevels obsTotal" as int32 and fx fy cx cy as float, then
// slotPoint[rows][cap], n[rows], obsStart[np+1], obsKf[obsTotal], obsIdx[obsTotal], flags[pcap], world[pcap][3], Tcw[rows][12],
// octave[rows][cap], kfIndex[C], matched12[C][cap], levelSigma2[nLevels], draws[C][maxIts][3]; writes, per candidate, the number
// of calls and per call report[8], the estimate (R12[9], t12[3], s12; zeros where nothing was returned) and vbInliers[n[cur]].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip/Sim3Solver.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: sim3_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[12];
    float k[4];
    if (std::fread(hdr, 4, 12, f) != 12 || std::fread(k, 4, 4, f) != 4) return 3;
    const size_t rows = (size_t)hdr[0], cap = (size_t)hdr[1], np = (size_t)hdr[2], pcap = (size_t)hdr[3], C = (size_t)hdr[5];
    const int cur = hdr[4], minInliers = hdr[6], maxIts = hdr[7], fixScale = hdr[8], matchForm = hdr[9], nLevels = hdr[10];
    const size_t obsTotal = (size_t)hdr[11];
    std::vector<int32_t> slotPoint, n, obsStart, obsKf, obsIdx, octave, kfIndex, matched, draws;
    std::vector<uint8_t> flags;
    std::vector<float> world, Tcw, sigma2;
    if (!rd(f, slotPoint, rows * cap) || !rd(f, n, rows) || !rd(f, obsStart, np + 1) || !rd(f, obsKf, obsTotal) || !rd(f, obsIdx, obsTotal) ||
        !rd(f, flags, pcap) || !rd(f, world, pcap * 3) || !rd(f, Tcw, rows * 12) || !rd(f, octave, rows * cap) || !rd(f, kfIndex, C) ||
        !rd(f, matched, C * cap) || !rd(f, sigma2, (size_t)nLevels) || !rd(f, draws, C * (size_t)maxIts * 3))
        return 3;
    std::fclose(f);
    std::vector<orbhip_keypoint> kps(rows * cap);
    std::memset(kps.data(), 0, kps.size() * sizeof(orbhip_keypoint));
    for (size_t i = 0; i < rows * cap; ++i) kps[i].octave = octave[i];
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
            const std::vector<int32_t> m12(matched.begin() + c * cap, matched.begin() + (c + 1) * cap);
            orbhip::Sim3Solver solver(matcher, cam, (int)rows, (int)cap, (int)np, (int)pcap, t, cur, kfIndex[c], m12, matchForm, sigma2,
                                      fixScale != 0);
            solver.SetRansacParameters(0.99, minInliers, maxIts);
            solver.SetDraws(std::vector<int32_t>(draws.begin() + c * (size_t)maxIts * 3, draws.begin() + (c + 1) * (size_t)maxIts * 3));
            std::vector<int32_t> reports;
            std::vector<float> estimates;
            std::vector<uint8_t> marks;
            bool bNoMore = false;
            int calls = 0, returned = 0;
            while (!bNoMore) {                                                  // src/LoopClosing.cc:274-334
                std::vector<bool> vbInliers;
                int nInliers = 0;
                const bool got = solver.iterate(5, bNoMore, vbInliers, nInliers);
                if (got && nInliers != solver.Report()[6]) return 6;
                reports.insert(reports.end(), solver.Report(), solver.Report() + 8);
                for (int i = 0; i < 13; ++i)
                    estimates.push_back(!got ? 0.f : i < 9 ? solver.GetEstimatedRotation()[i] : i < 12 ? solver.GetEstimatedTranslation()[i - 9]
                                                                                                      : solver.GetEstimatedScale());
                for (size_t i = 0; i < vbInliers.size(); ++i) marks.push_back(vbInliers[i] ? 1 : 0);
                returned += got;
                if (++calls > maxIts + 2) return 7;
            }
            const int32_t ncalls = calls;
            std::fwrite(&ncalls, 4, 1, o);
            std::fwrite(reports.data(), 4, reports.size(), o);
            std::fwrite(estimates.data(), 4, estimates.size(), o);
            std::fwrite(marks.data(), 1, marks.size(), o);
            std::printf("candidate %zu row %d N %d limit %d calls %d returned %d\n", c, kfIndex[c], solver.Report()[1], solver.Report()[2],
                        calls, returned);
        }
        std::fclose(o);
        // a candidate outside the bank and a capacity over the limit: refused
        if (C) {
            const std::vector<int32_t> m12(matched.begin(), matched.begin() + cap);
            orbhip::Sim3Solver bad(matcher, cam, (int)rows, (int)cap, (int)np, (int)pcap, t, cur, (int)rows, m12, matchForm, sigma2, false);
            bad.SetRansacParameters(0.99, minInliers, maxIts);
            std::vector<bool> v;
            int ni;
            try { bad.find(v, ni); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
            orbhip::Sim3Solver big(matcher, cam, (int)rows, 4097, (int)np, (int)pcap, t, cur, kfIndex[0], m12, matchForm, sigma2, false);
            big.SetRansacParameters(0.99, minInliers, maxIts);
            try { big.find(v, ni); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_CAPACITY) return 6; }
        }
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
