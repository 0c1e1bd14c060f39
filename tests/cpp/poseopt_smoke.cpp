// The C++ mirror of Optimizer::PoseOptimization (include/orbhip/Optimizer.hpp) the way Tracking calls it: once on a frame,
// then the epilogue of the mode.  Reads "n np nLevels mode flags hasRight" as int32 and fx fy cx cy bf as float, then x[n],
// y[n], octave[n], uRight[n] (if hasRight), mapPoints[n], world[np][3], pointFlags[np], invLevelSigma2[nLevels], Tcw[12];
// writes the return value, report[8], Tcw[12], mvbOutlier[n], mvpMapPoints[n] and discarded[n].
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
    if (argc < 3) { std::fprintf(stderr, "usage: poseopt_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[6];
    float k[5];
    if (std::fread(hdr, 4, 6, f) != 6 || std::fread(k, 4, 5, f) != 5) return 3;
    const size_t n = (size_t)hdr[0], np = (size_t)hdr[1];
    const int nLevels = hdr[2], mode = hdr[3], flags = hdr[4];
    std::vector<float> x, y, ur, world, inv, tcw;
    std::vector<int32_t> octave, points;
    std::vector<uint8_t> pflags;
    if (!rd(f, x, n) || !rd(f, y, n) || !rd(f, octave, n) || !rd(f, ur, hdr[5] ? n : 0) || !rd(f, points, n) || !rd(f, world, np * 3) ||
        !rd(f, pflags, np) || !rd(f, inv, (size_t)nLevels) || !rd(f, tcw, 12))
        return 3;
    std::fclose(f);
    orbhip::PoseFrame F;
    F.mvKeysUn.resize(n);
    if (n) std::memset(F.mvKeysUn.data(), 0, n * sizeof(orbhip_keypoint));
    for (size_t i = 0; i < n; ++i) { F.mvKeysUn[i].x = x[i]; F.mvKeysUn[i].y = y[i]; F.mvKeysUn[i].octave = octave[i]; }
    F.mvuRight = ur;
    F.mvpMapPoints = points;
    F.mvbOutlier.assign(n, 1);
    for (int i = 0; i < 12; ++i) F.mTcw[i] = tcw[(size_t)i];
    std::vector<float> sf((size_t)nLevels, 1.f);
    const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(k[0], k[1], k[2], k[3], k[4], 0.f, 0.f, 1241.f, 0.f, 376.f, sf, 0.f);
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        std::vector<int32_t> discarded;
        int32_t report[8];
        const int32_t ret = orbhip::Optimizer::PoseOptimization(matcher, cam, F, world, pflags, inv, mode, flags, &discarded, report);
        if (ret != report[3] || discarded.size() != n) return 6;
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        std::fwrite(&ret, 4, 1, o);
        std::fwrite(report, 4, 8, o);
        std::fwrite(F.mTcw, 4, 12, o);
        std::fwrite(F.mvbOutlier.data(), 1, n, o);
        std::fwrite(F.mvpMapPoints.data(), 4, n, o);
        std::fwrite(discarded.data(), 4, n, o);
        std::fclose(o);
        std::printf("edges %d bad %d returned %d rounds %d iterations %d\n", report[1], report[2], ret, report[4], report[5]);
        // a mode the library does not know: refused
        try { orbhip::Optimizer::PoseOptimization(matcher, cam, F, world, pflags, inv, 7, 0); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        // flags that do not cover the map: refused by the mirror before anything is read
        if (np > 1) {
            const std::vector<uint8_t> shortFlags(pflags.begin(), pflags.begin() + (np - 1));
            try { orbhip::Optimizer::PoseOptimization(matcher, cam, F, world, shortFlags, inv, mode, flags); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        }
        // an empty map and a frame without points: no edge, return 0
        orbhip::PoseFrame E = F;
        E.mvpMapPoints.assign(n, -1);
        int32_t r0[8];
        if (orbhip::Optimizer::PoseOptimization(matcher, cam, E, std::vector<float>(), std::vector<uint8_t>(), inv, ORBHIP_POSEOPT_PLAIN, 0,
                                                nullptr, r0) != 0 || r0[0] != ORBHIP_POSEOPT_TOO_FEW || r0[1] != 0)
            return 6;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
