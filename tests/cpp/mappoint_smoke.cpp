// The map-point refresh of the C++ mirror (include/orbhip/ORBextractor.hpp: UpdateMapPoints) the way LocalMapping uses
// MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371).  Reads
// "K nkeys np nobs what nLevels hasBad" as int32, scaleFactors[nLevels] and Tcw[K][12] as floats, kfBad[K], then per key
// frame keys[nkeys] and desc[nkeys][32], then obsStart[np+1], obsKf[nobs], obsIdx[nobs], refObs[np], world[np][3],
// flags[np] and the current pointDesc[np][32], normal[np][3], maxDist[np], minDist[np]; writes the four arrays, bestObs[np]
// and status[np].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbhip/ORBextractor.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: mappoint_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[7];
    if (std::fread(hdr, 4, 7, f) != 7) return 3;
    const size_t K = (size_t)hdr[0], nkeys = (size_t)hdr[1], np = (size_t)hdr[2], nobs = (size_t)hdr[3];
    const int what = hdr[4];
    std::vector<float> sf, Tcw, world, normal, maxDist, minDist;
    std::vector<uint8_t> kfBad, flags, pointDesc;
    std::vector<int32_t> obsStart, obsKf, obsIdx, refObs;
    std::vector<std::vector<orbhip::KeyPoint> > keys(K);
    std::vector<std::vector<uint8_t> > desc(K);
    if (!rd(f, sf, (size_t)hdr[5]) || !rd(f, Tcw, 12 * K) || !rd(f, kfBad, K)) return 3;
    for (size_t k = 0; k < K; ++k)
        if (!rd(f, keys[k], nkeys) || !rd(f, desc[k], 32 * nkeys)) return 3;
    if (!rd(f, obsStart, np + 1) || !rd(f, obsKf, nobs) || !rd(f, obsIdx, nobs) || !rd(f, refObs, np) || !rd(f, world, 3 * np) ||
        !rd(f, flags, np) || !rd(f, pointDesc, 32 * np) || !rd(f, normal, 3 * np) || !rd(f, maxDist, np) || !rd(f, minDist, np))
        return 3;
    std::fclose(f);
    if (!hdr[6]) kfBad.clear();
    try {
        orbhip::ORBmatcher matcher(0.9f, true);
        const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(500.f, 500.f, 320.f, 240.f, 0.f, 0.f, 0.f, 640.f, 0.f, 480.f, sf, 0.f);
        std::vector<orbhip_frame_view> views(K);
        std::vector<const orbhip_frame_view *> KFs(K);
        for (size_t k = 0; k < K; ++k) {
            views[k] = orbhip::ORBmatcher::MakeFrameView(keys[k], desc[k], nullptr, 0.f, 0.f, 640.f, 480.f, sf);
            KFs[k] = &views[k];
        }
        std::vector<int32_t> bestObs;
        std::vector<uint8_t> status;
        matcher.UpdateMapPoints(cam, what, KFs, Tcw, kfBad, obsStart, obsKf, obsIdx, refObs, world, flags, pointDesc, normal, maxDist,
                                minDist, bestObs, status);
        if (bestObs.size() != np || status.size() != np) return 4;
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        std::fwrite(pointDesc.data(), 1, pointDesc.size(), o);
        std::fwrite(normal.data(), 4, normal.size(), o);
        std::fwrite(maxDist.data(), 4, maxDist.size(), o);
        std::fwrite(minDist.data(), 4, minDist.size(), o);
        std::fwrite(bestObs.data(), 4, bestObs.size(), o);
        std::fwrite(status.data(), 1, status.size(), o);
        std::fclose(o);
        size_t updated = 0;
        for (size_t p = 0; p < np; ++p) updated += status[p] == ORBHIP_MAPPOINT_UPDATED;
        std::printf("points %zu updated %zu\n", np, updated);
        // a mask of 0, a row outside the bank and mismatched sizes: ORBHIP_E_ARG, nothing changed
        const std::vector<uint8_t> before = pointDesc;
        try { matcher.UpdateMapPoints(cam, 0, KFs, Tcw, kfBad, obsStart, obsKf, obsIdx, refObs, world, flags, pointDesc, normal, maxDist, minDist, bestObs, status); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        if (nobs) {
            std::vector<int32_t> wrong = obsKf;
            wrong[nobs - 1] = (int32_t)K;
            try { matcher.UpdateMapPoints(cam, what, KFs, Tcw, kfBad, obsStart, wrong, obsIdx, refObs, world, flags, pointDesc, normal, maxDist, minDist, bestObs, status); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        }
        std::vector<float> shorter(world.begin(), world.end() - (np ? 1 : 0));
        if (np) {
            try { matcher.UpdateMapPoints(cam, what, KFs, Tcw, kfBad, obsStart, obsKf, obsIdx, refObs, shorter, flags, pointDesc, normal, maxDist, minDist, bestObs, status); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        }
        if (pointDesc != before) return 7;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
