// ORBmatcher::FuseBatch of the C++ mirror (include/orbhip/ORBextractor.hpp) the way LocalMapping::SearchInNeighbors uses
// ORBmatcher::Fuse (src/LocalMapping.cc:454-515): one set of map points against K key frames.  Reads "K n sim3Form
// nLevels" as int32, "fx fy cx cy mbf mb maxX maxY logScaleFactor th" as floats, scaleFactors[nLevels],
// invLevelSigma2[nLevels]; per key frame "nk hasRight" as int32, Tcw[12], keys[nk], desc[nk][32], uRight[nk] when
// hasRight; then world[n][3], normal[n][3], maxDist[n], minDist[n], pointDesc[n][32], flags[K][n].  Writes
// bestIdx[K][n] and bestDist[K][n].
#include <cstdio>
#include <vector>

#include "orbhip/ORBextractor.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: fuse_batch_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[4];
    float cf[10];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(cf, 4, 10, f) != 10) return 3;
    const int K = hdr[0], n = hdr[1];
    std::vector<float> sf, sig;
    if (!rd(f, sf, (size_t)hdr[3]) || !rd(f, sig, (size_t)hdr[3])) return 3;
    std::vector<std::vector<orbhip::KeyPoint> > keys(K);
    std::vector<std::vector<uint8_t> > desc(K);
    std::vector<std::vector<float> > uRight(K);
    std::vector<orbhip_frame_view> views(K);
    std::vector<float> Tcw((size_t)K * 12);
    for (int k = 0; k < K; ++k) {
        int32_t kh[2];
        if (std::fread(kh, 4, 2, f) != 2 || std::fread(&Tcw[(size_t)k * 12], 4, 12, f) != 12) return 3;
        if (!rd(f, keys[k], (size_t)kh[0]) || !rd(f, desc[k], (size_t)kh[0] * 32)) return 3;
        if (kh[1] && !rd(f, uRight[k], (size_t)kh[0])) return 3;
        views[k] = orbhip::ORBmatcher::MakeFrameView(keys[k], desc[k], kh[1] ? uRight[k].data() : nullptr, 0.f, 0.f, cf[6], cf[7], sf);
    }
    std::vector<float> world, normal, maxDist, minDist;
    std::vector<uint8_t> pointDesc, flags;
    if (!rd(f, world, (size_t)n * 3) || !rd(f, normal, (size_t)n * 3) || !rd(f, maxDist, (size_t)n) || !rd(f, minDist, (size_t)n) ||
        !rd(f, pointDesc, (size_t)n * 32) || !rd(f, flags, (size_t)K * n)) return 3;
    std::fclose(f);
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(cf[0], cf[1], cf[2], cf[3], cf[4], cf[5], 0.f, cf[6], 0.f, cf[7], sf, cf[8]);
        std::vector<const orbhip_frame_view *> kfs;
        for (int k = 0; k < K; ++k) kfs.push_back(&views[k]);
        std::vector<int> bestIdx, bestDist;
        matcher.FuseBatch(kfs, cam, Tcw.data(), hdr[2] != 0, n, world.data(), normal.data(), maxDist.data(), minDist.data(),
                          flags.data(), pointDesc.data(), cf[9], sig.data(), bestIdx, bestDist);
        if (bestIdx.size() != (size_t)K * n || bestDist.size() != (size_t)K * n) return 4;
        // every row is what the single-frame member gives
        int fused = 0;
        for (int k = 0; k < K; ++k) {
            std::vector<int> bi, bd;
            matcher.Fuse(views[k], cam, &Tcw[(size_t)k * 12], hdr[2] != 0, n, world.data(), normal.data(), maxDist.data(),
                         minDist.data(), &flags[(size_t)k * n], pointDesc.data(), cf[9], sig.data(), bi, bd);
            for (int i = 0; i < n; ++i) {
                if (bi[i] != bestIdx[(size_t)k * n + i] || bd[i] != bestDist[(size_t)k * n + i]) return 4;
                fused += bd[i] <= 50;
            }
        }
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        std::fwrite(bestIdx.data(), 4, bestIdx.size(), o);
        std::fwrite(bestDist.data(), 4, bestDist.size(), o);
        std::fclose(o);
        std::printf("key frames %d points %d within TH_LOW %d\n", K, n, fused);
        // no key frames and no points: nothing; a level count the camera cannot hold: ORBHIP_E_ARG
        std::vector<const orbhip_frame_view *> none;
        matcher.FuseBatch(none, cam, Tcw.data(), false, n, world.data(), normal.data(), maxDist.data(), minDist.data(), flags.data(),
                          pointDesc.data(), cf[9], sig.data(), bestIdx, bestDist);
        if (!bestIdx.empty()) return 4;
        matcher.FuseBatch(kfs, cam, Tcw.data(), false, 0, world.data(), normal.data(), maxDist.data(), minDist.data(), flags.data(),
                          pointDesc.data(), cf[9], sig.data(), bestIdx, bestDist);
        if (!bestIdx.empty()) return 4;
        orbhip_camera bad = cam;
        bad.n_levels = ORBHIP_MAX_LEVELS + 1;
        try {
            matcher.FuseBatch(kfs, bad, Tcw.data(), false, n, world.data(), normal.data(), maxDist.data(), minDist.data(),
                              flags.data(), pointDesc.data(), cf[9], sig.data(), bestIdx, bestDist);
            return 6;
        } catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
