// ORBmatcher::CreateNewMapPoints of the C++ mirror (include/orbhip/ORBextractor.hpp) the way
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-452) would call it: the current key frame against K
// neighbours.  Reads "K nLevels checkOri onlyStereo" as int32, "fx fy cx cy mbf mb maxX maxY logScaleFactor" as floats,
// scaleFactors[nLevels], levelSigma2[nLevels]; then K + 1 frames (the current one first), each "n" as int32, Tcw[12],
// keys[n], desc[n][32], uRight[n], depth[n], node[n] (uint32), hasPoint[n].  Writes matches12[K][n0] (int32),
// nmatches[K] (int32), x3D[K][n0][3] (float), status[K][n0], skipped[K] (bytes).
#include <cstdio>
#include <vector>

#include "orbhip/ORBextractor.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: triangulate_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[4];
    float cf[9];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(cf, 4, 9, f) != 9) return 3;
    const int K = hdr[0], R = K + 1;
    std::vector<float> sf, sigma2;
    if (!rd(f, sf, (size_t)hdr[1]) || !rd(f, sigma2, (size_t)hdr[1])) return 3;
    std::vector<std::vector<orbhip::KeyPoint> > keys(R);
    std::vector<std::vector<uint8_t> > desc(R), hasPoint(R);
    std::vector<std::vector<float> > uRight(R), depth(R);
    std::vector<std::vector<uint32_t> > node(R);
    std::vector<orbhip_frame_view> views(R);
    std::vector<float> Tcw((size_t)R * 12);
    for (int r = 0; r < R; ++r) {
        int32_t n;
        if (std::fread(&n, 4, 1, f) != 1 || std::fread(&Tcw[(size_t)r * 12], 4, 12, f) != 12) return 3;
        if (!rd(f, keys[r], (size_t)n) || !rd(f, desc[r], (size_t)n * 32) || !rd(f, uRight[r], (size_t)n) ||
            !rd(f, depth[r], (size_t)n) || !rd(f, node[r], (size_t)n) || !rd(f, hasPoint[r], (size_t)n)) return 3;
        views[r] = orbhip::ORBmatcher::MakeFrameView(keys[r], desc[r], uRight[r].data(), 0.f, 0.f, cf[6], cf[7], sf);
    }
    std::fclose(f);
    try {
        orbhip::ORBmatcher matcher(0.6f, hdr[2] != 0);
        const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(cf[0], cf[1], cf[2], cf[3], cf[4], cf[5], 0.f, cf[6], 0.f, cf[7], sf, cf[8]);
        std::vector<const orbhip_frame_view *> kfs;
        std::vector<const uint32_t *> nodes;
        std::vector<const uint8_t *> hps;
        std::vector<const float *> depths;
        for (int r = 1; r < R; ++r) {
            kfs.push_back(&views[r]); nodes.push_back(node[r].data()); hps.push_back(hasPoint[r].data());
            depths.push_back(depth[r].data());
        }
        orbhip::ORBmatcher::NewMapPoints out;
        matcher.CreateNewMapPoints(views[0], node[0].data(), hasPoint[0].data(), depth[0].data(), &Tcw[0], kfs, nodes, hps, depths,
                                   &Tcw[12], nullptr, cam, hdr[3] != 0, sigma2.data(), out);
        const size_t n0 = keys[0].size();
        if (out.matches12.size() != (size_t)K * n0 || out.status.size() != (size_t)K * n0 || out.nmatches.size() != (size_t)K) return 4;
        int created = 0;
        for (size_t i = 0; i < out.status.size(); ++i) created += out.status[i] == ORBHIP_NEWPOINT_CREATED;
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        std::fwrite(out.matches12.data(), 4, out.matches12.size(), o);
        std::fwrite(out.nmatches.data(), 4, out.nmatches.size(), o);
        std::fwrite(out.x3D.data(), 4, out.x3D.size(), o);
        std::fwrite(out.status.data(), 1, out.status.size(), o);
        std::fwrite(out.skipped.data(), 1, out.skipped.size(), o);
        std::fclose(o);
        std::printf("neighbours %d key points %d created %d\n", K, (int)n0, created);
        // no neighbours: nothing; a level count the camera cannot hold: ORBHIP_E_ARG
        std::vector<const orbhip_frame_view *> none;
        std::vector<const uint32_t *> no_nodes;
        matcher.CreateNewMapPoints(views[0], node[0].data(), hasPoint[0].data(), depth[0].data(), &Tcw[0], none, no_nodes, hps,
                                   depths, &Tcw[12], nullptr, cam, false, sigma2.data(), out);
        if (!out.matches12.empty() || !out.nmatches.empty()) return 4;
        orbhip_camera bad = cam;
        bad.n_levels = ORBHIP_MAX_LEVELS + 1;
        try {
            matcher.CreateNewMapPoints(views[0], node[0].data(), hasPoint[0].data(), depth[0].data(), &Tcw[0], kfs, nodes, hps,
                                       depths, &Tcw[12], nullptr, bad, false, sigma2.data(), out);
            return 6;
        } catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
