// The seeding part of the C++ mirror (include/orbhip/ORBextractor.hpp: SeedStereoPoints, UnprojectStereo,
// CountClosePoints) the way Tracking::UpdateLastFrame / StereoInitialization / NeedNewKeyFrame use the reference classes
// (src/Tracking.cc:812-864, 523-538, 1001-1018).  Reads "n mode createdFlags" as int32, "fx fy cx cy thDepth" and Tcw[12]
// as floats, then keys[n], depth[n], world[n][3], flags[n]; writes world, flags, counts[3], order[nVisited], created[n],
// the two close counts, and UnprojectStereo of keypoint `probe` (valid flag as int32 + 3 floats).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbhip/ORBextractor.hpp"

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: seed_smoke in.bin probe out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[3];
    float cf[5], Tcw[12];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(cf, 4, 5, f) != 5 || std::fread(Tcw, 4, 12, f) != 12) return 3;
    const size_t n = (size_t)hdr[0];
    std::vector<orbhip::KeyPoint> keys(n);
    std::vector<float> depth(n), world(3 * n);
    std::vector<uint8_t> flags(n);
    if (std::fread(keys.data(), sizeof(orbhip::KeyPoint), n, f) != n || std::fread(depth.data(), 4, n, f) != n ||
        std::fread(world.data(), 4, 3 * n, f) != 3 * n || std::fread(flags.data(), 1, n, f) != n) return 3;
    std::fclose(f);
    const int probe = std::atoi(argv[2]);
    try {
        orbhip::ORBmatcher matcher(0.9f, true);
        const std::vector<float> sf(8, 1.f);
        const orbhip_camera cam = orbhip::ORBmatcher::MakeCamera(cf[0], cf[1], cf[2], cf[3], 0.f, 0.f, 0.f, 1.f, 0.f, 1.f, sf, 0.f);
        int tracked = -1, other = -1;
        matcher.CountClosePoints(depth, flags, cf[4], tracked, other);      // on the caller's flags, before they change
        float X[3] = {0.f, 0.f, 0.f};
        const int32_t ok = matcher.UnprojectStereo(probe, cam, Tcw, keys, depth, X) ? 1 : 0;
        std::vector<int> order;
        std::vector<uint8_t> created;
        orbhip::ORBmatcher::SeedCounts c;
        const int made = matcher.SeedStereoPoints(cam, Tcw, keys, depth, cf[4], hdr[1], hdr[2], world, flags, order, created, &c);
        if (made != c.nCreated || (int)order.size() != c.nVisited || created.size() != n) return 4;
        FILE *o = std::fopen(argv[3], "wb");
        if (!o) return 3;
        const int32_t counts[3] = {c.nValid, c.nVisited, c.nCreated}, close[2] = {tracked, other};
        std::fwrite(world.data(), 4, world.size(), o);
        std::fwrite(flags.data(), 1, flags.size(), o);
        std::fwrite(counts, 4, 3, o);
        std::fwrite(order.data(), 4, order.size(), o);
        std::fwrite(created.data(), 1, created.size(), o);
        std::fwrite(close, 4, 2, o);
        std::fwrite(&ok, 4, 1, o);
        std::fwrite(X, 4, 3, o);
        std::fclose(o);
        std::printf("valid %d visited %d created %d close %d %d\n", c.nValid, c.nVisited, c.nCreated, tracked, other);
        // a bad mode and mismatched sizes: ORBHIP_E_ARG; no keypoints: nothing
        try { matcher.SeedStereoPoints(cam, Tcw, keys, depth, cf[4], 2, 1, world, flags, order, created); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        std::vector<float> shorter(depth.begin(), depth.end() - (n ? 1 : 0));
        if (n) {
            try { matcher.SeedStereoPoints(cam, Tcw, keys, shorter, cf[4], 1, 1, world, flags, order, created); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        }
        std::vector<orbhip::KeyPoint> nokeys;
        std::vector<float> nof;
        std::vector<uint8_t> nob;
        if (matcher.SeedStereoPoints(cam, Tcw, nokeys, nof, cf[4], 1, 1, nof, nob, order, created, &c) != 0 || !order.empty() ||
            !created.empty() || c.nValid != 0) return 4;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
