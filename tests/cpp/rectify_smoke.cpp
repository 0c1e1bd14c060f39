// One raw stereo pair through the C++ mirror (include/orbhip/ORBextractor.hpp) the way Examples/Stereo/stereo_euroc.cc uses
// OpenCV and the reference classes (:96-98 initUndistortRectifyMap, :136-137 remap, then Frame::ComputeStereoMatches):
// InitUndistortRectifyMap for both cameras, SetRemap on the two extractors, ExtractRemap, ComputeStereoMatches.  Reads a
// calibration of 2 x (K[9] D[5] R[9] P3x3[9]) doubles and two raw grey frames; writes the two maps of the left camera,
// "n" + keypoints + descriptors of both images and mvuRight + mvDepth as binary.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbhip/ORBextractor.hpp"

static bool read_all(const char *path, void *dst, size_t bytes)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(dst, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 10) { std::fprintf(stderr, "usage: rectify_smoke calib.bin left.raw right.raw rows cols nfeatures mbf mb out.bin\n"); return 2; }
    const int rows = std::atoi(argv[4]), cols = std::atoi(argv[5]), nf = std::atoi(argv[6]);
    const float mbf = (float)std::atof(argv[7]), mb = (float)std::atof(argv[8]);
    double cal[2][32];
    std::vector<uint8_t> img[2] = {std::vector<uint8_t>((size_t)rows * cols), std::vector<uint8_t>((size_t)rows * cols)};
    if (!read_all(argv[1], cal, sizeof(cal)) || !read_all(argv[2], img[0].data(), img[0].size()) ||
        !read_all(argv[3], img[1].data(), img[1].size())) return 3;
    try {
        orbhip::ORBextractor left(nf, 1.2f, 8, 20, 7), right(nf, 1.2f, 8, 20, 7);
        orbhip::ORBextractor *ext[2] = {&left, &right};
        orbhip::ORBmatcher matcher(0.9f, true);
        std::vector<float> m1[2], m2[2];
        std::vector<orbhip::KeyPoint> kps[2];
        std::vector<uint8_t> desc[2];
        for (int c = 0; c < 2; ++c) {
            const double *K = cal[c], *D = cal[c] + 9, *R = cal[c] + 14, *P = cal[c] + 23;
            orbhip::ORBextractor::InitUndistortRectifyMap(K, std::vector<double>(D, D + 5), R, P, cols, rows, m1[c], m2[c]);
            ext[c]->SetRemap(rows, cols, rows, cols, m1[c].data(), m2[c].data());
            orbhip::ImageView view{img[c].data(), rows, cols, (size_t)cols};
            ext[c]->ExtractRemap(view, kps[c], desc[c]);
        }
        std::vector<float> ur, dp;
        const int nm = matcher.ComputeStereoMatches(left, right, kps[0], desc[0], kps[1], desc[1], mbf, mb, ur, dp);
        FILE *o = std::fopen(argv[9], "wb");
        if (!o) return 3;
        std::fwrite(m1[0].data(), 4, m1[0].size(), o);
        std::fwrite(m2[0].data(), 4, m2[0].size(), o);
        for (int c = 0; c < 2; ++c) {
            int n = (int)kps[c].size();
            std::fwrite(&n, 4, 1, o);
            std::fwrite(kps[c].data(), sizeof(orbhip::KeyPoint), kps[c].size(), o);
            std::fwrite(desc[c].data(), 1, desc[c].size(), o);
        }
        std::fwrite(ur.data(), 4, ur.size(), o);
        std::fwrite(dp.data(), 4, dp.size(), o);
        std::fclose(o);
        std::printf("keypoints %d %d stereo %d\n", (int)kps[0].size(), (int)kps[1].size(), nm);
        // a frame of another size, no map, an out-of-range weight: ORBHIP_E_ARG; an empty image: nothing
        orbhip::ImageView shorter{img[0].data(), rows - 1, cols, (size_t)cols};
        try { left.ExtractRemap(shorter, kps[0], desc[0]); return 6; } catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        left.ClearRemap();
        orbhip::ImageView view{img[0].data(), rows, cols, (size_t)cols};
        try { left.ExtractRemap(view, kps[0], desc[0]); return 6; } catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        std::vector<int32_t> tab(ORBHIP_REMAP_TABLE_SIZE, 8192);
        right.SetRemapTable(tab.data());
        tab[5] = 65536;
        try { right.SetRemapTable(tab.data()); return 6; } catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        right.SetRemapTable(nullptr);
        orbhip::ImageView empty{nullptr, 0, 0, 0};
        right.ExtractRemap(empty, kps[1], desc[1]);
        if (!kps[1].empty() || !desc[1].empty()) return 4;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
