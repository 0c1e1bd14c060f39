// One RGB-D frame through the C++ mirror (include/orbhip/ORBextractor.hpp) the way Tracking::GrabImageRGBD and the RGB-D
// Frame constructor use the reference classes (src/Tracking.cc:207-231, src/Frame.cc:119-171): colour extraction,
// UndistortKeyPoints, ComputeStereoFromRGBD on the raw 16-bit depth image.  Reads raw colour bytes and raw little-endian
// uint16 depth; writes "n" + keypoints + descriptors + mvuRight + mvDepth as binary.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbhip/ORBextractor.hpp"

int main(int argc, char **argv)
{
    if (argc < 10) { std::fprintf(stderr, "usage: color_smoke color.raw depth.raw rows cols channels rgb nfeatures depth_factor out.bin\n"); return 2; }
    const int rows = std::atoi(argv[3]), cols = std::atoi(argv[4]), ch = std::atoi(argv[5]), rgb = std::atoi(argv[6]), nf = std::atoi(argv[7]);
    const float factor = (float)std::atof(argv[8]);
    std::vector<uint8_t> img((size_t)rows * cols * ch);
    std::vector<uint16_t> depth((size_t)rows * cols);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(img.data(), 1, img.size(), f) != img.size()) return 3;
    std::fclose(f);
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(depth.data(), 2, depth.size(), f) != depth.size()) return 3;
    std::fclose(f);
    try {
        orbhip::ORBextractor ext(nf, 1.2f, 8, 20, 7);
        orbhip::ORBmatcher matcher(0.9f, true);
        std::vector<orbhip::KeyPoint> kps;
        std::vector<uint8_t> desc;
        orbhip::ColorImageView view{img.data(), rows, cols, ch, (size_t)cols * ch};
        ext.ExtractColor(view, rgb != 0, kps, desc);
        const float dist[5] = {0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f};
        std::vector<orbhip::KeyPoint> un = matcher.UndistortKeyPoints(kps, 517.306408f, 516.469215f, 318.643040f, 255.313989f, dist);
        std::vector<float> ur, dp;
        matcher.ComputeStereoFromRGBD(kps, un, depth.data(), ORBHIP_DEPTH_U16, rows, cols, cols, factor, 40.0f, ur, dp);
        FILE *o = std::fopen(argv[9], "wb");
        if (!o) return 3;
        int n = (int)kps.size();
        std::fwrite(&n, 4, 1, o);
        std::fwrite(kps.data(), sizeof(orbhip::KeyPoint), kps.size(), o);
        std::fwrite(desc.data(), 1, desc.size(), o);
        std::fwrite(ur.data(), 4, ur.size(), o);
        std::fwrite(dp.data(), 4, dp.size(), o);
        std::fclose(o);
        std::printf("keypoints %d\n", n);
        const int32_t w15[3] = {9798, 19235, 3735}, bad[3] = {65536, 0, 0};
        ext.SetGrayWeights(w15, 15);
        try { ext.SetGrayWeights(bad, 14); return 6; } catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        orbhip::ColorImageView empty{nullptr, 0, 0, 3, 0};
        ext.ExtractColor(empty, true, kps, desc);
        if (!kps.empty() || !desc.empty()) return 4;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
