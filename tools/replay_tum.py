#!/usr/bin/env python3
"""Front-end replay of a TUM RGB-D sequence, the counterpart of Examples/RGB-D/rgbd_tum.cc and
Examples/Monocular/mono_tum.cc for the part of ORB-SLAM2 this repository replaces.

With an association file (rgbd_tum.cc:142-167: `t rgb_file t depth_file` per line) every frame goes the way
Tracking::GrabImageRGBD and the RGB-D Frame constructor take it (src/Tracking.cc:207-231, src/Frame.cc:119-171): colour
-> grey on the device + ORBextractor::operator() (one call), Frame::UndistortKeyPoints with the settings file's
Camera.k1 / k2 / p1 / p2 / k3, and Frame::ComputeStereoFromRGBD on the raw depth image with DepthMapFactor and Camera.bf.
Without one the sequence is <sequence>/rgb.txt (mono_tum.cc:127-160) and every frame goes through
Tracking::GrabImageMonocular: the first through the 2*nFeatures initialisation extractor (src/Tracking.cc:258-260).
A one-channel file in the sequence goes through the grey entry, as the reference's channel test does (:172, :212).

Images arrive as cv::imread delivers them (B first, settings.read_color_image) and Camera.RGB of the settings file
chooses between the RGB and the BGR conversion (src/Tracking.cc:103-104, :174-183, :214-225), so the grey image is the
reference's for the same file and settings -- including TUM1-3.yaml's `Camera.RGB: 1` on imread's BGR data.

  python tools/replay_tum.py path/to/TUM1.yaml path/to/sequence [path/to/associations.txt] [--max-frames N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam2_comment_amd import ORBmatcher  # noqa: E402
from orb_slam2_comment_amd.matcher import SeedReplay  # noqa: E402
from orb_slam2_comment_amd.settings import (MONOCULAR, RGBD, camera_rgb, depth_map_factor, load_settings, load_tum_association,  # noqa: E402
                                            load_tum_rgb_list, make_extractors, read_color_image, read_depth_image)


def extract(e, im, rgb):
    return e(im) if im.ndim == 2 else e.extract_color(im, rgb)    # channels() == 1 takes neither cvtColor branch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings")
    ap.add_argument("sequence")
    ap.add_argument("association", nargs="?")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--seed", action="store_true", help="RGB-D: seed map points from the depths (StereoInitialization, "
                                                        "src/Tracking.cc:509-540, then the closest-points rule, :812-864)")
    args = ap.parse_args()
    st = load_settings(args.settings)
    if args.association:
        names, depths, stamps = load_tum_association(args.association)
        if not names:
            print("No images found in provided path.", file=sys.stderr)
            return 1
    else:
        names, stamps = load_tum_rgb_list(os.path.join(args.sequence, "rgb.txt"))
        depths = None
    if args.max_frames:
        names, stamps = names[:args.max_frames], stamps[:args.max_frames]
    ex = make_extractors(st, RGBD if depths is not None else MONOCULAR)
    print("Images in the sequence: %d" % len(names))
    matcher = ORBmatcher(0.9, True)
    cam = [float(st["Camera." + k]) for k in ("fx", "fy", "cx", "cy")]
    dist = [float(st.get("Camera." + k, 0.0)) for k in ("k1", "k2", "p1", "p2", "k3")]
    factor, mbf, rgb = depth_map_factor(st), float(st.get("Camera.bf", 0.0)), camera_rgb(st)
    seeder = SeedReplay(matcher, st) if args.seed and depths is not None else None
    times, counts, with_depth = [], [], []
    for ni, name in enumerate(names):
        im = read_color_image(os.path.join(args.sequence, name))
        if im.size == 0:
            print("Failed to load image at: %s" % name, file=sys.stderr)
            return 1
        imd = read_depth_image(os.path.join(args.sequence, depths[ni])) if depths is not None else None
        t1 = time.perf_counter()
        if depths is not None:
            kps, _ = extract(ex["left"], im, rgb)
            kun = matcher.UndistortKeyPoints(kps, cam[0], cam[1], cam[2], cam[3], dist)
            _, dp = matcher.ComputeStereoFromRGBDRaw(kps, kun, imd, factor, mbf)
            with_depth.append(int((dp > 0).sum()))
            if seeder is not None:
                seeder.frame(kun, dp)
        else:
            kps, _ = extract(ex["ini"] if ni == 0 else ex["left"], im, rgb)
        times.append(time.perf_counter() - t1)
        counts.append(len(kps))
    times.sort()
    n = len(times)
    print("-------\n")
    print("median tracking time: %.6f" % times[n // 2])
    print("mean tracking time: %.6f" % (sum(times) / n))
    print("mean keypoints: %.2f" % (sum(counts) / n))
    if with_depth:
        print("mean keypoints with depth: %.2f" % (sum(with_depth) / n))
    if seeder is not None:
        print(seeder.summary())
    return 0


if __name__ == "__main__":
    sys.exit(main())
