"""The colour / RGB-D part of the C++ host mirror (include/orbhip/ORBextractor.hpp: ColorImageView, ExtractColor,
SetGrayWeights, the raw-depth ComputeStereoFromRGBD), built with g++ against liborbhip.so: one RGB-D frame must give
what the oracle gives on the sequentially converted grey and depth images."""
import os
import subprocess

import numpy as np
import pytest

from helpers import assert_kps_equal
from seqref import color as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name="color_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_color_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rgb", [(3, True), (4, False)])
def test_cpp_color_mirror_matches_oracle(tmp_path, oracle, ch, rgb):
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.synth import synth_color_frame, synth_depth
    exe = _build(tmp_path)
    W, H, nf = 640, 480, 800
    img = synth_color_frame(5, W, H, channels=ch, rgb=rgb)
    dep = synth_depth(5, W, H)
    craw, draw, out = str(tmp_path / "c.raw"), str(tmp_path / "d.raw"), str(tmp_path / "out.bin")
    img.tofile(craw)
    dep.astype("<u2").tofile(draw)
    factor = SC.depth_map_factor(5000.0)
    r = subprocess.run([exe, craw, draw, str(H), str(W), str(ch), str(int(rgb)), str(nf), repr(float(factor)), out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(out, "rb").read()
    n = int(np.frombuffer(buf[:4], np.int32)[0])
    off = 4
    kps = np.frombuffer(buf[off:off + 28 * n], pkg.KP_DTYPE); off += 28 * n
    desc = np.frombuffer(buf[off:off + 32 * n], np.uint8).reshape(n, 32); off += 32 * n
    ur = np.frombuffer(buf[off:off + 4 * n], np.float32); off += 4 * n
    dp = np.frombuffer(buf[off:off + 4 * n], np.float32)
    gray, fdepth = SC.grab_image_rgbd(img, dep, rgb, factor)
    okps, odesc = oracle.OracleExtractor(nf, 1.2, 8, 20, 7).extract(gray)
    assert n > 100
    assert_kps_equal(kps, okps)
    assert np.array_equal(desc, odesc)
    kun = oracle.undistort_keypoints(okps, 517.306408, 516.469215, 318.643040, 255.313989,
                                     (0.262383, -0.953104, -0.005358, 0.002628, 1.163314))
    our, odp = oracle.compute_stereo_from_rgbd(okps, kun, fdepth, np.float32(40.0))
    assert np.array_equal(ur, our) and np.array_equal(dp, odp)
    assert (dp > 0).sum() > 50 and (dp < 0).sum() > 5
