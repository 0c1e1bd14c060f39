"""ORBmatcher::FuseBatch of the C++ host mirror (include/orbhip/ORBextractor.hpp), built with g++ against liborbhip.so:
the rows tests/cpp/fuse_batch_smoke.cpp dumps must be the oracle's keyframe_queries + search_best_in_window per key
frame, element for element."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name="fuse_batch_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_fuse_batch_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
@pytest.mark.parametrize("sim3_form,th", [(False, 3.0), (True, 4.0)])
def test_cpp_fuse_batch_mirror_matches_the_oracle(tmp_path, oracle, sim3_form, th):
    import orb_slam2_comment_amd as pkg
    from helpers import synth_frame
    import test_fuse_batch_gpu as FB
    O = oracle
    exe = _build(tmp_path)
    ext = pkg.ORBextractor(FB.NF, 1.2, 8, 20, 7)
    imgs = [synth_frame(41, FB.W, FB.H), synth_frame(41, FB.W, FB.H, shift_xy=(3, 1)), synth_frame(42, FB.W, FB.H)]
    kd = [ext(im) for im in imgs]
    kd.insert(1, (kd[0][0][:0], kd[0][1][:0]))                       # an empty key frame
    S = FB.build_scene(kd, ext.GetScaleFactors(), seed=17, kf_index=[0, 1, 2, 3])
    K, n, cam = len(kd), S["np"], S["cam"]
    ur = list(S["ur"])
    ur[3] = None                                                     # a monocular key frame among stereo ones
    rows = FB.oracle_rows(O, S, list(range(K)), S["flags"], th, sim3_form, ur=ur)
    assert sum((r[2] <= 50).sum() for r in rows) > 450
    blob = np.array([K, n, int(sim3_form), len(S["sf"])], np.int32).tobytes()
    blob += np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf, cam.mb, FB.W, FB.H, cam.log_scale_factor, th], np.float32).tobytes()
    blob += S["sf"].tobytes() + S["inv_sigma2"].tobytes()
    for f, (k, d) in enumerate(kd):
        blob += np.array([len(k), int(ur[f] is not None)], np.int32).tobytes() + np.ascontiguousarray(S["T"][f][:3, :4]).tobytes()
        blob += k.tobytes() + d.tobytes() + (ur[f].tobytes() if ur[f] is not None else b"")
    blob += S["X"].tobytes() + S["nrm"].tobytes() + S["max_d"].tobytes() + S["min_d"].tobytes() + S["pdesc"].tobytes()
    blob += S["flags"].tobytes()
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, np.int32).reshape(2, K, n)
    for k in range(K):
        assert np.array_equal(got[0, k], rows[k][1]) and np.array_equal(got[1, k], rows[k][2]), k
    assert ("within TH_LOW %d" % sum((r_[2] <= 50).sum() for r_ in rows)) in r.stdout
