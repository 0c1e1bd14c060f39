"""ORBmatcher::CreateNewMapPoints of the C++ host mirror (include/orbhip/ORBextractor.hpp), built with g++ against
liborbhip.so: what tests/cpp/triangulate_smoke.cpp dumps must be the Python result on the scene of
tests/test_triangulate_gpu.py, element for element."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name="triangulate_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_triangulate_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_triangulate_mirror_equals_the_python_result(tmp_path):
    import test_triangulate_gpu as TG
    exe = _build(tmp_path)
    e = TG.make_env(tmp_path)
    S, cam = e["S"], e["S"]["cam"]
    kf = TG.KF_INDEX
    got = e["run"].device(kf, False, False, False)
    K, n0 = len(kf), S["n"][TG.CUR]
    blob = np.array([K, len(S["sf"]), 0, 0], np.int32).tobytes()
    blob += np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf, cam.mb, TG.W, TG.H, cam.log_scale_factor], np.float32).tobytes()
    blob += S["sf"].tobytes() + S["sigma2"].tobytes()
    for f in [TG.CUR] + kf:
        blob += np.array([S["n"][f]], np.int32).tobytes() + S["T"][f].tobytes() + S["keys"][f].tobytes()
        blob += S["desc"][f].tobytes() + S["ur"][f].tobytes() + S["depth"][f].tobytes() + S["node"][f].tobytes()
        blob += S["hp"][f].tobytes()
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        fh.write(blob)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    o = 0
    m12 = np.frombuffer(raw, np.int32, K * n0, o).reshape(K, n0); o += K * n0 * 4
    nm = np.frombuffer(raw, np.int32, K, o); o += K * 4
    x3d = np.frombuffer(raw, np.uint32, K * n0 * 3, o).reshape(K, n0, 3); o += K * n0 * 12
    st = np.frombuffer(raw, np.uint8, K * n0, o).reshape(K, n0); o += K * n0
    sk = np.frombuffer(raw, np.uint8, K, o)
    assert np.array_equal(m12, got["m12"][:, :n0]) and np.array_equal(nm, got["nm"])
    assert np.array_equal(x3d, TG.bits(got["x3d"][:, :n0])) and np.array_equal(st, got["st"][:, :n0])
    assert np.array_equal(sk, got["sk"])
    assert ("created %d" % int((st == 0).sum())) in r.stdout and (st == 0).sum() > 50
