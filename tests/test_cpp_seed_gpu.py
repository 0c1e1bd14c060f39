"""The seeding part of the C++ host mirror (include/orbhip/ORBextractor.hpp: SeedStereoPoints, UnprojectStereo,
CountClosePoints), built with g++ against liborbhip.so: what tests/cpp/seed_smoke.cpp dumps must be the sequential
restatement's answer bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from seqref import seed as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name="seed_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_seed_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
@pytest.mark.parametrize("mode,cf,n,th", [(SS.SEED_CLOSEST, 1, 900, 12.0), (SS.SEED_CLOSEST, 3, 300, 40.0), (SS.SEED_ALL, 3, 700, 12.0)])
def test_cpp_seed_mirror_matches_seqref(tmp_path, mode, cf, n, th):
    import orb_slam2_comment_amd as pkg
    exe = _build(tmp_path)
    rng = np.random.default_rng(11 * n + mode)
    K = (718.856, 718.856, 607.1928, 185.2157)
    a = rng.normal(0, 0.5, 3)
    ang = np.linalg.norm(a)
    k = a / ang
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Tcw = np.zeros((3, 4), np.float32)
    Tcw[:, :3] = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx).astype(np.float32)
    Tcw[:, 3] = rng.normal(0, 2, 3).astype(np.float32)
    keys = np.zeros(n, pkg.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, 1241, n).astype(np.float32), rng.uniform(0, 376, n).astype(np.float32)
    depth = rng.uniform(1.0, 60.0, n).astype(np.float32)
    depth[rng.integers(0, n, n // 5)] = -1.0
    depth[rng.integers(0, n, n // 8)] = depth[rng.integers(0, n, n // 8)]
    world = rng.normal(0, 5, (n, 3)).astype(np.float32)
    flags = rng.integers(0, 4, n).astype(np.uint8)
    probe = int(np.nonzero(depth > 0)[0][7])
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([n, mode, cf], np.int32).tobytes() + np.array(K + (th,), np.float32).tobytes() + Tcw.tobytes()
                + keys.tobytes() + depth.tobytes() + world.tobytes() + flags.tobytes())
    r = subprocess.run([exe, inp, str(probe), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    xy = np.stack([keys["x"], keys["y"]], 1)
    rw, rf, ro, rc, rcounts = SS.seed_stereo_points(K, Tcw, xy, depth, th, mode, cf, world, flags)
    close = SS.count_close_points(depth, flags, th)
    assert ("valid %d visited %d created %d close %d %d" % (rcounts + close)) in r.stdout
    assert rcounts[2] > 50 and rcounts[1] > rcounts[2] - (mode == SS.SEED_ALL)
    buf, off = open(out, "rb").read(), 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype, count, off)
        off += a.nbytes
        return a
    assert np.array_equal(take(np.int32, 3 * n), rw.view(np.int32).ravel())
    assert np.array_equal(take(np.uint8, n), rf)
    assert tuple(take(np.int32, 3)) == rcounts
    assert np.array_equal(take(np.int32, rcounts[1]), ro)
    assert np.array_equal(take(np.uint8, n), rc)
    assert tuple(take(np.int32, 2)) == close
    assert take(np.int32, 1)[0] == 1
    X = SS.unproject_stereo(xy[probe, 0], xy[probe, 1], depth[probe], K, Tcw)
    assert np.array_equal(take(np.int32, 3), np.array(X, np.float32).view(np.int32))
    assert off == len(buf)
