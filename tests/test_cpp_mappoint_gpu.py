"""The map-point refresh of the C++ host mirror (include/orbhip/ORBextractor.hpp: UpdateMapPoints), built with g++ against
liborbhip.so: what tests/cpp/mappoint_smoke.cpp dumps for the random scene of test_mappoint_cpu.py must be the sequential
restatement's answer bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import test_mappoint_cpu as MC
import test_seqref_projection_cpu as PC
from seqref import mappoint as MP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name="mappoint_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_mappoint_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
@pytest.mark.parametrize("what,with_bad", [(MC.BOTH, True), (MP.UPDATE_NORMAL_DEPTH, False)])
def test_cpp_mappoint_mirror_matches_seqref(tmp_path, what, with_bad):
    exe = _build(tmp_path)
    S = MC.scene_and_reference(MC.BOTH)[0]
    n = MC.NPTS
    bad = S["kf_bad"] if with_bad else None
    init = MC.sentinels(n)
    ref = MP.update_map_points(S["scam"], what, S["T"], S["keys"], S["desc"], bad, S["obs_start"], S["obs_kf"], S["obs_idx"],
                               S["ref_obs"], S["world"], S["flags"], *init)
    nobs = int(S["obs_start"][-1])
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([MC.ROWS, MC.NKEYS, n, nobs, what, len(PC.SF), int(with_bad)], np.int32).tobytes())
        f.write(np.asarray(PC.SF, np.float32).tobytes())
        f.write(np.stack([np.asarray(t, np.float32)[:3].reshape(12) for t in S["T"]]).tobytes())
        f.write(S["kf_bad"].tobytes())
        for r in range(MC.ROWS):
            f.write(S["keys"][r].tobytes() + S["desc"][r].tobytes())
        for a in (S["obs_start"], S["obs_kf"][:nobs], S["obs_idx"][:nobs], S["ref_obs"], S["world"], S["flags"]) + init:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, inp, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    updated = int((ref[5] == MP.UPDATED).sum())
    assert ("points %d updated %d" % (n, updated)) in r.stdout and updated > 200
    buf, off = open(out, "rb").read(), 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype, count, off)
        off += a.nbytes
        return a
    assert np.array_equal(take(np.uint8, 32 * n), ref[0].ravel())
    assert np.array_equal(take(np.int32, 3 * n), ref[1].view(np.int32).ravel())
    assert np.array_equal(take(np.int32, n), ref[2].view(np.int32))
    assert np.array_equal(take(np.int32, n), ref[3].view(np.int32))
    assert np.array_equal(take(np.int32, n), ref[4])
    assert np.array_equal(take(np.uint8, n), ref[5])
    assert off == len(buf)
