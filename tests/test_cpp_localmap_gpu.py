"""The local-map call of the C++ host mirror (include/orbhip/ORBextractor.hpp: UpdateLocalMap), built with g++ against
liborbhip.so: what tests/cpp/localmap_smoke.cpp dumps for scene A of test_localmap_cpu.py must be the sequential
restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_localmap_cpu as LC
from seqref import localmap as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A


def _build(tmp_path, name="localmap_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_localmap_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_localmap_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    S, R = LC.scene_and_reference("A")
    frames, rows, cap, n_pts, pcap = S["frames"], S["rows"], S["cap"], S["np"], S["pcap"]
    nchild, nobs = int(S["child_start"][-1]), int(S["obs_start"][-1])
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([frames, rows, cap, n_pts, pcap, nchild, nobs], np.int32).tobytes())
        for a in (S["slot_point"], S["n"], S["kf_bad"], S["covis"], S["child_start"], S["child"][:nchild], S["parent"],
                  S["obs_start"], S["obs_kf"][:nobs], S["flags"], S["world"], S["normal"], S["max_dist"], S["min_dist"],
                  S["point_desc"], S["frame_point"], S["frame_n"], S["local_kf"], S["n_local_kf"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, inp, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for fr in range(frames):
        rep = LC.report(R, fr)
        assert ("frame %d status %d local key frames %d local points %d" %
                (fr, rep["status"], rep["n_local_kf"], rep["n_local_points"])) in r.stdout
    buf, off = open(out, "rb").read(), 0

    def take(dtype, *shape):
        nonlocal off
        a = np.frombuffer(buf, dtype, int(np.prod(shape)), off).reshape(shape)
        off += a.nbytes
        return a
    i32, u8 = np.int32, np.uint8
    got = dict(frame_point=take(i32, frames, cap), local_kf=take(i32, frames, rows), n_local_kf=take(i32, frames),
               votes=take(i32, frames, rows), local_point=take(i32, frames, pcap), world_l=take(u8, frames, pcap, 12),
               normal_l=take(u8, frames, pcap, 12), max_dist_l=take(u8, frames, pcap, 4), min_dist_l=take(u8, frames, pcap, 4),
               desc_l=take(u8, frames, pcap, 32), flags_l=take(u8, frames, pcap), np_l=take(i32, frames), taken=take(u8, frames, cap),
               report=take(i32, frames, 8))
    assert off == len(buf)
    assert np.array_equal(got["frame_point"], R["frame_point"]) and np.array_equal(got["votes"], R["votes"])
    assert np.array_equal(got["report"], R["report"]) and np.array_equal(got["np_l"], R["report"][:, 6])
    for fr in range(frames):
        nk, npt, nf = len(R["local_kf"][fr]), len(R["local_point"][fr]), int(S["frame_n"][fr])
        assert npt > 250
        assert np.array_equal(got["local_kf"][fr, :nk], R["local_kf"][fr]) and (got["local_kf"][fr, nk:] == -1).all()
        assert np.array_equal(got["local_point"][fr, :npt], R["local_point"][fr])
        w, nrm, mx, mn, d = LM.gather(S, R["local_point"][fr])
        for k, ref in (("world_l", w), ("normal_l", nrm), ("max_dist_l", mx), ("min_dist_l", mn), ("desc_l", d),
                       ("flags_l", R["flags_l"][fr])):
            assert np.array_equal(got[k][fr, :npt].reshape(npt, -1), np.ascontiguousarray(ref).view(u8).reshape(npt, -1)), k
            assert (got[k][fr, npt:] == FILL).all(), k
        assert (got["local_point"][fr, npt:].view(u8) == FILL).all()
        assert np.array_equal(got["taken"][fr, :nf], R["taken"][fr, :nf]) and (got["taken"][fr, nf:] == FILL).all()
