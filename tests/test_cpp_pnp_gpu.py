"""The C++ mirror of PnPsolver (include/orbhip/PnPsolver.hpp), built with g++ against liborbhip.so: what
tests/cpp/pnp_smoke.cpp dumps for the "plain" scene of test_pnp_cpu.py, five iterations at a time until bNoMore, must be the
sequential restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_pnp_cpu as K
from seqref import pnp as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, u8, f32 = np.int32, np.uint8, np.float32


def _build(tmp_path, name="pnp_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_pnp_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_pnp_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    sc, draws, prm, more = K.case("plain")
    ref = K.reference("plain")
    n, pcap = sc["n"], len(sc["map"]["flags"])
    inp, dump = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([n, pcap, pcap, sc["C"], len(K.SIGMA2), draws.shape[1], prm["min_inliers"], prm["max_its"], len(ref)],
                         i32).tobytes())
        f.write(np.array([K.CAM[k] for k in ("fx", "fy", "cx", "cy")] + [prm["epsilon"], prm["th2"]], f32).tobytes())
        for a in (sc["kps"]["x"], sc["kps"]["y"], sc["kps"]["octave"].astype(i32), sc["map"]["flags"], sc["map"]["world"],
                  sc["m_points"][:, :n], K.SIGMA2, draws):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, inp, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, off = open(dump, "rb").read(), 0

    def take(dtype, *shape):
        nonlocal off
        a = np.frombuffer(buf, dtype, int(np.prod(shape)), off).reshape(shape)
        off += a.nbytes
        return a
    total_returned = 0
    for c in range(sc["C"]):
        mine = []                                                               # the calls up to and including the first bNoMore
        for call in ref:
            mine.append(call[c])
            if call[c][0][0] != P.REFINED:
                break
        ncalls = int(take(i32, 1)[0])
        assert ncalls == len(mine), c
        reports, poses, marks = take(i32, ncalls, 8), take(f32, ncalls, 12), take(u8, ncalls, n)
        for t, (r_rep, r_tcw, r_inl, _) in enumerate(mine):
            assert reports[t].tolist() == r_rep.tolist(), (c, t)
            assert poses[t].tobytes() == (np.zeros(12, f32) if r_tcw is None else r_tcw).tobytes(), (c, t)
            assert np.array_equal(marks[t], np.zeros(n, u8) if r_inl is None else r_inl), (c, t)
        returned = sum(1 for x in mine if x[1] is not None)
        total_returned += returned
        assert ("candidate %d N %d limit %d calls %d returned %d" % (c, mine[0][0][1], mine[0][0][2], ncalls, returned)) in r.stdout
    assert off == len(buf) and total_returned >= sc["C"]
