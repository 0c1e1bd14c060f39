"""The C++ mirror of Optimizer::PoseOptimization (include/orbhip/Optimizer.hpp), built with g++ against liborbhip.so: what
tests/cpp/poseopt_smoke.cpp dumps for scene A of test_poseopt_cpu.py with the DISCARD epilogue must be the sequential
restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_poseopt_cpu as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, u8, f32 = np.int32, np.uint8, np.float32


def _build(tmp_path, name="poseopt_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_poseopt_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_poseopt_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    b, ref = K.case("discard_f0"), K.reference("discard_f0")
    n, np_ = int(b["n"][0]), b["pcap"]
    inp, dump = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([n, np_, len(K.INV_SIGMA2), b["mode"], b["flags"], 1], i32).tobytes())
        f.write(np.array(K.CAM, f32).tobytes())
        for a in (b["kps"][0]["x"][:n], b["kps"][0]["y"][:n], b["kps"][0]["octave"][:n].astype(i32), b["u_right"][0][:n],
                  b["frame_point"][0][:n], b["world"][0], b["point_flags"][0], K.INV_SIGMA2, b["Tcw"][0]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, inp, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, off = open(dump, "rb").read(), 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype, count, off)
        off += a.nbytes
        return a
    ret, rep, tcw, out, fp, dis = take(i32, 1), take(i32, 8), take(f32, 12), take(u8, n), take(i32, n), take(i32, n)
    assert off == len(buf)
    assert ret[0] == ref["report"][0][3] and rep.tolist() == ref["report"][0].tolist()
    assert tcw.tobytes() == ref["Tcw"][0].tobytes()
    has = b["frame_point"][0][:n] >= 0
    assert (out[has] == ref["outlier"][0][:n][has]).all() and (out[~has] == 1).all()      # slots without a point keep the caller's
    assert (fp == ref["frame_point"][0][:n]).all() and (dis == ref["discarded"][0][:n]).all()
    assert (dis >= 0).sum() == 12
    assert ("edges 60 bad 12 returned 48 rounds 4 iterations %d" % rep[5]) in r.stdout
