"""The C++ mirror of Optimizer::OptimizeEssentialGraph (include/orbhip/Optimizer.hpp), built with g++ against liborbhip.so: what
tests/cpp/essgraph_smoke.cpp dumps for scene H of test_essgraph_cpu.py, through the host mirror and through
OptimizeEssentialGraphDevice, must be the sequential restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_essgraph_cpu as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, f32, f64 = np.int32, np.float32, np.float64


def _build(tmp_path, name="essgraph_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I",
                    "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_essgraph_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_essgraph_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    b, ref = K.case("H"), K.reference("H")
    inp, dump = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(K.pack(b, K.prefilled(b)))
    r = subprocess.run([exe, inp, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, off = open(dump, "rb").read(), 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype, count, off)
        off += a.nbytes
        return a
    raw = ref["raw"]
    status, rep = take(i32, 1), take(i32, 16)
    assert status[0] == raw["report"][0] and rep.tolist() == raw["report"]
    assert take(f32, b["rows"] * 12).tobytes() == ref["Tcw"].tobytes() and take(f32, b["pcap"] * 3).tobytes() == ref["world"].tobytes()
    cnt = int(take(i32, 1)[0])
    assert take(i32, cnt).tolist() == raw["point_list"]
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1], f64)
    for k in ("Scw", "Swc"):
        got = take(f64, b["rows"] * 8).reshape(-1, 8)
        for row in range(b["rows"]):
            want = np.array(raw[k][row], f64) if row in raw[k] else ident      # a bad row keeps the identity the mirror starts from
            assert got[row].tobytes() == want.tobytes(), (k, row)
    assert ("status 0 vertices %d edges %d points %d" % (raw["report"][1], sum(raw["report"][2:6]), len(raw["point_list"]))) in r.stdout
    got = dict(Tcw=take(f32, b["rows"] * 12), world=take(f32, b["pcap"] * 3), point_list=take(i32, b["pcap"]), Scw=take(f64, b["rows"] * 8),
               Swc=take(f64, b["rows"] * 8), report=take(i32, 16))
    K.assert_same(got, ref, "H through OptimizeEssentialGraphDevice")
    assert off == len(buf)
