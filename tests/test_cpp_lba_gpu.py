"""The C++ mirror of Optimizer::LocalBundleAdjustment (include/orbhip/Optimizer.hpp), built with g++ against liborbhip.so:
what tests/cpp/lba_smoke.cpp dumps for scene S of test_lba_cpu.py, through the host mirror (with a clear stop flag) and
through LocalBundleAdjustmentDevice (null stop byte), must be the sequential restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_lba_cpu as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, f32 = np.int32, np.float32


def _build(tmp_path, name="lba_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I",
                    "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_lba_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_lba_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    b = K.case("S")
    inp, dump = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(K.pack(b, K.prefilled(b), None))
    r = subprocess.run([exe, inp, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf, off = open(dump, "rb").read(), 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype, count, off)
        off += a.nbytes
        return a
    ref = K.reference("stop_clear")
    raw = ref["raw"]
    status, rep = take(i32, 1), take(i32, 16)
    assert status[0] == raw["report"][0] and rep.tolist() == raw["report"]
    assert take(f32, b["rows"] * 12).tobytes() == ref["Tcw"].tobytes() and take(f32, b["pcap"] * 3).tobytes() == ref["world"].tobytes()
    for k in ("local_kf", "fixed_kf", "local_point"):
        cnt = int(take(i32, 1)[0])
        assert take(i32, cnt).tolist() == raw[k], k
    cnt = int(take(i32, 1)[0])
    assert take(i32, cnt).reshape(-1, 3).tolist() == raw["erase"]
    assert ("status 0 local %d fixed %d points %d erase %d" % (len(raw["local_kf"]), len(raw["fixed_kf"]), len(raw["local_point"]),
                                                               len(raw["erase"]))) in r.stdout
    ref = K.reference("S")
    got = dict(Tcw=take(f32, b["rows"] * 12), world=take(f32, b["pcap"] * 3), local_kf=take(i32, b["rows"]), fixed_kf=take(i32, b["rows"]),
               local_point=take(i32, b["max_points"]), erase=take(i32, b["max_edges"] * 3), report=take(i32, 16))
    K.assert_same(got, ref, "S through LocalBundleAdjustmentDevice")
    assert off == len(buf)
