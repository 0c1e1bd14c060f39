"""The C++ mirror of Optimizer::BundleAdjustment (include/orbhip/Optimizer.hpp), built with g++ against liborbhip.so: what
tests/cpp/gba_smoke.cpp dumps for two cases of test_gba_cpu.py, through the host mirror and through BundleAdjustmentDevice, must
be the sequential restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_gba_cpu as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, f32, u8 = np.int32, np.float32, np.uint8


def _build(tmp_path, name="gba_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I",
                    "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_gba_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "pt_list", "newer_row"])
def test_cpp_gba_mirror_matches_seqref(tmp_path, name):
    exe = _build(tmp_path)
    b, ref = K.case(name), K.reference(name)
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
    rows, pcap = b["rows"], b["pcap"]
    status, rep = take(i32, 1), take(i32, 16)
    assert status[0] == ref["report"][0] and rep.tobytes() == ref["report"].tobytes()
    assert take(f32, rows * 12).tobytes() == ref["Tcw"].tobytes() and take(f32, pcap * 3).tobytes() == ref["world"].tobytes()
    TG, pG, km, pm = take(f32, rows * 12).reshape(rows, 12), take(f32, pcap * 3).reshape(pcap, 3), take(u8, rows), take(u8, pcap)
    assert km.tobytes() == ref["kf_mark"].tobytes() and pm.tobytes() == ref["pt_mark"].tobytes()
    assert TG[km == 1].tobytes() == ref["TcwGBA"][km == 1].tobytes() and pG[pm == 1].tobytes() == ref["posGBA"][pm == 1].tobytes()
    assert not TG[km == 0].any() and not pG[pm == 0].any()                    # the mirror hands out zeros where nothing was written
    cnt = int(take(i32, 1)[0])
    assert cnt == ref["report"][12] and take(i32, cnt).tolist() == ref["point_list"][:cnt].tolist()
    assert ("status %d vertices %d free %d points %d" % tuple(ref["report"][:4])) in r.stdout
    got = dict(Tcw=take(f32, rows * 12), world=take(f32, pcap * 3), TcwGBA=take(f32, rows * 12), posGBA=take(f32, pcap * 3),
               kf_mark=take(u8, rows), pt_mark=take(u8, pcap), point_list=take(i32, b["max_points"]), report=take(i32, 16))
    K.assert_same(got, ref, name + " through BundleAdjustmentDevice")
    syncs, launches = take(i32, 2)
    assert syncs == 1 + ref["report"][10] + 1 and launches > 3
    assert off == len(buf)
