"""The C++ mirror of Sim3Solver (include/orbhip/Sim3Solver.hpp), built with g++ against liborbhip.so: what
tests/cpp/sim3_smoke.cpp dumps for the hand-worked candidates of test_sim3_cpu.py, five iterations at a time until "no
more", must be the sequential restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_sim3_cpu as K
from seqref import sim3 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32, u8, f32 = np.int32, np.uint8, np.float32


def _build(tmp_path, name="sim3_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_sim3_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_sim3_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    sc, draws, mn, mx = K.case("hand")
    ref = K.reference("hand", 5, False)
    T = sc["T"]
    n1 = int(T["n"][sc["cur"]])
    inp, dump = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([sc["rows"], sc["cap"], sc["np"], sc["pcap"], sc["cur"], sc["C"], mn, mx, 0, S.MATCH_SLOTS, len(K.SIGMA2),
                          len(T["obs_kf"])], i32).tobytes())
        f.write(np.array([K.CAM[k] for k in ("fx", "fy", "cx", "cy")], f32).tobytes())
        for a in (T["slot_point"], T["n"], T["obs_start"], T["obs_kf"], T["obs_idx"], T["flags"], T["world"], T["Tcw"],
                  T["kps"]["octave"].astype(i32), sc["kf_index"], sc["m_slots"], K.SIGMA2, draws):
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
        # the calls of this candidate up to and including its first "no more"
        mine = []
        for call in ref:
            mine.append(call[c])
            if call[c][0][0] in (S.NO_MORE, S.TOO_FEW):
                break
        ncalls = int(take(i32, 1)[0])
        assert ncalls == len(mine), c
        reports, est, marks = take(i32, ncalls, 8), take(f32, ncalls, 13), take(u8, ncalls, n1)
        for t, (r_rep, r_sim3, r_inl, _) in enumerate(mine):
            assert reports[t].tolist() == r_rep.tolist(), (c, t)
            want = np.zeros(13, f32) if r_sim3 is None else r_sim3[:13]
            assert est[t].tobytes() == want.tobytes(), (c, t)
            assert np.array_equal(marks[t], r_inl), (c, t)
        returned = sum(1 for x in mine if x[0][0] == S.RETURNED)
        total_returned += returned
        assert ("candidate %d row %d N %d limit %d calls %d returned %d" % (c, sc["kf_index"][c], mine[0][0][1], mine[0][0][2],
                                                                            ncalls, returned)) in r.stdout
    assert off == len(buf) and total_returned > 10
