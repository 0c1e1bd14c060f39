"""The covisibility calls of the C++ host mirror (include/orbhip/ORBextractor.hpp: UpdateConnections, CovisibleTargets), built
with g++ against liborbhip.so: what tests/cpp/covisibility_smoke.cpp dumps for the 65-row scene of test_covisibility_cpu.py
must be the sequential restatement's answer byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import test_covisibility_cpu as CC
from seqref import covisibility as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A
NN, NN2 = 10, 5


def _build(tmp_path, name="covisibility_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_covisibility_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_covisibility_mirror_matches_seqref(tmp_path):
    exe = _build(tmp_path)
    S = CC.scene_and_reference(("random", 65))
    T, state, upd, out = S["T"], S["state"], S["upd"], S["out"]
    rows, nobs, U = T["rows"], int(T["obs_start"][-1]), len(upd)
    bad = np.zeros(rows, np.uint8)
    bad[[3, 9]] = 1
    cur = np.arange(24, dtype=np.int32)
    ref = CV.covisible_targets(CV.Graph.from_dense(out), cur, NN, NN2, bad)
    inp, dump = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([rows, T["cap"], T["np"], T["pcap"], nobs, U, S["id0"], len(cur), NN, NN2], np.int32).tobytes())
        for a in ([T["slot_point"], T["n"], T["obs_start"], T["obs_kf"][:nobs], T["flags"]] + [state[k] for k in CC.STATE_KEYS] +
                  [upd, bad, cur]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, inp, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for u in range(U):
        assert ("entry %d row %d status %d ordered %d parent %d" % (u, upd[u], S["report"][u, 0], S["report"][u, 2], S["report"][u, 5])) \
            in r.stdout
    buf, off = open(dump, "rb").read(), 0

    def take(dtype, *shape):
        nonlocal off
        a = np.frombuffer(buf, dtype, int(np.prod(shape)), off).reshape(shape)
        off += a.nbytes
        return a
    i32, u8 = np.int32, np.uint8
    got = dict(conn_w=take(i32, rows, rows), ord_kf=take(i32, rows, rows), ord_w=take(i32, rows, rows), n_ord=take(i32, rows),
               covis=take(i32, rows, 10), first_conn=take(u8, rows), parent=take(i32, rows), report=take(i32, U, 8))
    targets, counts = take(i32, len(cur), NN * (1 + NN2)), take(i32, len(cur))
    assert off == len(buf)
    for k in CC.STATE_KEYS:
        assert np.array_equal(got[k], out[k]), k
    assert np.array_equal(got["report"], S["report"])
    assert counts.tolist() == [len(l) for l in ref] and max(counts) > NN
    for q in range(len(cur)):
        assert targets[q, :counts[q]].tolist() == ref[q] and (targets[q, counts[q]:] == -1).all()
