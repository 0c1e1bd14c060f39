"""The rectification part of the C++ host mirror (include/orbhip/ORBextractor.hpp: InitUndistortRectifyMap, SetRemap,
SetRemapTable, ExtractRemap), built with g++ against liborbhip.so: one raw EuRoC-calibrated stereo pair must give the
sequential restatement's maps and what the oracle gives on the sequentially rectified pair."""
import os
import subprocess

import numpy as np
import pytest

from helpers import assert_kps_equal
from seqref import rectify as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "EuRoC_stereo.yaml")


def _build(tmp_path, name="rectify_smoke"):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "orb_slam2_comment_amd")
    subprocess.run(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lorbhip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_cpp_rectify_mirror_compiles_against_the_header(tmp_path):
    _build(tmp_path)      # CPU-side: the mirror and the C ABI header are self-consistent C++11


@pytest.mark.gpu
def test_cpp_rectify_mirror_matches_seqref_and_oracle(tmp_path, oracle):
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd import settings as S
    from orb_slam2_comment_amd.synth import synth_raw_stereo
    exe = _build(tmp_path)
    W, H, nf = 752, 480, 1200
    calib = S.stereo_rectification(FIXTURE)
    raw = synth_raw_stereo(3, calib)
    cal = np.concatenate([np.concatenate([calib[s]["K"].ravel(), calib[s]["D"], calib[s]["R"].ravel(), calib[s]["P"][:, :3].ravel()])
                          for s in ("left", "right")])
    assert cal.size == 64
    cal.astype("<f8").tofile(str(tmp_path / "cal.bin"))
    raw[0].tofile(str(tmp_path / "l.raw"))
    raw[1].tofile(str(tmp_path / "r.raw"))
    mbf = np.float32(47.90639384423901)
    mb = np.float32(mbf / np.float32(435.2046959714599))
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe, str(tmp_path / "cal.bin"), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(H), str(W), str(nf),
                        repr(float(mbf)), repr(float(mb)), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(out, "rb").read()
    maps = {s: SR.init_undistort_rectify_map(calib[s]["K"], calib[s]["D"], calib[s]["R"], calib[s]["P"], (W, H)) for s in calib}
    off = 0
    for m in maps["left"]:
        assert np.array_equal(np.frombuffer(buf[off:off + 4 * W * H], np.float32).reshape(H, W), m)
        off += 4 * W * H
    rect = [SR.remap_linear(raw[0], *maps["left"]), SR.remap_linear(raw[1], *maps["right"])]
    ora = [oracle.OracleExtractor(nf, 1.2, 8, 20, 7), oracle.OracleExtractor(nf, 1.2, 8, 20, 7)]
    got, want = [], []
    for c in range(2):
        n = int(np.frombuffer(buf[off:off + 4], np.int32)[0]); off += 4
        kps = np.frombuffer(buf[off:off + 28 * n], pkg.KP_DTYPE); off += 28 * n
        desc = np.frombuffer(buf[off:off + 32 * n], np.uint8).reshape(n, 32); off += 32 * n
        okps, odesc = ora[c].extract(rect[c])
        assert n > 100
        assert_kps_equal(kps, okps)
        assert np.array_equal(desc, odesc)
        got.append((kps, desc))
        want.append((okps, odesc))
    nl = len(got[0][0])
    ur = np.frombuffer(buf[off:off + 4 * nl], np.float32); off += 4 * nl
    dp = np.frombuffer(buf[off:off + 4 * nl], np.float32)
    lv = [[np.ascontiguousarray(o.level_padded(l))[19:-19, 19:-19] for l in range(8)] for o in ora]
    t = ora[0].tables()
    on, our, odp = oracle.compute_stereo_matches(want[0][0], want[0][1], want[1][0], want[1][1], lv[0], lv[1], t["scale"],
                                                 t["inv_scale"], float(mbf), float(mb))
    assert on >= 100 and ("stereo %d" % on) in r.stdout
    assert np.array_equal(ur, our) and np.array_equal(dp, odp)
