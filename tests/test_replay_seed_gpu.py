"""tools/replay_kitti.py --stereo --seed on a small generated stereo sequence: the counts it prints are the sequential
restatement's (tests/seqref/seed.py) on the oracle's depths, and without --seed the tool prints what it always printed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import synth_stereo
from seqref import seed as SS
from test_settings_cpu import YAML, _png

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replay_kitti_stereo_seed(tmp_path, oracle):
    from orb_slam2_comment_amd import settings as S
    O = oracle
    seq = tmp_path / "00"
    (seq / "image_0").mkdir(parents=True)
    (seq / "image_1").mkdir(parents=True)
    nfr, Wd, Hd, nf = 3, 640, 360, 800
    pairs = [synth_stereo(5, Wd, Hd, shift_xy=(2 * i, 0)) for i in range(nfr)]
    (seq / "times.txt").write_text("".join("%e\n" % (0.1 * i) for i in range(nfr)))
    for i, (l, r) in enumerate(pairs):
        _png(str(seq / "image_0" / ("%06d.png" % i)), l, [0, 1, 2])
        _png(str(seq / "image_1" / ("%06d.png" % i)), r, [2, 0, 1])
    yaml = tmp_path / "KITTI.yaml"
    # ThDepth 35 gives mThDepth = 18.8 m; the scene's disparities of 2 .. 80 px are depths of 4.8 .. 193 m, both sides of it
    yaml.write_text(YAML.replace("nFeatures: 2000", "nFeatures: %d" % nf))
    tool = os.path.join(ROOT, "tools", "replay_kitti.py")
    plain = subprocess.run([sys.executable, tool, str(yaml), str(seq), "--stereo"], capture_output=True, text=True)
    seeded = subprocess.run([sys.executable, tool, str(yaml), str(seq), "--stereo", "--seed"], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert seeded.returncode == 0, seeded.stderr

    def shape(text):      # every line with its numbers after "time:" removed (the only run-dependent part)
        return [ln.split("time:")[0] for ln in text.splitlines()]
    want_plain = ["Images in the sequence: %d" % nfr, "-------", "", "median extraction + stereo ", "mean extraction + stereo "]
    got = shape(plain.stdout)
    assert got[:5] == want_plain and len(got) == 7
    assert got[5].startswith("mean keypoints per left frame: ") and got[6].startswith("mean stereo matches per pair: ")
    assert "New map" not in plain.stdout and "close points" not in plain.stdout
    # --seed adds exactly two lines and changes none of the others
    sgot = shape(seeded.stdout)
    assert len(sgot) == 9 and sgot[1].startswith("New map created with ") and sgot[8].startswith("mean close points per frame: ")
    assert [sgot[0]] + sgot[2:8] == got
    # the counts against seqref on the ORACLE's keypoints and depths
    st = S.load_settings(str(yaml))
    mbf = np.float32(st["Camera.bf"]); mb = np.float32(mbf / np.float32(st["Camera.fx"]))
    th = SS.th_depth(st["Camera.bf"], st["ThDepth"], st["Camera.fx"])
    K = tuple(float(st["Camera." + k]) for k in ("fx", "fy", "cx", "cy"))
    T = np.eye(4, dtype=np.float32)[:3]
    want = []
    for i, (l, rr) in enumerate(pairs):
        oL, oR = O.OracleExtractor(nf, 1.2, 8, 20, 7), O.OracleExtractor(nf, 1.2, 8, 20, 7)
        kl, dl = oL.extract(l)
        kr, dr = oR.extract(rr)
        lv_l = [np.ascontiguousarray(oL.level_padded(k))[19:-19, 19:-19] for k in range(8)]
        lv_r = [np.ascontiguousarray(oR.level_padded(k))[19:-19, 19:-19] for k in range(8)]
        t = oL.tables()
        _, _, dp = O.compute_stereo_matches(kl, dl, kr, dr, lv_l, lv_r, t["scale"], t["inv_scale"], float(mbf), float(mb))
        n = len(kl)
        assert n > 500
        xy = np.stack([kl["x"], kl["y"]], 1)
        mode, cf = (SS.SEED_ALL, 3) if i == 0 else (SS.SEED_CLOSEST, 1)
        want.append(SS.seed_stereo_points(K, T, xy, dp, th, mode, cf, np.zeros((n, 3), np.float32), np.zeros(n, np.uint8))[4])
    assert ("New map created with %d points" % want[0][2]) in seeded.stdout and want[0][2] > 30
    got_mean = float(seeded.stdout.split("mean close points per frame:")[1].split()[0])
    assert abs(got_mean - sum(w[2] for w in want[1:]) / (nfr - 1)) < 0.006
    assert all(w[2] >= min(w[0], 101) for w in want[1:])
