"""The REFLECT_101 frames of pyramid levels >= 1 are not written by an extraction (orbhip_extractor.hip: kPyrFrame,
ensure_frames): the descriptor kernel reflects by index what a border keypoint's window overshoots, and the accessors
fill the frames on demand.  Everything here is bit for bit against the oracle, at the two smallest shapes whose level 7
still passes the 40-px minimum: 203x152 (one column chunk on every level) and 331x157 (level 1 is 276 px = 69 dwords:
two column chunks), 8 levels, scale 1.2, 300 features, with lazy level 0 on and off.

The product build writes 8 px of every frame eagerly, which keeps the descriptor kernel's windows inside written bytes;
the build without any eager frame (`make -C orb_slam2_comment_amd/csrc frame0`), in which that kernel reflects the
border windows of every level by index, runs the same cases in a child process: a process can load one build only."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from helpers import assert_kps_equal, synth_stereo  # noqa: E402

pytestmark = pytest.mark.gpu

NF, SCALE, NLEV, INI, MIN = 300, 1.2, 8, 20, 7
SHAPES = [(203, 152), (331, 157)]
SEED_A, SEED_B = 5, 6          # SEED_A: chosen on the CPU so that the oracle's keypoints meet the strip precondition below
KITTI_BF, KITTI_FX = 386.1448, 718.856


def textured(seed, W, H):
    """Blocky noise of four scales, full contrast in a band along the four edges and a quarter of it inside: corners at
    every pyramid level, the strongest ones (which the octree keeps) right up to the edges."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W), np.float64)
    for cell in (3, 7, 16, 37):
        g = rng.integers(0, 256, ((H + cell - 1) // cell, (W + cell - 1) // cell)).astype(np.float64)
        img += np.kron(g, np.ones((cell, cell)))[:H, :W]
    img /= 4.0
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(xx, W - 1 - xx), np.minimum(yy, H - 1 - yy))
    gain = np.where(d < 0.17 * min(W, H), 1.0, 0.25)
    return np.clip(128.0 + (img - 128.0) * gain, 0, 255).astype(np.uint8)


def high_contrast(seed, W, H):
    """0 / 255 blocks of 5 px: whatever it leaves in a plane's frame differs from any other image's frame"""
    g = np.random.default_rng(seed).integers(0, 2, ((H + 4) // 5, (W + 4) // 5)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(g, np.ones((5, 5), np.uint8))[:H, :W])


_REF = {}


def reference(O, seed, W, H):
    """The oracle's results for one image, computed once and shared (read-only) by the tests."""
    key = (seed, W, H)
    if key not in _REF:
        ora = O.OracleExtractor(NF, SCALE, NLEV, INI, MIN)
        img = textured(seed, W, H)
        kps, desc = ora.extract(img)
        r = dict(img=img, kps=kps, desc=desc, padded=[ora.level_padded(l).copy() for l in range(NLEV)],
                 blurred=[ora.level_blurred(l) for l in range(NLEV)], sizes=[ora.level_size(l) for l in range(NLEV)],
                 scale=ora.tables()["scale"].copy())
        for a in [kps, desc] + r["padded"] + r["blurred"]:   # the oracle blurs only the levels that have keypoints
            if a is not None:
                a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


@pytest.fixture(scope="module")
def mods(oracle):
    import orb_slam2_comment_amd as pkg
    return pkg, oracle


def make_ext(pkg, lazy):
    ext = pkg.ORBextractor(NF, SCALE, NLEV, INI, MIN)
    ext.set_lazy_level0(lazy)
    return ext


def border_strip_levels(r):
    """Levels on which at least one oracle keypoint lies in each of the four strips whose descriptor window leaves the
    level's interior (level coordinates: x < 21, x + 22 >= w, y < 21, y + 21 >= h)."""
    n = 0
    for l in range(NLEV):
        w, h = r["sizes"][l]
        k = r["kps"][r["kps"]["octave"] == l]
        x, y = np.rint(k["x"] / r["scale"][l]).astype(int), np.rint(k["y"] / r["scale"][l]).astype(int)
        assert np.array_equal((x * r["scale"][l]).astype(np.float32), k["x"])   # level coordinates recovered exactly
        n += bool((x < 21).any() and (x + 22 >= w).any() and (y < 21).any() and (y + 21 >= h).any())
    return n


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("W,H", SHAPES)
def test_keypoints_and_descriptors_of_border_keypoints(mods, W, H, lazy):
    pkg, O = mods
    r = reference(O, SEED_A, W, H)
    assert border_strip_levels(r) >= 4, "the test image has no keypoints in the border strips of four levels"
    ext = make_ext(pkg, lazy)
    for _ in range(2):                       # capture, then replay
        kps, desc = ext(r["img"])
        assert_kps_equal(kps, r["kps"])
        assert np.array_equal(desc, r["desc"])


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("W,H", SHAPES)
def test_padded_planes_after_lazy_fill(mods, W, H, lazy):
    pkg, O = mods
    r = reference(O, SEED_A, W, H)
    ext = make_ext(pkg, lazy)
    ext(r["img"])
    for l in range(NLEV):
        assert np.array_equal(ext.image_pyramid(l, with_border=True), r["padded"][l]), "padded level %d" % l
    assert sum(b is not None for b in r["blurred"]) >= 5
    for l in range(NLEV):
        if r["blurred"][l] is not None:
            assert np.array_equal(ext.blurred_level(l), r["blurred"][l]), "blurred level %d" % l
    # the blurred planes first: their kernel reads every level's frame
    ext2 = make_ext(pkg, lazy)
    ext2(r["img"])
    for l in range(NLEV):
        if r["blurred"][l] is not None:
            assert np.array_equal(ext2.blurred_level(l), r["blurred"][l]), "blurred level %d before any plane download" % l
    for l in range(NLEV):
        assert np.array_equal(ext2.image_pyramid(l, with_border=False), r["padded"][l][19:-19, 19:-19]), "level %d" % l


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("W,H", SHAPES)
def test_no_stale_frames(mods, W, H, lazy):
    pkg, O = mods
    a, b = reference(O, SEED_A, W, H), reference(O, SEED_B, W, H)
    ext = make_ext(pkg, lazy)
    ext(a["img"])
    assert np.array_equal(ext.image_pyramid(3, with_border=True), a["padded"][3])
    ext(b["img"])
    assert np.array_equal(ext.image_pyramid(3, with_border=True), b["padded"][3])
    # and without the first download
    ext(a["img"])
    ext(b["img"])
    assert np.array_equal(ext.image_pyramid(3, with_border=True), b["padded"][3])


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("W,H", SHAPES)
def test_frame_bytes_do_not_leak_into_results(mods, W, H, lazy):
    """The planes of the first extraction are the poison: nothing touches an accessor in between, so the frames of the
    second image's levels still hold what the first one (and its accessors) left there."""
    pkg, O = mods
    b = reference(O, SEED_B, W, H)
    ext = make_ext(pkg, lazy)
    ext(high_contrast(9, W, H))
    ext.image_pyramid(NLEV - 1, with_border=True)      # every level's frame now holds the first image's reflection
    ext(high_contrast(10, W, H))
    kps, desc = ext(b["img"])
    assert_kps_equal(kps, b["kps"])
    assert np.array_equal(desc, b["desc"])


@pytest.mark.parametrize("lazy", [True, False])
def test_stereo_without_an_accessor_in_between(mods, lazy):
    pkg, O = mods
    W, H = SHAPES[0]
    left, right = synth_stereo(1, W, H)
    eL, eR = make_ext(pkg, lazy), make_ext(pkg, lazy)
    kl, dl = eL(left)
    kr, dr = eR(right)
    mbf = np.float32(KITTI_BF)
    mb = np.float32(mbf / np.float32(KITTI_FX))
    n, ur, dp = pkg.ORBmatcher().ComputeStereoMatches(eL, eR, kl, dl, kr, dr, float(mbf), float(mb))
    oL, oR = O.OracleExtractor(NF, SCALE, NLEV, INI, MIN), O.OracleExtractor(NF, SCALE, NLEV, INI, MIN)
    okl, odl = oL.extract(left)
    okr, odr = oR.extract(right)
    assert_kps_equal(kl, okl)
    assert_kps_equal(kr, okr)
    lv_l = [np.ascontiguousarray(oL.level_padded(l))[19:-19, 19:-19] for l in range(NLEV)]
    lv_r = [np.ascontiguousarray(oR.level_padded(l))[19:-19, 19:-19] for l in range(NLEV)]
    t = oL.tables()
    on, our, odp = O.compute_stereo_matches(okl, odl, okr, odr, lv_l, lv_r, t["scale"], t["inv_scale"], float(mbf), float(mb))
    assert on >= 50, "the test pair gives too few stereo matches"
    assert n == on
    assert np.array_equal(ur, our) and np.array_equal(dp, odp)


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("W,H", SHAPES)
def test_device_batch_fills_the_frames_of_every_slot(mods, W, H, lazy):
    import torch
    pkg, O = mods
    refs = [reference(O, SEED_A, W, H), reference(O, SEED_B, W, H), reference(O, SEED_B + 1, W, H)]
    B = len(refs)
    d_img = torch.from_numpy(np.stack([r["img"] for r in refs])).cuda()
    ext = make_ext(pkg, lazy)
    cap = ext.capacity(H, W)
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_s = torch.zeros(B, dtype=torch.int32, device="cuda")
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(), d_s.data_ptr(),
                             stride=W, frame_stride=W * H)
    ext.sync()
    assert int(d_s.abs().sum().item()) == 0
    n = d_n.cpu().numpy()
    kps = d_k.cpu().numpy().view(np.uint8).reshape(B, cap, 28).view(pkg.capi.KP_DTYPE).reshape(B, cap)
    desc = d_d.cpu().numpy()
    assert np.array_equal(ext.image_pyramid(5, frame=2, with_border=True), refs[2]["padded"][5])
    for b in range(B):
        assert_kps_equal(kps[b, :n[b]], refs[b]["kps"], "frame %d" % b)
        assert np.array_equal(desc[b, :n[b]], refs[b]["desc"])
        assert np.array_equal(ext.image_pyramid(1, frame=b, with_border=True), refs[b]["padded"][1])


def test_build_without_eager_frames():
    """Child process on the frame-less build: every case above."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:], file=sys.stderr)
    assert r.returncode == 0, "child failed with status %d" % r.returncode
    assert "no eager frames: all cases equal the oracle" in r.stdout


def _child():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), "frame0"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    sys.path.insert(0, ROOT)
    from orb_slam2_comment_amd import capi
    capi.use_library(os.path.join(ROOT, "tools", "_dev", "liborbhip_frame0.so"))
    import orb_slam2_comment_amd as pkg
    from oracle import oracle_py as O
    mods = (pkg, O)
    for lazy in (True, False):
        for W, H in SHAPES:
            test_keypoints_and_descriptors_of_border_keypoints(mods, W, H, lazy)
            test_padded_planes_after_lazy_fill(mods, W, H, lazy)
            test_no_stale_frames(mods, W, H, lazy)
            test_frame_bytes_do_not_leak_into_results(mods, W, H, lazy)
            test_device_batch_fills_the_frames_of_every_slot(mods, W, H, lazy)
        test_stereo_without_an_accessor_in_between(mods, lazy)
    print("no eager frames: all cases equal the oracle")


if __name__ == "__main__":
    _child()
