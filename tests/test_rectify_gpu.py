"""Stereo rectification on the GPU, bit for bit: the rectified plane of orbhip_extract_remap* against the sequential
restatement (tests/seqref/rectify.py) for the EuRoC calibration, a border calibration and unequal sizes; the extraction
and ComputeStereoMatches behind it against the oracle and the grey entries on the seqref-rectified images; handles reused
across entries, maps replaced and removed, a custom weight table; tools/replay_euroc.py end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_kps_equal, synth_frame
from seqref import rectify as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "EuRoC_stereo.yaml")
W, H = 752, 480


@pytest.fixture(scope="module")
def mods():
    import orb_slam2_comment_amd as pkg
    from oracle import oracle_py as O
    return pkg, O


@pytest.fixture(scope="module")
def calib():
    from orb_slam2_comment_amd import settings as S
    return S.stereo_rectification(FIXTURE)


def scaled(c, w, h):
    """The calibration of the same camera read out at w x h: K and P scaled per axis."""
    s = np.diag([w / c["width"], h / c["height"], 1.0])
    return dict(c, K=s @ c["K"], P=s @ c["P"], width=w, height=h)


def border_calibration(c):
    """LEFT with the signs of k1 and k2 flipped: the rectified image reaches far outside the source."""
    D = c["D"].copy()
    D[0], D[1] = -D[0], -D[1]
    return dict(c, D=D)


def maps_of(c, size=None):
    return SR.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], size or (c["width"], c["height"]))


@pytest.fixture(scope="module")
def all_maps(calib):
    out = {"left": (maps_of(calib["left"]), (H, W)), "right": (maps_of(calib["right"]), (H, W)),
           "border": (maps_of(border_calibration(calib["left"])), (H, W)),
           "small": (maps_of(border_calibration(scaled(calib["left"], 321, 243))), (243, 321)),
           # source size != destination size: a 640x400 rectified image cut from the 752x480 camera ...
           "crop": (maps_of(calib["right"], (640, 400)), (H, W)),
           # ... and a 323x241 one (row tail of 3 pixels) from a 400x300 read-out of the border calibration
           "tail": (maps_of(border_calibration(scaled(calib["left"], 400, 300)), (323, 241)), (300, 400))}
    return out


def strided(frames, pad):
    """[B, H, W] -> (flat uint8 buffer that ends with the last pixel, row stride, frame stride, view on the frames)."""
    B, h, w = frames.shape
    stride = w + pad
    fstride = h * stride + (3 if pad else 0)
    buf = np.full((B - 1) * fstride + (h - 1) * stride + w, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, frames.shape, (fstride, stride, 1))
    view[...] = frames
    return buf, stride, fstride, view


def run_device(ext, pkg, frames, pad=0, dst=None):
    """extract_remap_batch_device on a buffer that ends with the last pixel; returns per-frame (keypoints, descriptors)."""
    import torch
    B, h, w = frames.shape
    buf, stride, fstride, _ = strided(frames, pad)
    drows, dcols = dst or (h, w)
    cap = ext.capacity(drows, dcols)
    d_img = torch.from_numpy(buf).cuda()
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_s = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_remap_batch_device(d_img.data_ptr(), B, h, w, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(), d_s.data_ptr(),
                                   stride=stride, frame_stride=fstride)
    ext.sync()
    assert np.all(d_s.cpu().numpy() == 0)
    n = d_n.cpu().numpy()
    k, d = d_k.cpu().numpy(), d_d.cpu().numpy()
    return [(k[b, :n[b]].copy().view(pkg.KP_DTYPE).reshape(-1), d[b, :n[b]].copy()) for b in range(B)]


def source_frame(seed, src_shape):
    return synth_frame(seed, src_shape[1], src_shape[0])


# ---- the inputs of the border cases are what the issue says they are -------------------------------------------------
@pytest.mark.parametrize("name", ["border", "small"])
def test_border_calibration_mixes_inside_and_outside(all_maps, name):
    (m1, m2), src = all_maps[name]
    cnt = SR.tap_classes(m1, m2, src)
    inside, outside, mixed = float((cnt == 4).mean()), float((cnt == 0).mean()), int(((cnt > 0) & (cnt < 4)).sum())
    print(name, inside, outside, mixed)
    assert inside >= 0.5 and outside >= 0.1 and mixed >= 500


# ---- the rectified plane ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pad", [("left", 0), ("right", 0), ("border", 0), ("small", 5), ("crop", 0), ("tail", 3)])
def test_rectified_plane_equals_seqref(mods, all_maps, name, pad):
    pkg, O = mods
    (m1, m2), src = all_maps[name]
    img, other = source_frame(41, src), source_frame(42, src)
    want, want2 = SR.remap_linear(img, m1, m2), SR.remap_linear(other, m1, m2)
    assert len(np.unique(want)) > 50 and want.shape == m1.shape
    _, _, _, view = strided(img[None], pad)
    for lazy in (False, True):
        ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
        ext.set_lazy_level0(lazy)
        ext.set_remap(m1, m2, src)
        ext.extract_remap(view[0])                                        # host entry, strided rows
        assert np.array_equal(ext.image_pyramid(0), want), "host lazy=%s" % lazy
        ext.extract_remap_batch(np.stack([other, img]))                   # host batch
        assert np.array_equal(ext.image_pyramid(0, frame=0), want2)
        assert np.array_equal(ext.image_pyramid(0, frame=1), want)
        run_device(ext, pkg, np.stack([img, other]), pad, m1.shape)       # device entry, buffer ends with the last pixel
        assert np.array_equal(ext.image_pyramid(0, frame=0), want), "device lazy=%s" % lazy
        assert np.array_equal(ext.image_pyramid(0, frame=1), want2)
        full = ext.image_pyramid(0, frame=1, with_border=True)            # the reflected border comes from the rectified plane
        assert np.array_equal(full, np.pad(want2, 19, mode="reflect"))


@pytest.mark.parametrize("name,B", [("left", 1), ("right", 8), ("border", 8), ("left", 136), ("small", 139), ("tail", 9)])
def test_device_batches(mods, all_maps, name, B):
    """Batches of 1, 8 and >= 136 frames (17 and more per frame group of k_remap, and group sizes that differ)."""
    pkg, O = mods
    (m1, m2), src = all_maps[name]
    uniq = [source_frame(50 + s, src) for s in range(min(B, 8))]
    want = [SR.remap_linear(u, m1, m2) for u in uniq]
    frames = np.stack([uniq[(5 * b) % len(uniq)] for b in range(B)])
    for lazy in (False, True):
        ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
        ext.set_lazy_level0(lazy)
        ext.set_remap(m1, m2, src)
        res = run_device(ext, pkg, frames, 0, m1.shape)
        first = {}
        for b in range(B):
            u = (5 * b) % len(uniq)
            assert np.array_equal(ext.image_pyramid(0, frame=b), want[u]), "frame %d lazy=%s" % (b, lazy)
            if u in first:
                assert_kps_equal(res[b][0], res[first[u]][0], "frame %d" % b)
                assert np.array_equal(res[b][1], res[first[u]][1])
            first.setdefault(u, b)


# ---- extraction behind the remap -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nf", [("left", 1000), ("right", 2000), ("border", 1000), ("small", 1000)])
def test_extract_remap_equals_oracle_and_grey_entry(mods, all_maps, name, nf):
    pkg, O = mods
    (m1, m2), src = all_maps[name]
    img = source_frame(61, src)
    rect = SR.remap_linear(img, m1, m2)
    ok, od = O.OracleExtractor(nf, 1.2, 8, 20, 7).extract(rect)
    gk, gd = pkg.ORBextractor(nf, 1.2, 8, 20, 7)(rect)
    assert len(ok) > 100
    for lazy in (False, True):
        ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7)
        ext.set_lazy_level0(lazy)
        ext.set_remap(m1, m2, src)
        k, d = ext.extract_remap(img)
        assert_kps_equal(k, ok, "host vs oracle")
        assert np.array_equal(d, od)
        assert_kps_equal(k, gk, "host vs grey entry")
        assert np.array_equal(d, gd)
        (k, d), = run_device(ext, pkg, img[None], 0, m1.shape)
        assert_kps_equal(k, ok, "device vs oracle")
        assert np.array_equal(d, od)


# ---- stereo ----------------------------------------------------------------------------------------------------------
def test_stereo_matches_behind_the_remap(mods, calib, all_maps):
    """Two handles with the LEFT / RIGHT maps + ComputeStereoMatches == two grey handles fed the seqref-rectified pair
    == the oracle on that pair (>= 100 stereo matches)."""
    pkg, O = mods
    from orb_slam2_comment_amd.synth import synth_raw_stereo
    raw_l, raw_r = synth_raw_stereo(3, calib)
    (l1, l2), _ = all_maps["left"]
    (r1, r2), _ = all_maps["right"]
    rect_l, rect_r = SR.remap_linear(raw_l, l1, l2), SR.remap_linear(raw_r, r1, r2)
    nf = 1200
    mbf = np.float32(47.90639384423901)
    mb = np.float32(mbf / np.float32(435.2046959714599))
    oL, oR = O.OracleExtractor(nf, 1.2, 8, 20, 7), O.OracleExtractor(nf, 1.2, 8, 20, 7)
    okl, odl = oL.extract(rect_l)
    okr, odr = oR.extract(rect_r)
    lv_l = [np.ascontiguousarray(oL.level_padded(l))[19:-19, 19:-19] for l in range(8)]
    lv_r = [np.ascontiguousarray(oR.level_padded(l))[19:-19, 19:-19] for l in range(8)]
    t = oL.tables()
    on, our, odp = O.compute_stereo_matches(okl, odl, okr, odr, lv_l, lv_r, t["scale"], t["inv_scale"], float(mbf), float(mb))
    assert on >= 100
    gL, gR = pkg.ORBextractor(nf, 1.2, 8, 20, 7), pkg.ORBextractor(nf, 1.2, 8, 20, 7)
    gkl, gdl = gL(rect_l)
    gkr, gdr = gR(rect_r)
    m = pkg.ORBmatcher()
    gn, gur, gdp = m.ComputeStereoMatches(gL, gR, gkl, gdl, gkr, gdr, float(mbf), float(mb))
    for lazy in (False, True):
        eL, eR = pkg.ORBextractor(nf, 1.2, 8, 20, 7), pkg.ORBextractor(nf, 1.2, 8, 20, 7)
        for e, mm in ((eL, (l1, l2)), (eR, (r1, r2))):
            e.set_lazy_level0(lazy)
            e.set_remap(*mm)
        kl, dl = eL.extract_remap(raw_l)
        kr, dr = eR.extract_remap(raw_r)
        assert_kps_equal(kl, okl, "left")
        assert_kps_equal(kr, okr, "right")
        n, ur, dp = m.ComputeStereoMatches(eL, eR, kl, dl, kr, dr, float(mbf), float(mb))
        assert n == gn == on
        assert np.array_equal(ur, gur) and np.array_equal(dp, gdp)
        assert np.array_equal(ur, our) and np.array_equal(dp, odp)


# ---- handles over time -----------------------------------------------------------------------------------------------
def test_handle_reused_across_entries_maps_and_sizes(mods, all_maps):
    pkg, O = mods
    from orb_slam2_comment_amd.synth import synth_color_frame
    from seqref import color as SC
    ext = pkg.ORBextractor(800, 1.2, 8, 20, 7)
    (l1, l2), src = all_maps["left"]
    (b1, b2), _ = all_maps["border"]
    (s1, s2), ssrc = all_maps["small"]
    (c1, c2), _ = all_maps["crop"]
    img, small = source_frame(71, src), source_frame(72, ssrc)
    fresh = lambda: pkg.ORBextractor(800, 1.2, 8, 20, 7)   # noqa: E731

    def same(got, rect):
        wk, wd = fresh()(rect)
        assert_kps_equal(got[0], wk)
        assert np.array_equal(got[1], wd)
        assert np.array_equal(ext.image_pyramid(0), rect)

    with pytest.raises(pkg.OrbHipError) as err:                            # no map installed yet
        ext.extract_remap(img)
    assert err.value.code == pkg.capi.E_ARG
    ext.set_remap(l1, l2)
    same(ext.extract_remap(img), SR.remap_linear(img, l1, l2))
    same(ext(img), img)                                                    # the grey entry ignores the map
    col = synth_color_frame(73, 640, 480)
    same(ext.extract_color(col, True), SC.cvt_gray(col, True))             # colour entry, another size, shares the grey frames
    same(ext.extract_remap(img), SR.remap_linear(img, l1, l2))             # the map survived both
    ext.set_remap(b1, b2)                                                  # replaced, same sizes
    same(ext.extract_remap(img), SR.remap_linear(img, b1, b2))
    ext.set_remap(s1, s2)                                                  # replaced, other sizes
    same(ext.extract_remap(small), SR.remap_linear(small, s1, s2))
    with pytest.raises(pkg.OrbHipError) as err:                            # a frame of the old size
        ext.extract_remap(img)
    assert err.value.code == pkg.capi.E_ARG
    ext.set_remap(c1, c2, src)                                             # destination smaller than the source
    same(ext.extract_remap(img), SR.remap_linear(img, c1, c2))
    same(ext.extract_remap_batch(np.stack([img, img]))[1], SR.remap_linear(img, c1, c2))
    ext.set_remap(None)                                                    # removed
    with pytest.raises(pkg.OrbHipError) as err:
        ext.extract_remap(img)
    assert err.value.code == pkg.capi.E_ARG
    same(ext(img), img)


def test_argument_checks_with_a_live_handle(mods, all_maps):
    import ctypes as C
    pkg, O = mods
    capi = pkg.capi
    L, p = capi.lib(), capi.ptr
    ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
    (m1, m2), src = all_maps["left"]
    h = ext._h
    assert L.orbhip_extractor_set_remap(h, H, W, H, W, p(m1), None) == capi.E_ARG       # one map only
    for dims in ((0, W, H, W), (H, 0, H, W), (H, W, 0, W), (H, W, H, 0), (H, W, 40000, W), (H, W, H, 40000)):
        assert L.orbhip_extractor_set_remap(h, *dims, p(m1), p(m2)) == capi.E_ARG
    ext.set_remap(m1, m2)
    cap = ext.capacity(H, W)
    img = source_frame(5, src)
    kps, desc = np.zeros(cap, capi.KP_DTYPE), np.zeros((cap, 32), np.uint8)
    n = C.c_int(-7)
    for ch in (3, 4, 0, 2):                                                # colour (or nonsense) through the remap entries
        assert L.orbhip_extract_remap(h, p(img), H, W, ch, W * max(ch, 1), p(kps), p(desc), cap, C.byref(n)) == capi.E_ARG
    assert L.orbhip_extract_remap(h, p(img), H, W, 1, W - 1, p(kps), p(desc), cap, C.byref(n)) == capi.E_ARG   # short stride
    assert L.orbhip_extract_remap(h, p(img), H, W - 1, 1, W, p(kps), p(desc), cap, C.byref(n)) == capi.E_ARG   # not the map's size
    assert L.orbhip_extract_remap(h, p(img), H, W, 1, W, p(kps), p(desc), 0, C.byref(n)) == capi.E_ARG
    assert L.orbhip_extract_remap(h, None, H, W, 1, W, p(kps), p(desc), cap, C.byref(n)) == capi.OK and n.value == 0   # empty image
    k, d = ext.extract_remap(np.zeros((0, 0), np.uint8))
    assert len(k) == 0 and d.shape == (0, 32)
    bad = np.zeros(capi.REMAP_TABLE_SIZE, np.int32)
    bad[17] = 65536
    assert L.orbhip_extractor_set_remap_table(h, p(bad)) == capi.E_ARG
    bad[17] = -1
    assert L.orbhip_extractor_set_remap_table(h, p(bad)) == capi.E_ARG
    k, _ = ext.extract_remap(img)                                          # the handle still works, with the default table
    assert np.array_equal(ext.image_pyramid(0), SR.remap_linear(img, m1, m2)) and len(k) > 100


def test_custom_weight_table(mods, all_maps):
    """The table is data: a nearest-neighbour-like table, one that saturates, and back to the default."""
    pkg, O = mods
    (m1, m2), src = all_maps["border"]
    img = source_frame(81, src)
    ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
    ext.set_remap(m1, m2)
    rng = np.random.default_rng(7)
    tabs = [np.tile(np.array([32768, 0, 0, 0]), (1024, 1)), SR.bilinear_table() * 2 - (SR.bilinear_table() * 2 > 65535),
            rng.integers(0, 65536, (1024, 4))]
    default = SR.remap_linear(img, m1, m2)
    for t in tabs:
        ext.set_remap_table(t)
        ext.extract_remap(img)
        want = SR.remap_linear(img, m1, m2, t)
        assert not np.array_equal(want, default)
        assert np.array_equal(ext.image_pyramid(0), want)
    ext.set_remap_table(None)
    ext.extract_remap(img)
    assert np.array_equal(ext.image_pyramid(0), default)


def test_nan_and_far_outside_maps(mods):
    pkg, O = mods
    w, h = 220, 160
    img = synth_frame(9, w, h)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    m1, m2 = xs * np.float32(0.97) + np.float32(1.3), ys * np.float32(1.02) - np.float32(0.7)
    m1[10:20, 30:50] = np.nan
    m2[40:45, 5:9] = np.nan
    m1[50:60, 60:70] = 3e9
    m2[70:80, 80:90] = -3e9
    m1[90, :] = -1.0 + 1 / 64
    m2[:, 100] = h - 1 + 1 / 32
    want = SR.remap_linear(img, m1, m2)
    assert np.array_equal(want, SR.remap_linear_scalar(img, m1, m2))
    assert np.all(want[10:20, 30:50] == 0) and np.all(want[50:60, 60:70] == 0)
    ext = pkg.ORBextractor(300, 1.2, 8, 20, 7)
    ext.set_remap(m1, m2)
    ext.extract_remap(img)
    assert np.array_equal(ext.image_pyramid(0), want)


# ---- the replay tool -------------------------------------------------------------------------------------------------
def test_replay_euroc_end_to_end(mods, calib, tmp_path):
    pkg, O = mods
    from orb_slam2_comment_amd.synth import synth_raw_stereo
    from test_color_cpu import write_png
    ldir, rdir = tmp_path / "cam0", tmp_path / "cam1"
    ldir.mkdir()
    rdir.mkdir()
    stamps = ["1403636579763555584", "1403636579813555456", "1403636579863555584"]
    pairs = []
    for i, s in enumerate(stamps):
        l, r = synth_raw_stereo(90 + i, calib)
        pairs.append((l, r))
        write_png(str(ldir / (s + ".png")), l, W, H, 8, 0, 1, (0, 1, 2, 3, 4))
        write_png(str(rdir / (s + ".png")), r, W, H, 8, 0, 1, (0,))
    (tmp_path / "times.txt").write_text("\n".join(stamps[:2]) + "\n\n" + stamps[2] + "\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay_euroc.py"), FIXTURE, str(ldir), str(rdir),
                          str(tmp_path / "times.txt")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Images in the sequence: 3" in out.stdout
    assert re.search(r"median tracking time: \d+\.\d+", out.stdout) and re.search(r"mean tracking time: \d+\.\d+", out.stdout)
    # the counts the tool prints are those of the seqref-rectified pairs through the grey entries
    maps = {s: SR.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], (W, H)) for s, c in calib.items()}
    nk, ns = [], []
    mbf = float(np.float32(47.90639384423901))
    mb = float(np.float32(47.90639384423901) / np.float32(435.2046959714599))
    eL, eR, m = pkg.ORBextractor(1200, 1.2, 8, 20, 7), pkg.ORBextractor(1200, 1.2, 8, 20, 7), pkg.ORBmatcher()
    for l, r in pairs:
        kl, dl = eL(SR.remap_linear(l, *maps["left"]))
        kr, dr = eR(SR.remap_linear(r, *maps["right"]))
        n, _, _ = m.ComputeStereoMatches(eL, eR, kl, dl, kr, dr, mbf, mb)
        nk.append(len(kl))
        ns.append(n)
    assert min(ns) >= 100
    assert "mean keypoints: %.2f" % (sum(nk) / 3) in out.stdout
    assert "mean stereo matches: %.2f" % (sum(ns) / 3) in out.stdout
