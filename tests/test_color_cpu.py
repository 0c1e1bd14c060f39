"""Colour / RGB-D input without a device: the sequential restatement of the grey and depth conversions
(tests/seqref/color.py) against hand-worked answers, the settings / list / image readers of the TUM examples, the
synthetic colour and depth generators, and the argument checks of the new C-ABI entries."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from seqref import color as SC

f32 = np.float32
W15 = (9798, 19235, 3735)   # a 15-bit table (sums to 1 << 15), used as the "other OpenCV build" of set_gray_weights


def _px(r, g, b, a=None):
    return np.array([[[r, g, b] if a is None else [r, g, b, a]]], np.uint8)


# ---- seqref.cvt_gray: hand-worked answers ---------------------------------------------------------------------------
def test_primaries():
    # (255*4899 + 8192) >> 14 = 1257437 >> 14 = 76; (255*9617 + 8192) >> 14 = 150; (255*1868 + 8192) >> 14 = 29
    for px, want in (((255, 0, 0), 76), ((0, 255, 0), 150), ((0, 0, 255), 29)):
        assert SC.cvt_gray(_px(*px), True)[0, 0] == want
        assert SC.cvt_gray(_px(*px[::-1]), False)[0, 0] == want        # the same colour stored B first
    assert SC.cvt_gray(_px(255, 0, 0), False)[0, 0] == 29              # byte 0 read as B
    assert SC.cvt_gray(_px(0, 0, 255), False)[0, 0] == 76


def test_grey_is_a_fixed_point():
    assert sum(SC.GRAY_WEIGHTS) == 1 << SC.GRAY_SHIFT
    img = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for rgb in (True, False):
        assert np.array_equal(SC.cvt_gray(img, rgb)[0], np.arange(256))


def test_alpha_is_ignored():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    other = img.copy()
    other[..., 3] = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    for rgb in (True, False):
        assert np.array_equal(SC.cvt_gray(img, rgb), SC.cvt_gray(img[..., :3], rgb))
        assert np.array_equal(SC.cvt_gray(img, rgb), SC.cvt_gray(other, rgb))


def test_14_and_15_bit_tables_differ_somewhere():
    found = None
    for r in range(256):
        for g in range(0, 256, 5):
            a = (r * 4899 + g * 9617 + 8192) >> 14
            b = (r * 9798 + g * 19235 + 16384) >> 15
            if a != b:
                found = (r, g, 0, a, b)
                break
        if found:
            break
    assert found is not None
    r, g, b_, a, b = found
    assert SC.cvt_gray(_px(r, g, b_), True)[0, 0] == a
    assert SC.cvt_gray(_px(r, g, b_), True, W15, 15)[0, 0] == b


def test_saturation():
    # weights summing to 2 << 14: white would be 510
    assert SC.cvt_gray(_px(255, 255, 255), True, (16384, 8192, 8192), 14)[0, 0] == 255
    assert SC.cvt_gray(_px(100, 100, 100), True, (16384, 8192, 8192), 14)[0, 0] == 200
    assert SC.cvt_gray(_px(255, 255, 255), True, (65535, 65535, 65535), 1)[0, 0] == 255


# ---- depth ---------------------------------------------------------------------------------------------------------
def test_depth_map_factor():
    assert SC.depth_map_factor(5000) == f32(1) / f32(5000)
    assert SC.depth_map_factor(5000).dtype == np.float32
    for v in (0, 1e-6, 1):
        assert SC.depth_map_factor(v) == f32(1)


def test_depth_to_float():
    rng = np.random.default_rng(2)
    fl = rng.uniform(0, 9, (6, 5)).astype(np.float32)
    assert SC.depth_to_float(fl, f32(1)) is fl
    assert np.array_equal(SC.depth_to_float(fl, f32(1) + f32(5e-6)), fl)          # inside the 1e-5 band: untouched
    half = SC.depth_to_float(fl, f32(0.5))
    assert half.dtype == np.float32 and np.array_equal(half, fl * f32(0.5))
    u = rng.integers(0, 65536, (6, 5)).astype(np.uint16)
    one = SC.depth_to_float(u, f32(1))                                            # type != CV_32F: always converted
    assert one.dtype == np.float32 and np.array_equal(one, u.astype(np.float32))
    k = SC.depth_map_factor(5000)
    conv = SC.depth_to_float(u, k)
    assert conv.dtype == np.float32 and np.array_equal(conv, u.astype(np.float32) * k)
    assert conv[0, 0] == f32(f32(int(u[0, 0])) * k)


def test_grab_image_rgbd():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (4, 6, 3), dtype=np.uint8)
    d = rng.integers(0, 65536, (4, 6)).astype(np.uint16)
    g, fd = SC.grab_image_rgbd(img, d, True, SC.depth_map_factor(5000))
    assert np.array_equal(g, SC.cvt_gray(img, True)) and fd.dtype == np.float32
    grey = img[..., 0].copy()
    assert SC.grab_image_rgbd(grey, d, True, f32(1))[0] is grey


# ---- settings, lists, readers ----------------------------------------------------------------------------------------
TUM_YAML = """%YAML:1.0
# TUM1-like
Camera.fx: 517.306408
Camera.fy: 516.469215
Camera.cx: 318.643040
Camera.cy: 255.313989
Camera.k1: 0.262383
Camera.k2: -0.953104
Camera.p1: -0.005358
Camera.p2: 0.002628
Camera.k3: 1.163314
Camera.width: 640
Camera.height: 480
Camera.fps: 30.0
Camera.bf: 40.0
Camera.RGB: 1
ThDepth: 40.0
DepthMapFactor: 5000.0
ORBextractor.nFeatures: 1000
ORBextractor.scaleFactor: 1.2
ORBextractor.nLevels: 8
ORBextractor.iniThFAST: 20
ORBextractor.minThFAST: 7
"""


def test_tum_settings(tmp_path):
    from orb_slam2_comment_amd import settings as S
    p = tmp_path / "TUM1.yaml"
    p.write_text(TUM_YAML)
    st = S.load_settings(str(p))
    assert S.camera_rgb(st) is True
    f = S.depth_map_factor(st)
    assert f.dtype == np.float32 and f == f32(1) / f32(5000) and f == SC.depth_map_factor(5000.0)
    assert S.extractor_args(st) == (1000, 1.2, 8, 20, 7)
    assert st["Camera.bf"] == 40.0 and st["Camera.k3"] == 1.163314
    del st["Camera.RGB"], st["DepthMapFactor"]
    assert S.camera_rgb(st) is False and S.depth_map_factor(st) == f32(1)
    for v in (0, 1e-6, 1):
        assert S.depth_map_factor({"DepthMapFactor": v}) == f32(1)
    assert S.RGBD == 2


def test_tum_lists(tmp_path):
    from orb_slam2_comment_amd import settings as S
    a = tmp_path / "assoc.txt"
    a.write_text("1305031102.175304 rgb/1305031102.175304.png 1305031102.160407 depth/1305031102.160407.png\n"
                 "\n"
                 "1305031102.211214 rgb/b.png 1305031102.226738 depth/b.png\n\n")
    rgb, dep, t = S.load_tum_association(str(a))
    assert rgb == ["rgb/1305031102.175304.png", "rgb/b.png"] and dep == ["depth/1305031102.160407.png", "depth/b.png"]
    assert t == [1305031102.175304, 1305031102.211214]
    r = tmp_path / "rgb.txt"
    r.write_text("# color images\n# file: 'x.bag'\n# timestamp filename\n1.5 rgb/1.5.png\n\n2.5 rgb/2.5.png\n")
    names, t = S.load_tum_rgb_list(str(r))
    assert names == ["rgb/1.5.png", "rgb/2.5.png"] and t == [1.5, 2.5]


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def write_png(path, rows_bytes, w, h, depth, ctype, bpp, filters):
    """rows_bytes: uint8 [h, w*bpp] (PNG byte order); row y is encoded with filter type filters[y % len(filters)]."""
    raw = bytearray()
    prev = [0] * (w * bpp)
    for y in range(h):
        cur = rows_bytes[y].tolist()
        ft = filters[y % len(filters)]
        raw.append(ft)
        for x, v in enumerate(cur):
            a = cur[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
            raw.append((v - pred) & 255)
        prev = cur

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))
    data = zlib.compress(bytes(raw))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
                + chunk(b"IDAT", data[:len(data) // 2]) + chunk(b"IDAT", data[len(data) // 2:]) + chunk(b"IEND", b""))


@pytest.mark.parametrize("filters", [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)])
def test_png_round_trip(tmp_path, filters):
    from orb_slam2_comment_amd import settings as S
    from orb_slam2_comment_amd.synth import synth_color_frame, synth_depth
    W, H = 37, 11
    rgb = synth_color_frame(3, 64, 48)[:H, :W]
    rgba = synth_color_frame(4, 64, 48, channels=4)[:H, :W]
    dep = synth_depth(5, 64, 48)[:H, :W].copy()
    dep[0, :3] = (0, 65535, 0x1234)
    write_png(str(tmp_path / "c.png"), rgb.reshape(H, -1), W, H, 8, 2, 3, filters)
    write_png(str(tmp_path / "a.png"), rgba.reshape(H, -1), W, H, 8, 6, 4, filters)
    write_png(str(tmp_path / "d.png"), dep.astype(">u2").view(np.uint8).reshape(H, -1), W, H, 16, 0, 2, filters)
    write_png(str(tmp_path / "g.png"), rgb[..., 1], W, H, 8, 0, 1, filters)
    got = S.read_color_image(str(tmp_path / "c.png"))
    assert got.shape == (H, W, 3) and got.dtype == np.uint8 and np.array_equal(got, rgb[..., ::-1])   # cv::imread: B first
    got = S.read_color_image(str(tmp_path / "a.png"))
    assert got.shape == (H, W, 4) and np.array_equal(got, rgba[..., [2, 1, 0, 3]])
    got = S.read_depth_image(str(tmp_path / "d.png"))
    assert got.shape == (H, W) and got.dtype == np.uint16 and np.array_equal(got, dep)
    assert np.array_equal(S.read_color_image(str(tmp_path / "g.png")), rgb[..., 1])       # a grey file stays 2-D
    assert np.array_equal(S._read_gray_image_py(str(tmp_path / "g.png")), rgb[..., 1])    # the unchanged grey reader
    with pytest.raises(ValueError):
        S.read_depth_image(str(tmp_path / "c.png"))
    with pytest.raises(ValueError):
        S._read_gray_image_py(str(tmp_path / "c.png"))
    np.save(str(tmp_path / "c.npy"), rgb)
    np.save(str(tmp_path / "d.npy"), dep)
    assert np.array_equal(S.read_color_image(str(tmp_path / "c.npy")), rgb)
    assert np.array_equal(S.read_depth_image(str(tmp_path / "d.npy")), dep)


def test_synth_color_and_depth():
    from orb_slam2_comment_amd.synth import synth_color_frame, synth_depth
    a = synth_color_frame(2, 160, 120)
    assert a.shape == (120, 160, 3) and a.dtype == np.uint8 and np.array_equal(a, synth_color_frame(2, 160, 120))
    assert not np.array_equal(a[..., 0], a[..., 1]) and not np.array_equal(a[..., 1], a[..., 2])
    b = synth_color_frame(2, 160, 120, rgb=False)
    assert np.array_equal(b, a[..., ::-1])
    c = synth_color_frame(2, 160, 120, channels=4)
    assert c.shape == (120, 160, 4) and np.array_equal(c[..., :3], a) and len(np.unique(c[..., 3])) > 100
    d = synth_depth(2, 160, 120)
    assert d.shape == (120, 160) and d.dtype == np.uint16 and np.array_equal(d, synth_depth(2, 160, 120))
    zeros = float((d == 0).mean())
    assert 0.04 < zeros < 0.2 and (d == 65535).sum() >= 1 and ((d > 0) & (d < 65535)).mean() > 0.7


# ---- C ABI without a device ------------------------------------------------------------------------------------------
def test_color_entries_exist_and_refuse_a_null_handle():
    """No handle can be created without a device, so all this can show here is that the new entries are exported with
    the declared signatures and refuse a null handle with ORBHIP_E_ARG without touching HIP, whatever else they are
    given.  The checks of channels / stride / weights against a live handle are in tests/test_color_gpu.py
    (test_argument_checks_with_a_live_handle, test_custom_gray_weights)."""
    from orb_slam2_comment_amd import capi
    L = capi.lib()
    assert capi.COLOR_BGR == 0 and capi.COLOR_RGB == 1 and capi.DEPTH_U16 == 0 and capi.DEPTH_F32 == 1
    img = np.zeros((48, 64, 4), np.uint8)
    kps = np.zeros(16, capi.KP_DTYPE)
    desc = np.zeros((16, 32), np.uint8)
    n = C.c_int(-7)
    n32 = np.full(1, -7, np.int32)
    p = capi.ptr
    for ch, stride in ((1, 64), (2, 128), (5, 320), (3, 191), (4, 255), (3, 192)):
        assert L.orbhip_extract_color(None, p(img), 48, 64, ch, 1, stride, p(kps), p(desc), 16, C.byref(n)) == capi.E_ARG
        assert L.orbhip_extract_color_batch(None, p(img), 1, 48, 64, ch, 1, stride, 0, p(kps), p(desc), 16, p(n32)) == capi.E_ARG
        assert L.orbhip_extract_color_batch_device(None, p(img), 1, 48, 64, ch, 1, stride, 0, p(kps), p(desc), 16, p(n32),
                                                   None) == capi.E_ARG
    assert L.orbhip_extract_color(None, p(img), 48, 64, 3, 1, 192, p(kps), p(desc), 16, None) == capi.E_ARG
    w = np.array([4899, 9617, 1868], np.int32)
    assert L.orbhip_extractor_set_gray_weights(None, p(w), 14) == capi.E_ARG
    d = np.zeros((4, 4), np.uint16)
    o = np.zeros(4, np.float32)
    assert L.orbhip_compute_stereo_from_rgbd_raw(None, p(kps), None, 1, p(d), 0, 4, 4, 4, 1.0, 1.0, p(o), p(o)) == capi.E_ARG
    assert L.orbhip_compute_stereo_from_rgbd_raw_device(None, 1, p(kps), None, p(n32), 4, p(d), 0, 4, 4, 4, 0, 1.0, 1.0, p(o),
                                                        p(o)) == capi.E_ARG


def test_python_mirror_declares_the_color_interface():
    import orb_slam2_comment_amd as pkg
    for name in ("set_gray_weights", "extract_color", "extract_color_batch", "extract_color_batch_device"):
        assert callable(getattr(pkg.ORBextractor, name))
    assert callable(pkg.ORBmatcher.ComputeStereoFromRGBDRaw)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbhip.h")).read()
    for sym in ("ORBHIP_COLOR_BGR 0", "ORBHIP_COLOR_RGB 1", "ORBHIP_DEPTH_U16 0", "ORBHIP_DEPTH_F32 1"):
        assert "#define " + sym in hdr
