"""Colour and RGB-D input on the GPU, bit for bit: the grey plane of orbhip_extract_color* against the sequential
restatement (tests/seqref/color.py), the extraction behind it against the oracle and the package's own grey entries on
that grey image, the lifetime rule of a lazy level 0, handles reused across colour / grey / sizes, custom weights,
raw-depth ComputeStereoFromRGBD, and tools/replay_tum.py end to end."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from helpers import assert_kps_equal, synth_frame
from seqref import color as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = [(1241, 376, 0), (752, 480, 0), (640, 480, 0), (321, 243, 5)]   # W, H, extra bytes per row
W15 = (9798, 19235, 3735)


@pytest.fixture(scope="module")
def mods():
    import orb_slam2_comment_amd as pkg
    from oracle import oracle_py as O
    return pkg, O


def color_frame(seed, W, H, ch, rgb):
    from orb_slam2_comment_amd.synth import synth_color_frame
    return synth_color_frame(seed, W, H, channels=ch, rgb=rgb)


def strided(frames, pad):
    """[B, H, W, ch] -> (flat uint8 buffer that ends with the last pixel, row stride, frame stride, view on the frames)."""
    B, H, W, ch = frames.shape
    stride = W * ch + pad
    fstride = H * stride + (3 if pad else 0)
    buf = np.full((B - 1) * fstride + (H - 1) * stride + W * ch, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, frames.shape, (fstride, stride, ch, 1))
    view[...] = frames
    return buf, stride, fstride, view


def run_device(ext, pkg, frames, rgb, pad=0, color=True):
    """extract_color_batch_device (or the grey device entry for [B, H, W] frames); returns (per-frame results, keepalive)."""
    import torch
    if color:
        B, H, W, ch = frames.shape
        buf, stride, fstride, _ = strided(frames, pad)
    else:
        B, H, W = frames.shape
        buf, stride, fstride = np.ascontiguousarray(frames).reshape(-1), W, H * W
    cap = ext.capacity(H, W)
    d_img = torch.from_numpy(buf).cuda()
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_s = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if color:
        ext.extract_color_batch_device(d_img.data_ptr(), B, H, W, ch, rgb, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(),
                                       d_s.data_ptr(), stride=stride, frame_stride=fstride)
    else:
        ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(), d_s.data_ptr())
    ext.sync()
    assert np.all(d_s.cpu().numpy() == 0)
    n = d_n.cpu().numpy()
    k, d = d_k.cpu().numpy(), d_d.cpu().numpy()
    out = [(k[b, :n[b]].copy().view(pkg.KP_DTYPE).reshape(-1), d[b, :n[b]].copy()) for b in range(B)]
    return out, d_img


# ---- the grey plane ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,pad", SIZES + [(322, 243, 1), (323, 241, 0)])     # + row tails of 2 and 3 pixels
@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("rgb", [True, False])
def test_gray_plane_equals_seqref(mods, W, H, pad, ch, rgb):
    pkg, O = mods
    img = color_frame(11 + ch, W, H, ch, rgb)
    want = SC.cvt_gray(img, rgb)
    assert len(np.unique(want)) > 50
    _, _, _, view = strided(img[None], pad)
    for lazy in (False, True):
        ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
        ext.set_lazy_level0(lazy)
        ext.extract_color(view[0], rgb)                                   # host entry, strided rows
        assert np.array_equal(ext.image_pyramid(0), want), "host lazy=%s" % lazy
        ext.extract_color(img[::-1], rgb)                                 # a view with a negative row stride
        assert np.array_equal(ext.image_pyramid(0), want[::-1])
        ext.extract_color_batch(np.stack([img, img[::-1, ::-1]]), rgb)    # host batch
        assert np.array_equal(ext.image_pyramid(0, frame=0), want)
        assert np.array_equal(ext.image_pyramid(0, frame=1), want[::-1, ::-1])
        run_device(ext, pkg, np.stack([img[::-1], img]), rgb, pad)        # device entry, buffer ends with the last pixel
        assert np.array_equal(ext.image_pyramid(0, frame=1), want), "device lazy=%s" % lazy
        assert np.array_equal(ext.image_pyramid(0, frame=0), want[::-1])
        full = ext.image_pyramid(0, frame=1, with_border=True)            # the reflected border comes from the grey plane too
        assert np.array_equal(full, np.pad(want, 19, mode="reflect"))


# ---- extraction behind the conversion ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,pad", SIZES)
@pytest.mark.parametrize("nf", [1000, 2000])
def test_extract_color_equals_oracle_and_grey_entry(mods, W, H, pad, nf):
    pkg, O = mods
    ch, rgb = (3, True) if nf == 1000 else (4, False)
    img = color_frame(21, W, H, ch, rgb)
    gray = SC.cvt_gray(img, rgb)
    ok, od = O.OracleExtractor(nf, 1.2, 8, 20, 7).extract(gray)
    gk, gd = pkg.ORBextractor(nf, 1.2, 8, 20, 7)(gray)
    assert len(ok) > 100
    for lazy in (False, True):
        ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7)
        ext.set_lazy_level0(lazy)
        _, _, _, view = strided(img[None], pad)
        k, d = ext.extract_color(view[0], rgb)
        assert_kps_equal(k, ok, "host vs oracle")
        assert np.array_equal(d, od)
        assert_kps_equal(k, gk, "host vs grey entry")
        assert np.array_equal(d, gd)
        (k, d), = run_device(ext, pkg, img[None], rgb, pad)[0]
        assert_kps_equal(k, ok, "device vs oracle")
        assert np.array_equal(d, od)


@pytest.mark.parametrize("W,H,pad,B,ch,rgb", [(1241, 376, 0, 8, 3, False), (752, 480, 0, 1, 4, True), (640, 480, 0, 136, 4, False),
                                              (321, 243, 5, 8, 3, True), (1241, 376, 0, 136, 3, True)])
def test_device_batches(mods, W, H, pad, B, ch, rgb):
    pkg, O = mods
    uniq = [color_frame(30 + s, W, H, ch, rgb) for s in range(min(B, 8))]
    grays = [SC.cvt_gray(u, rgb) for u in uniq]
    frames = np.stack([uniq[b % 8] for b in range(B)])
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    out, _ = run_device(ext, pkg, frames, rgb, pad)
    for b in (0, B // 2, B - 1):
        assert np.array_equal(ext.image_pyramid(0, frame=b), grays[b % 8])
    gout, _ = run_device(pkg.ORBextractor(1000, 1.2, 8, 20, 7), pkg, np.stack([grays[b % 8] for b in range(B)]), rgb, color=False)
    ora = O.OracleExtractor(1000, 1.2, 8, 20, 7)
    want = [ora.extract(g) for g in grays]
    for b in range(B):
        assert_kps_equal(out[b][0], want[b % 8][0], "frame %d vs oracle" % b)
        assert np.array_equal(out[b][1], want[b % 8][1])
        assert_kps_equal(out[b][0], gout[b][0], "frame %d vs grey entry" % b)
        assert np.array_equal(out[b][1], gout[b][1])


# ---- lazy level 0 lives in the handle ---------------------------------------------------------------------------------
def test_lazy_level0_does_not_need_the_colour_buffer(mods):
    import torch
    pkg, O = mods
    from orb_slam2_comment_amd import matcher as M
    W, H = 640, 480
    left, right = color_frame(41, W, H, 3, True), color_frame(41, W, H, 3, True)
    right[:, :-7] = left[:, 7:]                                        # a crude second eye: 7 px disparity
    gl, gr = SC.cvt_gray(left, True), SC.cvt_gray(right, True)
    results = {}
    for lazy in (False, True):
        ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
        ext.set_lazy_level0(lazy)
        out, d_img = run_device(ext, pkg, np.stack([left, right]), True)
        d_img.fill_(0x5A)                                              # the caller recycles its colour buffer
        torch.cuda.synchronize()
        assert np.array_equal(ext.image_pyramid(0, frame=0), gl) and np.array_equal(ext.image_pyramid(0, frame=1), gr)
        ext2 = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
        ext2.set_lazy_level0(lazy)
        out2, d_img2 = run_device(ext2, pkg, np.stack([left, right]), True)
        d_img2.fill_(0x5A)
        torch.cuda.synchronize()
        m = pkg.ORBmatcher(0.9, True)
        # ComputeStereoMatches reads level 0 of both frames of the handle's last batch: first reader after the overwrite
        results[lazy] = m.ComputeStereoMatches(ext2, ext2, out2[0][0], out2[0][1], out2[1][0], out2[1][1], 40.0, 0.08,
                                               frame_l=0, frame_r=1)
        assert np.array_equal(ext2.blurred_level(0, frame=1), _blur_of(pkg, gr))
    (n0, ur0, dp0), (n1, ur1, dp1) = results[False], results[True]
    assert n0 == n1 and np.array_equal(ur0, ur1) and np.array_equal(dp0, dp1) and n0 > 50


def _blur_of(pkg, gray):
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    e(gray)
    return e.blurred_level(0)


# ---- one handle, colour / grey / another size ----------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [False, True])
def test_interleaving_on_one_handle(mods, lazy):
    pkg, O = mods
    a = color_frame(51, 640, 480, 3, True)
    g = synth_frame(52, 640, 480)
    b = color_frame(53, 752, 480, 4, False)

    def fresh():
        e = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
        e.set_lazy_level0(lazy)
        return e
    want = [fresh().extract_color(a, True), fresh()(g), fresh().extract_color(b, False), fresh()(g)]
    ext = fresh()
    got = [ext.extract_color(a, True), ext(g)]
    assert np.array_equal(ext.image_pyramid(0), g)
    got.append(ext.extract_color(b, False))
    assert np.array_equal(ext.image_pyramid(0), SC.cvt_gray(b, False))
    got.append(ext(g))
    got.append(ext(g))                                                  # the grey entry's graph replay
    want.append(want[3])
    for i, ((k, d), (wk, wd)) in enumerate(zip(got, want)):
        assert_kps_equal(k, wk, "step %d" % i)
        assert np.array_equal(d, wd), i
    # device entries on the same handle: colour after grey after colour, same geometry
    o1, _ = run_device(ext, pkg, np.stack([a, a[::-1]]), True)
    o2, _ = run_device(ext, pkg, np.stack([g, g[::-1]]), True, color=False)
    o3, _ = run_device(ext, pkg, np.stack([a]), True, pad=9)
    assert_kps_equal(o1[0][0], want[0][0])
    assert_kps_equal(o3[0][0], want[0][0])
    assert np.array_equal(o1[0][1], want[0][1]) and np.array_equal(o3[0][1], want[0][1])
    assert_kps_equal(o2[0][0], want[1][0])
    assert np.array_equal(o2[0][1], want[1][1])


def test_grey_golden_after_a_colour_call(mods):
    pkg, O = mods
    g = np.load(os.path.join(ROOT, "tests", "golden", "extract_golden.npz"))
    keys = sorted(k[:-4] for k in g.files if k.endswith("_kps"))
    assert keys
    for key in keys:
        seed, W, H, nf = (int(v) for v in key.split("_")[1:])
        ext = pkg.ORBextractor(nf, 1.2, 8, 20, 7)
        ext.extract_color(color_frame(seed, W, H, 4, True), True)
        k, d = ext(synth_frame(seed, W, H))
        gk = np.frombuffer(zlib.decompress(g[key + "_kps"].tobytes()), pkg.KP_DTYPE)
        gd = np.frombuffer(zlib.decompress(g[key + "_desc"].tobytes()), np.uint8).reshape(-1, 32)
        assert_kps_equal(k, gk, key)
        assert np.array_equal(d, gd), key


# ---- the weights are data -------------------------------------------------------------------------------------------
def test_custom_gray_weights(mods):
    pkg, O = mods
    from orb_slam2_comment_amd import capi
    img = color_frame(61, 640, 480, 4, False)
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    ext.extract_color(img, False)
    d14 = SC.cvt_gray(img, False)
    assert np.array_equal(ext.image_pyramid(0), d14)
    ext.set_gray_weights(W15, 15)
    k, d = ext.extract_color(img, False)
    d15 = SC.cvt_gray(img, False, W15, 15)
    assert not np.array_equal(d14, d15)
    assert np.array_equal(ext.image_pyramid(0), d15)
    ok, od = O.OracleExtractor(1000, 1.2, 8, 20, 7).extract(d15)
    assert_kps_equal(k, ok)
    assert np.array_equal(d, od)
    ext.set_gray_weights((65535, 65535, 65535), 16)                     # saturating table, extreme values
    ext.extract_color(img, False)
    assert np.array_equal(ext.image_pyramid(0), SC.cvt_gray(img, False, (65535, 65535, 65535), 16))
    ext.set_gray_weights((0, 1, 0), 1)
    ext.extract_color(img, False)
    assert np.array_equal(ext.image_pyramid(0), SC.cvt_gray(img, False, (0, 1, 0), 1))
    for bad_w, bad_s in (((65536, 0, 0), 14), ((-1, 0, 0), 14), (W15, 0), (W15, 17)):
        with pytest.raises(pkg.OrbHipError) as ei:
            ext.set_gray_weights(bad_w, bad_s)
        assert ei.value.code == capi.E_ARG
    ext.extract_color(img, False)                                       # a refused table changes nothing
    assert np.array_equal(ext.image_pyramid(0), SC.cvt_gray(img, False, (0, 1, 0), 1))
    ext.set_gray_weights()
    ext.extract_color(img, False)
    assert np.array_equal(ext.image_pyramid(0), d14)


def test_argument_checks_with_a_live_handle(mods):
    import ctypes as C
    pkg, O = mods
    from orb_slam2_comment_amd import capi
    L = capi.lib()
    ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
    img = color_frame(62, 320, 240, 4, True)
    cap = ext.capacity(240, 320)
    kps = np.zeros(cap, capi.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int(-7)
    p = capi.ptr
    for ch, stride in ((1, 320), (2, 640), (5, 1600), (3, 959), (4, 1279)):
        assert L.orbhip_extract_color(ext._h, p(img), 240, 320, ch, 1, stride, p(kps), p(desc), cap, C.byref(n)) == capi.E_ARG
    assert L.orbhip_extract_color(ext._h, p(img), 240, 320, 4, 1, 1280, None, p(desc), cap, C.byref(n)) == capi.E_ARG
    assert L.orbhip_extract_color_batch_device(ext._h, None, 1, 240, 320, 4, 1, 1280, 0, p(kps), p(desc), cap, p(kps), None) == capi.E_ARG
    assert L.orbhip_extract_color(ext._h, None, 240, 320, 4, 1, 1280, p(kps), p(desc), cap, C.byref(n)) == 0 and n.value == 0
    assert L.orbhip_extract_color(ext._h, p(img), 0, 320, 4, 1, 1280, p(kps), p(desc), cap, C.byref(n)) == 0 and n.value == 0
    with pytest.raises(TypeError):
        ext(img)                                                        # operator() still wants CV_8UC1
    with pytest.raises(TypeError):
        ext.extract_color(img[..., 0], True)
    k, d = ext.extract_color(img, True)
    assert len(k) > 50


# ---- raw depth --------------------------------------------------------------------------------------------------------
def oracle_rgbd(O, keys, kun, conv, mbf):
    """oracle.compute_stereo_from_rgbd for the keypoints that fall inside the image.  The oracle, like src/Frame.cc:655,
    indexes the depth image without a bounds check, so for a keypoint outside it there is no reference value to compare
    with (it reads a neighbouring row or past the buffer); those are held to the rule include/orbhip.h states for every
    form of the call instead: d = 0, hence mvuRight = mvDepth = -1."""
    H, W = conv.shape
    u, v = keys["x"].astype(np.int64), keys["y"].astype(np.int64)      # truncation, as Mat::at<float>(int, int) gets them
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    ur, dp = np.full(len(keys), -1, np.float32), np.full(len(keys), -1, np.float32)
    ur[inside], dp[inside] = O.compute_stereo_from_rgbd(keys[inside], kun[inside], conv, mbf)
    return ur, dp


def test_compute_stereo_from_rgbd_raw(mods):
    import torch
    pkg, O = mods
    from orb_slam2_comment_amd import capi
    from orb_slam2_comment_amd.synth import synth_depth
    W, H, mbf = 640, 480, f32(40.0)
    img = color_frame(71, W, H, 3, True)
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    keys, _ = ext.extract_color(img, True)
    raw = synth_depth(71, W, H)
    zy, zx = np.argwhere(raw == 0)[5]
    sy, sx = np.argwhere(raw == 65535)[0]
    extra = np.zeros(7, pkg.KP_DTYPE)
    extra["x"] = [0.0, W - 1 + 0.9, W, -1.5, 17.5, zx + 0.25, sx + 0.75]
    extra["y"] = [0.0, H - 1 + 0.9, 3.0, 5.0, H, zy, sy]
    keys = np.concatenate([keys, extra])
    m = pkg.ORBmatcher(0.9, True)
    kun = m.UndistortKeyPoints(keys, 517.3, 516.5, 318.6, 255.3, (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))
    k5000 = SC.depth_map_factor(5000)
    cases = [(raw, k5000), (raw, f32(1)), ((raw.astype(np.float32) * k5000), f32(1)), ((raw.astype(np.float32) * k5000), f32(0.5)),
             (raw.astype(np.float32), f32(1) + f32(5e-6))]
    dev_in = []
    for depth, factor in cases:
        conv = SC.depth_to_float(depth, factor)
        assert conv.dtype == np.float32
        our, odp = oracle_rgbd(O, keys, kun, conv, mbf)
        ur, dp = m.ComputeStereoFromRGBDRaw(keys, kun, depth, factor, mbf)
        assert np.array_equal(ur, our) and np.array_equal(dp, odp), (depth.dtype, factor)
        ur2, dp2 = m.ComputeStereoFromRGBD(keys, kun, conv, mbf)          # the float entry fed the converted image
        assert np.array_equal(ur2, our) and np.array_equal(dp2, odp)
        assert (dp > 0).sum() > 500 and (dp < 0).sum() > 20
        dev_in.append((depth, factor, our, odp))
    n = len(keys)
    assert dp[n - 3] == -1
    assert dp[n - 2] == -1 and dp[n - 4] == -1 and dp[n - 5] == -1        # zero hole, outside, outside (last case: float, x1)
    # batched device form: two frames with different keypoint counts, row and frame strides in elements
    for depth, factor, our, odp in dev_in[:4]:
        cap, pad = n + 5, 3
        big = np.zeros((2, H + 1, W + pad), depth.dtype)
        big[0, :H, :W] = depth
        big[1, :H, :W] = depth[::-1]
        conv1 = SC.depth_to_float(np.ascontiguousarray(depth[::-1]), factor)
        n1 = n - 100
        our1, odp1 = oracle_rgbd(O, keys[:n1], kun[:n1], conv1, mbf)
        hk = np.zeros((2, cap), pkg.KP_DTYPE); hku = np.zeros((2, cap), pkg.KP_DTYPE)
        hk[0, :n], hku[0, :n], hk[1, :n1], hku[1, :n1] = keys, kun, keys[:n1], kun[:n1]
        as_t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.fields else a).cuda()
        d_depth = torch.from_numpy(big.view(np.int16) if big.dtype == np.uint16 else big).cuda()
        d_k, d_ku = as_t(hk), as_t(hku)
        d_n = torch.tensor([n, n1], dtype=torch.int32, device="cuda")
        d_ur = torch.full((2, cap), 7.0, dtype=torch.float32, device="cuda")
        d_dp = torch.full((2, cap), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        typ = capi.DEPTH_U16 if depth.dtype == np.uint16 else capi.DEPTH_F32
        m.compute_stereo_from_rgbd_raw_device(2, d_k.data_ptr(), d_ku.data_ptr(), d_n.data_ptr(), cap, d_depth.data_ptr(), typ, H, W,
                                              factor, mbf, d_ur.data_ptr(), d_dp.data_ptr(), stride=W + pad,
                                              frame_stride=(H + 1) * (W + pad))
        m.sync()
        ur, dp = d_ur.cpu().numpy(), d_dp.cpu().numpy()
        assert np.array_equal(ur[0, :n], our) and np.array_equal(dp[0, :n], odp)
        assert np.array_equal(ur[1, :n1], our1) and np.array_equal(dp[1, :n1], odp1)
        assert np.all(ur[0, n:] == 7.0) and np.all(dp[1, n1:] == 7.0)     # nothing beyond a frame's count is written
    with pytest.raises(pkg.OrbHipError):
        capi.check(capi.lib().orbhip_compute_stereo_from_rgbd_raw(m._h, capi.ptr(keys), None, n, capi.ptr(raw), 2, H, W, W, 1.0, 1.0,
                                                                  capi.ptr(ur), capi.ptr(dp)), "depth type 2")


# ---- tools/replay_tum.py ------------------------------------------------------------------------------------------------
def _chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def _write_png(path, rows_bytes, w, h, depth, ctype):
    raw = b"".join(b"\x00" + rows_bytes[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(raw, 1)) + _chunk(b"IEND", b""))


def test_replay_tum_tool(mods, tmp_path):
    pkg, O = mods
    from orb_slam2_comment_amd.synth import synth_depth
    from test_color_cpu import TUM_YAML
    W, H, N = 640, 480, 6
    seq = tmp_path / "seq"
    (seq / "rgb").mkdir(parents=True)
    (seq / "depth").mkdir()
    (tmp_path / "TUM1.yaml").write_text(TUM_YAML)
    assoc, rgbtxt, frames = [], ["# color images", "# file", "# timestamp filename"], []
    for i in range(N):
        img = color_frame(80 + i, W, H, 3 if i != 2 else 4, True)
        if i == 4:
            img = np.ascontiguousarray(img[..., 1])                          # a grey file in a colour sequence
        dep = synth_depth(80 + i, W, H)
        t = 1305031102.0 + i / 30.0
        _write_png(str(seq / "rgb" / ("%d.png" % i)), img.reshape(H, -1), W, H, 8, 0 if img.ndim == 2 else (2 if img.shape[2] == 3 else 6))
        _write_png(str(seq / "depth" / ("%d.png" % i)), dep.astype(">u2").view(np.uint8).reshape(H, -1), W, H, 16, 0)
        assoc.append("%.6f rgb/%d.png %.6f depth/%d.png" % (t, i, t + 0.01, i))
        if i == 1:
            assoc.append("")
        rgbtxt.append("%.6f rgb/%d.png" % (t, i))
        frames.append((img, dep))
    (tmp_path / "assoc.txt").write_text("\n".join(assoc) + "\n")
    (seq / "rgb.txt").write_text("\n".join(rgbtxt) + "\n")

    (tmp_path / "TUM1_bgr.yaml").write_text(TUM_YAML.replace("Camera.RGB: 1", "Camera.RGB: 0"))

    def run(yaml, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay_tum.py"), str(tmp_path / yaml), str(seq)]
                           + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    def number(out, label):
        mm = re.search(re.escape(label) + r":\s*([-0-9.e+]+)", out)
        assert mm, (label, out)
        return float(mm.group(1))
    # What rgbd_tum / mono_tum compute on these files: cv::imread hands Tracking the pixels B first (the PNGs above store
    # R first), Camera.RGB picks the conversion (src/Tracking.cc:103-104, :174-183, :214-225), then the Frame constructor.
    # Expected counts come from the oracle on the sequentially converted images, for Camera.RGB 1 and 0 separately.
    factor = SC.depth_map_factor(5000.0)
    dist = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
    want = {}
    for rgb in (True, False):
        ora, ora_ini = O.OracleExtractor(1000, 1.2, 8, 20, 7), O.OracleExtractor(2000, 1.2, 8, 20, 7)
        nk, nd, nmono = [], [], []
        for i, (img, dep) in enumerate(frames):
            if img.ndim == 3:
                img = img.copy()
                img[..., [0, 2]] = img[..., [2, 0]]                             # imread: B G R [A]
            gray, conv = SC.grab_image_rgbd(img, dep, rgb, factor)
            k, _ = ora.extract(gray)
            kun = O.undistort_keypoints(k, 517.306408, 516.469215, 318.643040, 255.313989, dist)
            _, odp = O.compute_stereo_from_rgbd(k, kun, conv, f32(40.0))
            nk.append(len(k)); nd.append(int((odp > 0).sum()))
            nmono.append(len((ora_ini if i == 0 else ora).extract(gray)[0]))
        want[rgb] = (nk, nd, nmono)
    assert want[True][0] != want[False][0] and want[True][1] != want[False][1]    # the setting shows in the counts
    for rgb, yaml in ((True, "TUM1.yaml"), (False, "TUM1_bgr.yaml")):
        nk, nd, nmono = want[rgb]
        out = run(yaml, str(tmp_path / "assoc.txt"))
        assert "median tracking time" in out and "mean tracking time" in out
        assert number(out, "Images in the sequence") == N
        assert number(out, "mean keypoints") == pytest.approx(np.mean(nk), abs=0.006), yaml
        assert number(out, "mean keypoints with depth") == pytest.approx(np.mean(nd), abs=0.006), yaml
        out = run(yaml)
        assert number(out, "Images in the sequence") == N
        assert number(out, "mean keypoints") == pytest.approx(np.mean(nmono), abs=0.006), yaml
        assert nmono[0] > nk[0]
    out = run("TUM1.yaml", str(tmp_path / "assoc.txt"), "--max-frames", "3")
    assert number(out, "Images in the sequence") == 3
    assert number(out, "mean keypoints") == pytest.approx(np.mean(want[True][0][:3]), abs=0.006)
