"""Stereo rectification without a device: the sequential restatement (tests/seqref/rectify.py) against hand-worked
answers, orbhip_init_undistort_rectify_map (host code of the library) against it bit for bit, the matrix / list readers
of the stereo example, and the argument checks of the new C-ABI entries."""
import ctypes as C
import os

import numpy as np
import pytest

from seqref import rectify as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "EuRoC_stereo.yaml")
f32 = np.float32


def identity_maps(w, h, dx=0.0, dy=0.0):
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return xs + f32(dx), ys + f32(dy)


def ramp(w=9, h=7):
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def both(img, m1, m2, table=None):
    a = SR.remap_linear(img, m1, m2, table)
    assert np.array_equal(a, SR.remap_linear_scalar(img, m1, m2, table))      # the array form equals the per-pixel loop
    return a.astype(np.int64)


# ---- seqref: hand-worked answers ---------------------------------------------------------------------------------------
def test_identity_calibration_gives_identity_map_and_image():
    K = [[400.0, 0, 30.0], [0, 410.0, 20.0], [0, 0, 1]]
    m1, m2 = SR.init_undistort_rectify_map(K, [0, 0, 0, 0], None, K, (64, 48))
    xs, ys = identity_maps(64, 48)
    assert np.array_equal(m1, xs) and np.array_equal(m2, ys)          # exactly (j, i)
    m1e, m2e = SR.init_undistort_rectify_map(K, [0, 0, 0, 0, 0], np.eye(3), np.hstack([K, [[0], [0], [0]]]), (64, 48))
    assert np.array_equal(m1e, xs) and np.array_equal(m2e, ys)
    img = np.random.default_rng(1).integers(0, 256, (48, 64), dtype=np.uint8)
    assert np.array_equal(SR.remap_linear(img, m1, m2), img)


def test_vector_form_equals_the_scalar_loop():
    from orb_slam2_comment_amd import settings as S
    c = S.stereo_rectification(FIXTURE)["right"]
    a = SR.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], (97, 31))
    b = SR.init_undistort_rectify_map_scalar(c["K"], c["D"], c["R"], c["P"], (97, 31))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    D8 = [-0.28, 0.07, 2e-4, 2e-5, 0.01, 0.02, -0.003, 0.001]
    a = SR.init_undistort_rectify_map(c["K"], D8, None, c["P"], (40, 33))
    b = SR.init_undistort_rectify_map_scalar(c["K"], D8, None, c["P"], (40, 33))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_table():
    t = SR.bilinear_table()
    assert t.shape == (1024, 4) and np.all(t.sum(1) == 32768) and t.min() == 0
    assert t[0].tolist() == [32768, 0, 0, 0]
    assert t[16].tolist() == [16384, 16384, 0, 0] and t[16 * 32].tolist() == [16384, 0, 16384, 0]
    assert t[1].tolist() == [31 * 1024, 1024, 0, 0] and t[31].tolist() == [1024, 31 * 1024, 0, 0]
    assert t[16 * 32 + 16].tolist() == [8192] * 4
    assert t[3 * 32 + 5].tolist() == [27 * 29 * 32, 5 * 29 * 32, 27 * 3 * 32, 5 * 3 * 32]


def test_half_pixel_offset():
    img = ramp()
    got = both(img, *identity_maps(8, 7, dx=0.5))
    a, b = img[:, :8].astype(np.int64), img[:, 1:9].astype(np.int64)
    assert np.array_equal(got, (a * 16384 + b * 16384 + 16384) >> 15)
    got = both(img, *identity_maps(9, 6, dy=0.5))
    a, b = img[:6].astype(np.int64), img[1:7].astype(np.int64)
    assert np.array_equal(got, (a * 16384 + b * 16384 + 16384) >> 15)


def test_neighbouring_table_rows():
    img = ramp()
    a, b = img[:, :8].astype(np.int64), img[:, 1:9].astype(np.int64)
    assert np.array_equal(both(img, *identity_maps(8, 7, dx=1 / 32)), (a * 31744 + b * 1024 + 16384) >> 15)
    assert np.array_equal(both(img, *identity_maps(8, 7, dx=31 / 32)), (a * 1024 + b * 31744 + 16384) >> 15)
    a, b = img[:6].astype(np.int64), img[1:7].astype(np.int64)
    assert np.array_equal(both(img, *identity_maps(9, 6, dy=1 / 32)), (a * 31744 + b * 1024 + 16384) >> 15)
    assert np.array_equal(both(img, *identity_maps(9, 6, dy=31 / 32)), (a * 1024 + b * 31744 + 16384) >> 15)


def test_round_half_to_even():
    # cvRound((k + 1/64) * 32) = cvRound(32k + 0.5) = 32k (even); cvRound((k + 3/64) * 32) = cvRound(32k + 1.5) = 32k + 2
    sx, _ = SR.cv_round_fixed(np.array([2 + 1 / 64, 2 + 3 / 64, 5 + 1 / 64, 5 + 3 / 64, -1 + 1 / 64, -1 + 3 / 64], np.float32))
    assert sx.tolist() == [64, 66, 160, 162, -32, -30]
    img = ramp()
    a, b = img[:, :8].astype(np.int64), img[:, 1:9].astype(np.int64)
    assert np.array_equal(both(img, *identity_maps(8, 7, dx=1 / 64)), a)                                    # fraction 0
    assert np.array_equal(both(img, *identity_maps(8, 7, dx=3 / 64)), (a * 30720 + b * 2048 + 16384) >> 15)   # fraction 2/32


def test_border_taps_mix_pixels_with_zero():
    img = ramp()                                                           # 7 rows x 9 cols
    h, w = img.shape
    I = img.astype(np.int64)
    got = both(img, *identity_maps(w, h, dx=-0.5))                         # column 0 reads columns -1 | 0
    assert np.array_equal(got[:, 0], (I[:, 0] * 16384 + 16384) >> 15)
    assert np.array_equal(got[:, 1:], (I[:, :-1] * 16384 + I[:, 1:] * 16384 + 16384) >> 15)
    got = both(img, *identity_maps(w, h, dx=0.5))                          # the last column reads cols-1 | cols
    assert np.array_equal(got[:, -1], (I[:, -1] * 16384 + 16384) >> 15)
    got = both(img, *identity_maps(w, h, dy=-0.5))                         # rows likewise
    assert np.array_equal(got[0], (I[0] * 16384 + 16384) >> 15)
    got = both(img, *identity_maps(w, h, dy=0.5))
    assert np.array_equal(got[-1], (I[-1] * 16384 + 16384) >> 15)
    got = both(img, *identity_maps(w, h, dx=-0.5, dy=-0.5))                # the corner: one real tap of four
    assert got[0, 0] == (int(img[0, 0]) * 8192 + 16384) >> 15
    got = both(img, *identity_maps(w, h, dx=-1.0))                         # x0 = -1 with fraction 0: weight 32768 on the outside tap
    assert np.all(got[:, 0] == 0) and np.array_equal(got[:, 1:], I[:, :-1])


def test_wholly_outside_and_nan_give_zero():
    img = np.full((7, 9), 200, np.uint8)
    m1, m2 = identity_maps(9, 7)
    for bad in (np.nan, -2.0, 9.0, 1e9, -1e9, 3e38, -3e38, np.inf, -np.inf):
        a, b = m1.copy(), m2.copy()
        a[2, 3] = bad
        b[4, 5] = bad if bad != 9.0 else 7.0
        got = both(img, a, b)
        assert got[2, 3] == 0 and got[4, 5] == 0 and (got == 200).sum() == 61
    cnt = SR.tap_classes(*identity_maps(9, 7, dx=-0.5), (7, 9))
    # the last row's lower taps are at row 7 = outside, whatever the weight they carry
    assert np.all(cnt[:-1, 0] == 2) and cnt[-1, 0] == 1 and np.all(cnt[:-1, 1:] == 4) and np.all(cnt[-1, 1:] == 2)


def test_table_that_sums_to_two_saturates():
    img = ramp()
    t = SR.bilinear_table() * 2
    t[0, 0] = 65535
    got = both(img, *identity_maps(8, 7, dx=0.5), t)
    a, b = img[:, :8].astype(np.int64), img[:, 1:9].astype(np.int64)
    assert np.array_equal(got, np.minimum(255, (a * 32768 + b * 32768 + 16384) >> 15))
    assert (got == 255).sum() > 5 and (got < 255).sum() > 5


# ---- the library's host code -----------------------------------------------------------------------------------------
def _scaled(c, w, h):
    s = np.diag([w / c["width"], h / c["height"], 1.0])
    return s @ c["K"], s @ c["P"]


def test_library_map_equals_seqref_bit_for_bit():
    from orb_slam2_comment_amd import init_undistort_rectify_map, settings as S
    cal = S.stereo_rectification(FIXTURE)
    D8 = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.011, 0.021, -0.0031, 0.0012])
    cases = []
    for side in ("left", "right"):
        c = cal[side]
        assert c["D"].size == 5
        cases.append((c["K"], c["D"], c["R"], c["P"], (752, 480)))                       # 5 coefficients
    c = cal["left"]
    cases.append((c["K"], D8, c["R"], c["P"], (752, 480)))                               # 8 coefficients
    cases.append((c["K"], c["D"][:4], c["R"], c["P"], (752, 480)))                       # 4 coefficients
    cases.append((c["K"], c["D"], None, c["P"], (752, 480)))                             # R = NULL
    K2, P2 = _scaled(cal["right"], 321, 243)
    cases.append((K2, cal["right"]["D"], cal["right"]["R"], P2, (321, 243)))
    cases.append((K2, D8, None, P2[:, :3], (321, 243)))
    for K, D, R, P, size in cases:
        want = SR.init_undistort_rectify_map(K, D, R, P, size)
        got = init_undistort_rectify_map(K, D, R, P, size)
        assert got[0].dtype == np.float32 and got[0].shape == (size[1], size[0])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (len(D), R is None, size)
    a = init_undistort_rectify_map(c["K"], c["D"], None, c["P"], (64, 48))
    b = init_undistort_rectify_map(c["K"], c["D"], np.eye(3), c["P"], (64, 48))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the EuRoC maps are what the issue describes: (almost) every tap inside the source
    for side, most in (("left", 1.0), ("right", 0.9998)):
        c = cal[side]
        m = init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], (752, 480))
        assert (SR.tap_classes(m[0], m[1], (480, 752)) == 4).mean() >= most


def test_map_argument_checks():
    from orb_slam2_comment_amd import capi
    L, p = capi.lib(), capi.ptr
    K = np.array([400.0, 0, 30, 0, 400, 20, 0, 0, 1])
    D = np.zeros(8)
    m = np.zeros((4, 4), np.float32)
    ok = L.orbhip_init_undistort_rectify_map
    assert ok(p(K), p(D), 5, None, p(K), 4, 4, p(m), p(m.copy())) == capi.OK
    for nD in (0, 3, 6, 7, 9, 12, 14):
        assert ok(p(K), p(D), nD, None, p(K), 4, 4, p(m), p(m)) == capi.E_ARG
    assert ok(None, p(D), 5, None, p(K), 4, 4, p(m), p(m)) == capi.E_ARG
    assert ok(p(K), None, 5, None, p(K), 4, 4, p(m), p(m)) == capi.E_ARG
    assert ok(p(K), p(D), 5, None, None, 4, 4, p(m), p(m)) == capi.E_ARG
    assert ok(p(K), p(D), 5, None, p(K), 0, 4, p(m), p(m)) == capi.E_ARG
    assert ok(p(K), p(D), 5, None, p(K), 4, -1, p(m), p(m)) == capi.E_ARG
    assert ok(p(K), p(D), 5, None, p(K), 4, 4, None, p(m)) == capi.E_ARG
    assert ok(p(K), p(D), 5, None, p(np.zeros(9)), 4, 4, p(m), p(m)) == capi.E_ARG        # singular P * R


# ---- settings, lists -------------------------------------------------------------------------------------------------
def test_matrix_reader_on_the_fixture():
    from orb_slam2_comment_amd import settings as S
    text = open(FIXTURE).read()
    assert "data:[" in text and "data: [" in text                       # both spellings are in the file
    mats = S.load_matrices(FIXTURE)
    assert sorted(mats) == sorted(s + k for s in ("LEFT.", "RIGHT.") for k in "DKRP")
    assert mats["LEFT.D"].shape == (1, 5) and mats["LEFT.K"].shape == (3, 3) and mats["RIGHT.P"].shape == (3, 4)
    assert all(m.dtype == np.float64 for m in mats.values())
    assert mats["LEFT.D"].tolist() == [[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]]
    assert mats["RIGHT.D"].tolist() == [[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0]]
    assert mats["LEFT.K"].tolist() == [[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]]
    assert mats["RIGHT.K"][0, 2] == 379.999 and mats["RIGHT.K"][2, 2] == 1.0
    assert mats["LEFT.R"][0, 0] == 0.999966347530033 and mats["LEFT.R"][2, 1] == -0.007044357138835809
    assert mats["RIGHT.R"][1, 2] == -0.007035845251224894
    assert mats["LEFT.P"][0].tolist() == [435.2046959714599, 0.0, 367.4517211914062, 0.0]
    assert mats["RIGHT.P"][0, 3] == -47.90639384423901 and mats["RIGHT.P"][2].tolist() == [0.0, 0.0, 1.0, 0.0]
    cal = S.stereo_rectification(FIXTURE)
    for side in ("left", "right"):
        c = cal[side]
        assert (c["width"], c["height"]) == (752, 480) and c["D"].shape == (5,)
        assert c["K"].shape == (3, 3) and c["R"].shape == (3, 3) and c["P"].shape == (3, 4)
    st = S.load_settings(FIXTURE)                                        # unchanged: scalars only
    assert st["LEFT.width"] == 752 and st["Camera.bf"] == 47.90639384423901 and st["ORBextractor.nFeatures"] == 1200
    assert not any(k.endswith((".K", ".D", ".R", ".P")) or k in ("rows", "cols", "dt", "data") for k in st)


def test_matrix_reader_spellings_and_missing_parameters(tmp_path):
    from orb_slam2_comment_amd import settings as S
    p = tmp_path / "s.yaml"
    p.write_text("%YAML:1.0\nCamera.fx: 1.5\nA.M: !!opencv-matrix\n   rows: 2\n   cols: 3\n   dt: f\n   data: [ 1., 2.5,\n"
                 "      -3e-2, 4,\n      5, 6 ]   # trailing comment\nB: 7\nC.M: !!opencv-matrix\n  rows: 1\n  cols: 2\n  dt: d\n"
                 "  data:[1,2]\n")
    mats = S.load_matrices(str(p))
    assert mats["A.M"].tolist() == [[1.0, 2.5, -0.03], [4.0, 5.0, 6.0]] and mats["C.M"].tolist() == [[1.0, 2.0]]
    assert S.load_settings(str(p)) == {"Camera.fx": 1.5, "B": 7}
    bad = tmp_path / "bad.yaml"
    bad.write_text("M: !!opencv-matrix\n   rows: 2\n   cols: 2\n   dt: d\n   data: [1, 2, 3]\n")
    with pytest.raises(ValueError):
        S.load_matrices(str(bad))
    text = open(FIXTURE).read()
    for drop in ("RIGHT.R:", "LEFT.D:", "LEFT.height: 480", "RIGHT.width: 752"):
        q = tmp_path / "missing.yaml"
        if drop.endswith(":"):
            i = text.index(drop)
            j = text.index("]", i) + 1
            q.write_text(text[:i] + text[j:])
        else:
            q.write_text(text.replace(drop, ""))
        with pytest.raises(ValueError, match="Calibration parameters to rectify stereo are missing"):
            S.stereo_rectification(str(q))
    with pytest.raises(ValueError, match="missing"):
        S.stereo_rectification(str(p))


def test_euroc_list(tmp_path):
    from orb_slam2_comment_amd import settings as S
    t = tmp_path / "MH01.txt"
    t.write_text("1403636579763555584\n1403636579813555456\n\n1403636579863555584\n\n")
    left, right, stamps = S.load_euroc_sequence("/d/cam0/data", "/d/cam1/data", str(t))
    assert left == ["/d/cam0/data/1403636579763555584.png", "/d/cam0/data/1403636579813555456.png",
                    "/d/cam0/data/1403636579863555584.png"]
    assert right[1] == "/d/cam1/data/1403636579813555456.png" and len(right) == 3
    assert stamps == [1403636579763555584 / 1e9, 1403636579813555456 / 1e9, 1403636579863555584 / 1e9]


def test_synth_raw_stereo_rectifies_back():
    """The raw pair the GPU tests and the replay test use: its seqref rectification shows the scene it was made from."""
    from orb_slam2_comment_amd import settings as S
    from orb_slam2_comment_amd.synth import synth_raw_stereo, synth_stereo
    cal = S.stereo_rectification(FIXTURE)
    raw = synth_raw_stereo(3, cal)
    ideal = synth_stereo(3, 752, 480)
    for side, r, i in (("left", raw[0], ideal[0]), ("right", raw[1], ideal[1])):
        c = cal[side]
        assert r.shape == (480, 752) and r.dtype == np.uint8
        rect = SR.remap_linear(r, *SR.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], (752, 480)))
        assert np.abs(rect[40:-40, 40:-40].astype(int) - i[40:-40, 40:-40]).mean() < 8


# ---- C ABI without a device ------------------------------------------------------------------------------------------
def test_remap_entries_exist_and_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device: what can be shown here is that the new entries are exported with the
    declared signatures and answer ORBHIP_E_ARG without touching HIP.  The checks against a live handle are in
    tests/test_rectify_gpu.py (test_argument_checks_with_a_live_handle)."""
    from orb_slam2_comment_amd import capi
    L, p = capi.lib(), capi.ptr
    assert capi.REMAP_TABLE_SIZE == 4096
    img = np.zeros((48, 64), np.uint8)
    m = np.zeros((48, 64), np.float32)
    kps = np.zeros(16, capi.KP_DTYPE)
    desc = np.zeros((16, 32), np.uint8)
    n = C.c_int(-7)
    n32 = np.full(1, -7, np.int32)
    assert L.orbhip_extractor_set_remap(None, 48, 64, 48, 64, p(m), p(m)) == capi.E_ARG
    assert L.orbhip_extractor_set_remap(None, 0, 0, 0, 0, None, None) == capi.E_ARG
    assert L.orbhip_extractor_set_remap_table(None, None) == capi.E_ARG
    for ch, stride in ((1, 64), (3, 192), (4, 256), (1, 63)):
        assert L.orbhip_extract_remap(None, p(img), 48, 64, ch, stride, p(kps), p(desc), 16, C.byref(n)) == capi.E_ARG
        assert L.orbhip_extract_remap_batch(None, p(img), 1, 48, 64, ch, stride, 0, p(kps), p(desc), 16, p(n32)) == capi.E_ARG
        assert L.orbhip_extract_remap_batch_device(None, p(img), 1, 48, 64, ch, stride, 0, p(kps), p(desc), 16, p(n32), None) == capi.E_ARG
    assert L.orbhip_extract_remap(None, p(img), 48, 64, 1, 64, p(kps), p(desc), 16, None) == capi.E_ARG


def test_mirrors_declare_the_rectification_interface():
    import orb_slam2_comment_amd as pkg
    for name in ("set_remap", "set_remap_table", "extract_remap", "extract_remap_batch", "extract_remap_batch_device"):
        assert callable(getattr(pkg.ORBextractor, name))
    assert callable(pkg.init_undistort_rectify_map)
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    assert "#define ORBHIP_REMAP_TABLE_SIZE 4096" in hdr
    for sym in ("orbhip_init_undistort_rectify_map", "orbhip_extractor_set_remap", "orbhip_extractor_set_remap_table",
                "orbhip_extract_remap", "orbhip_extract_remap_batch", "orbhip_extract_remap_batch_device"):
        assert ("int %s(" % sym) in hdr and any(s[0] == sym for s in pkg.capi.SYMBOLS)
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for m in ("SetRemap", "ClearRemap", "SetRemapTable", "ExtractRemap", "ExtractRemapBatch", "ExtractRemapBatchDevice",
              "InitUndistortRectifyMap"):
        assert ("void %s(" % m) in hpp
