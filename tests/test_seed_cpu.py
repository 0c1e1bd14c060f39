"""Hand-worked answers of the sequential restatement tests/seqref/seed.py (the arbiter of tests/test_seed_gpu.py), the
mThDepth of the settings reader, and the argument checks of the new C-ABI entries.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

from seqref import seed as SS
from test_color_cpu import TUM_YAML
from test_settings_cpu import YAML

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.eye(4, dtype=np.float32)[:3]
P, O = SS.POINT_PRESENT, SS.POINT_OBSERVED


def _seed(depth, th, mode=SS.SEED_CLOSEST, flags=None, created_flags=P, K=(2.0, 2.0, 0.0, 0.0), Tcw=IDENT, keys=None):
    n = len(depth)
    keys = np.zeros((n, 2), np.float32) if keys is None else keys
    flags = np.zeros(n, np.uint8) if flags is None else flags
    return SS.seed_stereo_points(K, Tcw, keys, np.asarray(depth, np.float32), th, mode, created_flags,
                                 np.full((n, 3), -77.0, np.float32), flags)


# ---- unprojection ----------------------------------------------------------------------------------------------------
def test_unprojection_identity_pose():
    # fx = fy = 2: invfx = 0.5 exactly; u - cx = 4, z = 3 -> x = 4 * 3 * 0.5 = 6; v - cy = -2 -> y = -3
    X = SS.unproject_stereo(5.0, 1.0, 3.0, (2.0, 2.0, 1.0, 3.0), IDENT)
    assert [float(v) for v in X] == [6.0, -3.0, 3.0]
    assert all(isinstance(v, np.float32) for v in X)


def test_unprojection_rotation_transposes_and_negates():
    # Rcw = 90 degrees about z (camera x = world y, camera y = -world x), tcw = (1, 2, 3):
    # Rwc = Rcw^T, Ow = -Rcw^T tcw = -(0*1 + -1*2 + 0*3, 1*1 + 0*2 + 0*3, 3) = (2, -1, -3)
    Tcw = np.array([[0, 1, 0, 1], [-1, 0, 0, 2], [0, 0, 1, 3]], np.float32)
    Rwc, Ow = SS.pose_matrices(Tcw)
    assert [[float(v) for v in r] for r in Rwc] == [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    assert [float(v) for v in Ow] == [2.0, -1.0, -3.0]
    # camera point (6, -3, 3) -> world Rwc * p + Ow = (3, 6, 3) + (2, -1, -3) = (5, 5, 0)
    X = SS.unproject_stereo(5.0, 1.0, 3.0, (2.0, 2.0, 1.0, 3.0), Tcw)
    assert [float(v) for v in X] == [5.0, 5.0, 0.0]
    # and it is the inverse of the projection: Rcw * X + tcw gives the camera point back
    back = Tcw[:, :3] @ np.array(X, np.float32) + Tcw[:, 3]
    assert back.tolist() == [6.0, -3.0, 3.0]


def test_unprojection_is_float32_one_operation_at_a_time():
    # (u - cx) * z * invfx with invfx = fl(1 / 3): the double-precision value rounds differently
    K = (3.0, 3.0, 0.25, 0.0)
    X = SS.unproject_stereo(10.1, 0.0, 7.3, K, IDENT)
    inv = f32(1.0) / f32(3.0)
    want = f32(f32(f32(f32(10.1) - f32(0.25)) * f32(7.3)) * inv)
    assert X[0] == want and X[0].dtype == np.float32
    assert float(X[0]) != float(f32((10.1 - 0.25) * 7.3 / 3.0))


# ---- stop rule -------------------------------------------------------------------------------------------------------
def _depths(n_valid, c, th=10.0):
    """n_valid positive depths of which c are <= th, shuffled, with a few invalid entries mixed in."""
    rng = np.random.default_rng(n_valid * 1000 + c)
    near = rng.uniform(0.5, th, c).astype(np.float32)
    far = rng.uniform(th * 1.01, th * 9, n_valid - c).astype(np.float32)
    d = np.concatenate([near, far, np.array([-1, 0, np.nan, -1], np.float32)])
    rng.shuffle(d)
    return d


@pytest.mark.parametrize("n_valid,c,visited", [(150, 30, 101), (150, 100, 101), (150, 101, 102), (150, 120, 121),
                                               (80, 10, 80), (80, 80, 80), (150, 0, 101), (150, 150, 150),
                                               (101, 3, 101), (100, 3, 100)])
def test_stop_rule(n_valid, c, visited):
    d = _depths(n_valid, c)
    w, fg, order, created, counts = _seed(d, 10.0)
    assert counts == (n_valid, visited, visited) and len(order) == visited
    assert visited == min(n_valid, max(101, c + 1))          # the closed form the kernel uses
    # the visited ones are the closest, in (z, i) order
    valid = [i for i in range(len(d)) if d[i] > 0]
    want = sorted(valid, key=lambda i: (d[i], i))[:visited]
    assert order.tolist() == want
    assert created.sum() == visited and set(np.nonzero(created)[0]) == set(want)


def test_closed_form_against_the_loop_everywhere():
    for n_valid in (0, 1, 99, 100, 101, 102, 130):
        for c in range(0, n_valid + 1, 7):
            counts = _seed(_depths(n_valid, c), 10.0)[4]
            assert counts[1] == min(n_valid, max(101, c + 1)), (n_valid, c)


def test_depth_equal_to_the_threshold_at_position_100_does_not_stop():
    # sorted: 100 entries at 1.0, then z == th exactly at j = 100 (nPoints = 101 but z > th is false), then far ones
    d = np.array([1.0] * 100 + [10.0] + [20.0, 30.0, 40.0], np.float32)
    counts = _seed(d, 10.0)[4]
    assert counts == (104, 102, 102)        # j = 100 passes, j = 101 (z = 20) is processed and stops
    d[100] = np.nextafter(f32(10.0), f32(11.0))
    assert _seed(d, 10.0)[4] == (104, 101, 101)


# ---- ordering and filtering ------------------------------------------------------------------------------------------
def test_ties_by_index_invalid_dropped_inf_last():
    d = np.array([5.0, np.inf, 2.0, -1.0, 5.0, 0.0, np.nan, 2.0, 5.0, -0.0], np.float32)
    w, fg, order, created, counts = _seed(d, 100.0)
    assert order.tolist() == [2, 7, 0, 4, 8, 1]
    assert counts == (6, 6, 6)
    assert created.tolist() == [1, 1, 1, 0, 1, 0, 0, 1, 1, 0]
    # dropped entries keep the caller's values
    for i in (3, 5, 6, 9):
        assert w[i].tolist() == [-77.0] * 3 and fg[i] == 0
    assert w[2].tolist() == [0.0, 0.0, 2.0] and fg[1] == P      # +inf is a valid depth: created (its position is not finite)


def test_mode_all_is_index_order_without_stop():
    d = _depths(150, 30)
    flags = np.full(len(d), P | O, np.uint8)
    w, fg, order, created, counts = _seed(d, 10.0, mode=SS.SEED_ALL, flags=flags, created_flags=P | O)
    valid = [i for i in range(len(d)) if d[i] > 0]
    assert order.tolist() == valid and counts == (150, 150, 150)      # flags are not read: everything is created


def test_the_integer_key_orders_like_the_pair():
    """bits(z) << 32 | i as an unsigned integer sorts like (z, i) for z > 0, +inf included."""
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.uniform(1e-30, 1e30, 500), [np.inf, 1e-45, 3.0, 3.0, 3.0]]).astype(np.float32)
    z = z[z > 0]
    rng.shuffle(z)
    key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(z), dtype=np.uint64)
    by_key = (np.sort(key) & np.uint64(0xffffffff)).astype(int).tolist()
    assert by_key == [i for _, i in sorted((z[i], i) for i in range(len(z)))]


# ---- flags -----------------------------------------------------------------------------------------------------------
def test_flags_decide_creation():
    d = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    flags = np.array([P | O, P, 0, O], np.uint8)
    w, fg, order, created, counts = _seed(d, 100.0, flags=flags, created_flags=P | O)
    assert created.tolist() == [0, 1, 1, 1] and counts == (4, 4, 3)      # the kept one is visited and counted
    assert fg.tolist() == [P | O] * 4
    assert w[0].tolist() == [-77.0] * 3 and w[1].tolist() == [0.0, 0.0, 2.0]
    # a kept point counts towards the 100: 101 tracked close points, then a far untracked one is still visited
    d = np.array([1.0] * 101 + [50.0, 60.0], np.float32)
    flags = np.array([P | O] * 101 + [0, 0], np.uint8)
    w, fg, order, created, counts = _seed(d, 10.0, flags=flags)
    assert counts == (103, 102, 1) and created[101] == 1 and created[102] == 0 and fg[101] == P


# ---- close counts ----------------------------------------------------------------------------------------------------
def test_close_counts_are_strict():
    d = np.array([1.0, 10.0, 9.999, -1.0, 0.0, np.nan, 5.0, np.inf, 2.0], np.float32)
    flags = np.array([P, P, 0, P, P, P, P | O, P, O], np.uint8)
    assert SS.count_close_points(d, flags, 10.0) == (2, 2)      # z == th is not close; OBSERVED alone is not tracked
    assert SS.count_close_points(d[:0], flags[:0], 10.0) == (0, 0)


# ---- settings --------------------------------------------------------------------------------------------------------
def test_th_depth_of_the_settings_fixtures(tmp_path):
    from orb_slam2_comment_amd import settings as S
    for text, bf, th, fx in ((YAML, 386.1448, 35, 718.856), (TUM_YAML, 40.0, 40.0, 517.306408)):
        p = tmp_path / "s.yaml"
        p.write_text(text)
        st = S.load_settings(str(p))
        got = S.th_depth(st)
        assert isinstance(got, np.float32)
        assert got == f32(f32(f32(bf) * f32(th)) / f32(fx)) == SS.th_depth(bf, th, fx)
    assert abs(float(S.th_depth(S.load_settings(str(p)))) - 40.0 * 40.0 / 517.306408) < 1e-5
    with pytest.raises(KeyError):
        S.th_depth({"Camera.fx": 500.0})


# ---- C ABI without a device ------------------------------------------------------------------------------------------
def test_seed_entries_exist_and_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device: the entries are exported with the declared signatures and refuse a null
    handle with ORBHIP_E_ARG without touching HIP.  The checks against a live handle are in tests/test_seed_gpu.py."""
    from orb_slam2_comment_amd import capi
    from orb_slam2_comment_amd.matcher import make_camera
    L = capi.lib()
    assert capi.SEED_ALL == 0 and capi.SEED_CLOSEST == 1
    p = capi.ptr
    cam = make_camera(500.0, 500.0, 320.0, 240.0, (0, 0, 640, 480), [1.0, 1.2])
    T = np.ascontiguousarray(IDENT)
    k = np.zeros(4, capi.KP_DTYPE)
    z = np.ones(4, np.float32)
    w = np.zeros((4, 3), np.float32)
    fg = np.zeros(4, np.uint8)
    o = np.zeros(4, np.int32)
    counts = np.full(3, -7, np.int32)
    for mode in (0, 1, 2):
        assert L.orbhip_seed_stereo_points(None, C.byref(cam), p(T), p(k), p(z), 4, 10.0, mode, 1, p(w), p(fg), p(o), p(fg),
                                           p(counts)) == capi.E_ARG
        assert L.orbhip_seed_stereo_points_device(None, 1, C.byref(cam), p(T), p(k), p(o), 4, 0, 1, p(z), 10.0, mode, 1, p(w),
                                                  p(fg), p(o), p(fg), p(counts)) == capi.E_ARG
    assert counts.tolist() == [-7] * 3
    a, b = C.c_int(-7), C.c_int(-7)
    assert L.orbhip_count_close_points(None, p(z), p(fg), 4, 10.0, C.byref(a), C.byref(b)) == capi.E_ARG
    assert L.orbhip_count_close_points_device(None, 1, p(z), p(fg), p(o), 4, 10.0, p(counts)) == capi.E_ARG
    assert (a.value, b.value) == (-7, -7)


def test_mirrors_declare_the_seeding_interface():
    import orb_slam2_comment_amd as pkg
    for name in ("SeedStereoPoints", "SeedStereoPointsDevice", "CountClosePoints", "CountClosePointsDevice"):
        assert callable(getattr(pkg.ORBmatcher, name))
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for sym in ("ORBHIP_SEED_ALL     0", "ORBHIP_SEED_CLOSEST 1"):
        assert "#define " + sym in hdr
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for name in ("SeedStereoPoints", "SeedStereoPointsDevice", "CountClosePoints", "CountClosePointsDevice", "UnprojectStereo"):
        assert name + "(" in hpp
