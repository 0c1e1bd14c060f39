"""tests/seqref/mappoint.py (MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth restated from the
reference text) against cases worked by hand, against the oracle's ComputeDistinctiveDescriptors, and its literal layer
against its plain fp64 layer under measured bounds; the declarations and the argument checks of the C-ABI entries.  No
device.  `random_scene` is the scene tests/test_mappoint_gpu.py and tests/test_cpp_mappoint_gpu.py run the kernels on."""
import ctypes as C
import os

import numpy as np
import pytest

import test_seqref_projection_cpu as PC
from helpers import synth_frame
from seqref import mappoint as MP
from seqref import projection as P

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = MP.UPDATE_DESCRIPTOR | MP.UPDATE_NORMAL_DEPTH
KEY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                      ("class_id", "<i4")])

# ---- fp32 literal layer against the fp64 layer, measured on random_scene() by running this module as a script (repository
# root and tests/ on PYTHONPATH): reference against reference, never a kernel.  A bound is 4x the measured figure, as for
# the projection prologues.
MEASURED = dict(normal=5.71e-7,        # components of mNormalVector, absolute (at most 1; a float sum of up to 130 terms)
                max_dist_rel=1.38e-7,  # mfMaxDistance, relative
                min_dist_rel=1.73e-7)  # mfMinDistance, relative
BOUND = {k: 4 * v for k, v in MEASURED.items()}


# ---- the random scene ------------------------------------------------------------------------------------------------
ROWS, CAP, NKEYS, NPTS, PCAP = 8, 256, 200, 300, 320
COUNTS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)     # both sides of the 16-lane group, the 64-lane row
FAMILIES, FAMILY_SLOTS = 40, 40                                          # and the LDS path (N > 64)
BAD_ROWS = (2, 5)
ONLY_BAD_KF_POINT = 23          # N = 16, observed only by the two bad key frames
BAD_REF_POINTS = {4: -1, 24: 17, 46: 70}        # N = 4, 17, 65: ref_obs = -1, N, N + 5
PATTERN = -0x5A5A5A5B


def random_scene(seed=11):
    """8 key-frame rows of 200 key points (random octaves 0-7, general poses), 300 map points whose observation counts
    cycle through COUNTS.  The 1600 key points form 40 families of 40; a family's descriptors are one random prototype with
    0-4 random bits flipped, and a point observes key points of its own family (p % 40) only, so every observation is its
    point's prototype with 0-4 bits flipped: medians tie and the winner is rarely index 0.  A family has 5 key points in
    every row; lists longer than 40 repeat (row, key point) pairs."""
    rng = np.random.default_rng(seed)
    cam, scam = PC.make_cam()
    S = dict(cam=cam, scam=scam)
    S["T"] = [PC.pose(rng, small=False) for _ in range(ROWS)]
    keys = np.zeros((ROWS, NKEYS), KEY_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, PC.W, (ROWS, NKEYS)), rng.uniform(0, PC.H, (ROWS, NKEYS))
    keys["octave"] = rng.integers(0, 8, (ROWS, NKEYS))
    S["keys"] = keys
    proto = rng.integers(0, 256, (FAMILIES, 32), dtype=np.uint8)
    desc = np.zeros((ROWS, NKEYS, 32), np.uint8)
    slot_row = np.arange(ROWS * NKEYS) % ROWS
    slot_idx = np.arange(ROWS * NKEYS) // ROWS
    for s in range(ROWS * NKEYS):
        bits = np.unpackbits(proto[s // FAMILY_SLOTS])
        bits[rng.choice(256, rng.integers(0, 5), replace=False)] ^= 1
        desc[slot_row[s], slot_idx[s]] = np.packbits(bits)
    S["desc"] = desc
    S["kf_bad"] = np.zeros(ROWS, np.uint8)
    S["kf_bad"][list(BAD_ROWS)] = 1
    start, okf, oidx = [0], [], []
    for p in range(NPTS):
        N = COUNTS[p % len(COUNTS)]
        fam = np.arange(FAMILY_SLOTS) + (p % FAMILIES) * FAMILY_SLOTS
        if p == ONLY_BAD_KF_POINT:
            fam = fam[np.isin(slot_row[fam], BAD_ROWS)]
        slots = rng.choice(fam, N, replace=N > len(fam))
        okf += slot_row[slots].tolist()
        oidx += slot_idx[slots].tolist()
        start.append(start[-1] + N)
    S["obs_start"], S["obs_kf"], S["obs_idx"] = (np.array(a, np.int32) for a in (start, okf, oidx))
    counts = np.diff(S["obs_start"])
    S["ref_obs"] = (rng.integers(0, 1 << 30, NPTS) % np.maximum(counts, 1)).astype(np.int32)
    for p, r in BAD_REF_POINTS.items():
        S["ref_obs"][p] = r
    S["world"] = rng.normal(0, 8, (NPTS, 3)).astype(f32)
    flags = np.where(rng.random(NPTS) < 0.1, 0, P.POINT_PRESENT).astype(np.uint8) | (rng.integers(0, 2, NPTS) * 2).astype(np.uint8)
    flags[[ONLY_BAD_KF_POINT] + list(BAD_REF_POINTS)] |= P.POINT_PRESENT
    S["flags"] = flags
    return S


def sentinels(n):
    """The four arrays pre-filled with a pattern that no result equals."""
    pat = np.array([PATTERN], np.int32).view(f32)[0]
    return np.full((n, 32), 0xA5, np.uint8), np.full((n, 3), pat, f32), np.full(n, pat, f32), np.full(n, pat, f32)


def scene_reference(S, what, n=NPTS):
    pd, nrm, mx, mn = sentinels(n)
    return MP.update_map_points(S["scam"], what, S["T"], S["keys"], S["desc"], S["kf_bad"], S["obs_start"][:n + 1], S["obs_kf"],
                                S["obs_idx"], S["ref_obs"], S["world"], S["flags"], pd, nrm, mx, mn)


_REF = {}


def scene_and_reference(what):
    """The scene and seqref's six arrays for it, computed once per mask and shared; nobody writes to them."""
    if "S" not in _REF:
        _REF["S"] = random_scene()
    if what not in _REF:
        _REF[what] = scene_reference(_REF["S"], what)
        for a in _REF[what]:
            a.setflags(write=False)
    return _REF["S"], _REF[what]


def assert_scene_is_not_vacuous(S, ref):
    """From seqref alone: the statuses all occur, and the descriptors tie the way that tells a wrong tie rule apart."""
    pd, nrm, mx, mn, best, status = ref
    counts = np.diff(S["obs_start"])
    for code in (MP.UPDATED, MP.BAD, MP.NO_OBSERVATION, MP.NO_DESCRIPTOR, MP.BAD_REF):
        assert (status == code).any(), code
    assert status[ONLY_BAD_KF_POINT] == MP.NO_DESCRIPTOR and best[ONLY_BAD_KF_POINT] == -1
    assert all(status[p] == MP.BAD_REF for p in BAD_REF_POINTS)
    tie = other = total = 0
    for p in range(NPTS):
        if best[p] < 0 or counts[p] < 3:
            continue
        o0 = S["obs_start"][p]
        kept = [j for j in range(counts[p]) if not S["kf_bad"][S["obs_kf"][o0 + j]]]
        D = S["desc"][S["obs_kf"][o0 + np.array(kept)], S["obs_idx"][o0 + np.array(kept)]]
        dist = np.unpackbits(D[:, None, :] ^ D[None, :, :], axis=2).sum(2)
        med = np.sort(dist, axis=1)[:, int(0.5 * (len(kept) - 1))]
        total += 1
        tie += (med == med.min()).sum() > 1
        other += best[p] != kept[0]
        assert kept[int(np.argmin(med))] == best[p]
    assert total >= 200 and tie * 2 >= total and other * 4 >= total, (total, tie, other)
    return total, tie, other


# ---- hand-worked cases of the literal layer ---------------------------------------------------------------------------------
IDENT = np.eye(4, dtype=f32)


def _translated(cx, cy, cz):
    """A key frame with identity rotation and camera centre (cx, cy, cz): tcw = -Ow."""
    T = IDENT.copy()
    T[:3, 3] = (-cx, -cy, -cz)
    return T


def _cam(levels=8):
    c, s = PC.make_cam()
    if levels != 8:
        s.n_levels = levels
        s.scale_factors = s.scale_factors[:levels]
    return s


def _run(T, obs, ref, X, what=BOTH, octaves=None, desc=None, kf_bad=None, flags=1, cam=None):
    """One map point observed at key point 0 .. of the key frames `obs` (a list of rows; key point j of row k is (k, j))."""
    K = len(T)
    per_row = [obs.count(k) for k in range(K)]
    keys = [np.zeros(max(n, 1), KEY_DTYPE) for n in per_row]
    descs = [np.zeros((max(n, 1), 32), np.uint8) for n in per_row]
    seen = [0] * K
    okf, oidx = [], []
    for j, k in enumerate(obs):
        i = seen[k]
        seen[k] += 1
        okf.append(k)
        oidx.append(i)
        if octaves is not None:
            keys[k]["octave"][i] = octaves[j]
        if desc is not None:
            descs[k][i] = desc[j]
    pd, nrm, mx, mn = sentinels(1)
    out = MP.update_map_points(cam or _cam(), what, T, keys, descs, kf_bad, [0, len(obs)], okf, oidx, [ref],
                               np.array([X], f32), [flags], pd, nrm, mx, mn)
    return [a[0] for a in out]


def _untouched(pd=None, nrm=None, mx=None, mn=None):
    for got, want in zip((pd, nrm, mx, mn), sentinels(1)):
        if got is not None:
            assert np.asarray(got).tobytes() == want[0].tobytes()


def test_two_observers_on_opposite_sides_give_a_zero_normal():
    # centres (0, 0, -4) and (0, 0, 6), the point at (0, 0, 1): directions (0, 0, 1) and (0, 0, -1); dist to the first is 5
    T = [_translated(0, 0, -4), _translated(0, 0, 6)]
    pd, nrm, mx, mn, best, st = _run(T, [0, 1], 0, (0, 0, 1), octaves=[2, 0])
    assert st == MP.UPDATED and nrm.tolist() == [0.0, 0.0, 0.0]
    s = _cam().scale_factors
    assert mx == f32(5) * s[2] and mn == f32(f32(5) * s[2]) / s[7]
    # referring to the other observer: distance 5 as well, octave 0
    pd, nrm, mx, mn, best, st = _run(T, [0, 1], 1, (0, 0, 1), octaves=[2, 0])
    assert mx == f32(5) and mn == f32(5) / s[7]


def test_single_observer_gives_the_unit_vector_and_min_is_max_over_the_last_factor():
    # centre at the origin, point (3, 0, 4): |.| = 5 exactly, 1.0/5 in double, (float)(0.2 * 3) = 0.6f
    pd, nrm, mx, mn, best, st = _run([IDENT], [0], 0, (3, 0, 4), octaves=[3])
    assert st == MP.UPDATED and best == 0
    assert nrm.tolist() == [float(f32(f64(1.0) / f64(5.0) * f64(3.0))), 0.0, float(f32(f64(1.0) / f64(5.0) * f64(4.0)))]
    assert abs(float(nrm[0]) - 0.6) < 1e-7 and abs(float(nrm[2]) - 0.8) < 1e-7
    s = _cam().scale_factors
    assert mx == f32(5) * s[3] and mn == mx / s[7] and mn.dtype == np.float32
    # fewer levels: the divisor is mvScaleFactors[nLevels-1]
    mn4 = _run([IDENT], [0], 0, (3, 0, 4), octaves=[3], cam=_cam(4))[3]
    assert mn4 == mx / s[3]
    # an octave outside the table: the first entry below 0, a factor of 0 at nLevels and above
    assert _run([IDENT], [0], 0, (3, 0, 4), octaves=[-2])[2] == f32(5) * s[0]
    mx0, mn0 = _run([IDENT], [0], 0, (3, 0, 4), octaves=[8])[2:4]
    assert mx0 == 0 and mn0 == 0


def test_the_sum_of_the_normal_is_float_in_table_order():
    # three directions whose float sum depends on the order; the restatement adds them as the table lists them
    T = [_translated(0.3, -1.7, 2.9), _translated(-5.1, 0.2, 0.4), _translated(1.1, 7.3, -0.6)]
    X = (0.37, 0.11, -0.93)
    v = [MP.view_direction(np.asarray(t, f32)[:3], np.array(X, f32))[1] for t in T]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        nrm = _run(T, order, 0, X)[1]
        third = f64(1.0) / f64(3)
        for c in range(3):
            s = f32(f32(f32(0) + v[order[0]][c]) + v[order[1]][c]) + v[order[2]][c]
            assert nrm[c] == f32(third * f64(s))
    sums = {tuple(_run(T, o, 0, X)[1].tolist()) for o in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0], [0, 2, 1], [1, 0, 2])}
    assert len(sums) > 1        # the order is visible in the bits, which is why it is stated


def test_a_bad_key_frame_leaves_the_descriptor_set_but_not_n():
    # z = 0 bits, a = 8 bits, b = a plus 4 more: d(z,a) = 8, d(z,b) = 12, d(a,b) = 4.  Sorted rows z (0,8,12), a (0,4,8),
    # b (0,4,12): the medians vDists[1] are 8, 4, 4 -> a, the first of the two.  With key frame 1 bad the set is {z, b}:
    # the medians vDists[0] are 0 and 0, the first wins -> list position 0
    z = np.zeros(32, np.uint8)
    a, b = z.copy(), z.copy()
    a[0] = 0xFF
    b[0], b[1] = 0xFF, 0x0F
    T = [_translated(0, 0, -4), _translated(0, 0, 6), _translated(0, 0, -9)]
    pd, nrm, mx, mn, best, st = _run(T, [0, 1, 2], 0, (0, 0, 1), desc=[z, a, b])
    assert best == 1 and np.array_equal(pd, a) and st == MP.UPDATED
    pd, nrm2, mx, mn, best, st = _run(T, [0, 1, 2], 0, (0, 0, 1), desc=[z, a, b], kf_bad=[0, 1, 0])
    assert best == 0 and np.array_equal(pd, z) and st == MP.UPDATED
    # the normal still has all three observers: ((0,0,1) + (0,0,-1) + (0,0,1)) / 3
    assert np.array_equal(nrm, nrm2) and nrm.tolist() == [0.0, 0.0, float(f32(f64(1.0) / f64(3)))]
    # the bad key frame last: the chosen position counts the whole list
    pd, _, _, _, best, _ = _run(T, [1, 0, 2], 0, (0, 0, 1), desc=[a, b, z], kf_bad=[0, 1, 0])
    assert best == 1 and np.array_equal(pd, b)


def test_all_key_frames_bad():
    T = [_translated(0, 0, -4), _translated(0, 0, 6)]
    pd, nrm, mx, mn, best, st = _run(T, [0, 1], 0, (0, 0, 1), kf_bad=[1, 1])
    assert st == MP.NO_DESCRIPTOR and best == -1
    _untouched(pd=pd)
    assert nrm.tolist() == [0.0, 0.0, 0.0] and mx == f32(5)         # normal and depth range are written all the same
    pd, nrm, mx, mn, best, st = _run(T, [0, 1], 0, (0, 0, 1), kf_bad=[1, 1], what=MP.UPDATE_NORMAL_DEPTH)
    assert st == MP.UPDATED


def test_empty_list_bad_point_and_too_many():
    out = _run([IDENT], [], 0, (3, 0, 4))
    assert out[5] == MP.NO_OBSERVATION and out[4] == -1
    _untouched(*out[:4])
    out = _run([IDENT], [0], 0, (3, 0, 4), flags=2)       # OBSERVED without PRESENT
    assert out[5] == MP.BAD and out[4] == -1
    _untouched(*out[:4])
    out = _run([IDENT], [0] * 2049, 0, (3, 0, 4))
    assert out[5] == MP.TOO_MANY and out[4] == -1
    _untouched(*out[:4])
    assert _run([IDENT], [0] * 2048, 0, (3, 0, 4))[5] == MP.UPDATED


@pytest.mark.parametrize("ref", [-1, 2, 100])
def test_ref_obs_out_of_range(ref):
    z = np.zeros(32, np.uint8)
    pd, nrm, mx, mn, best, st = _run([IDENT, _translated(1, 0, 0)], [0, 1], ref, (3, 0, 4), desc=[z + 1, z + 3])
    assert st == MP.BAD_REF and best == 0 and np.array_equal(pd, z + 1)      # the descriptor is written
    _untouched(nrm=nrm, mx=mx, mn=mn)


def test_a_point_on_a_camera_centre_gives_nan():
    T = [_translated(1, 2, 3), _translated(0, 0, 0)]
    pd, nrm, mx, mn, best, st = _run(T, [0, 1], 1, (1, 2, 3))
    assert st == MP.UPDATED and np.isnan(nrm).all()        # 0 * (1.0/0) = NaN, and it stays in the sum
    assert np.isfinite(mx)
    pd, nrm, mx, mn, best, st = _run(T, [0, 1], 0, (1, 2, 3), octaves=[1, 0])
    assert mx == 0 and mn == 0                             # |PC| = 0 times a finite factor


def test_the_first_of_two_equal_medians_wins():
    z = np.zeros(32, np.uint8)
    a, b = z.copy(), z.copy()
    a[0], b[1] = 0x0F, 0xF0          # d(z,a) = d(z,b) = 4, d(a,b) = 8
    # rows sorted: z (0,4,4), a (0,4,8), b (0,4,8): every median is 4 -> index 0, whatever comes first
    assert MP.distinctive_descriptor(np.stack([z, a, b])) == 0
    assert MP.distinctive_descriptor(np.stack([b, a, z])) == 0
    # four: the median is vDists[1]; rows z (0,4,4,12) a (0,4,8,8)... make two rows share the least median, not the first
    c = z.copy()
    c[2:4] = 0xFF                    # far from everything: its own row has the largest median
    assert MP.distinctive_descriptor(np.stack([c, z, a, b])) == 1
    T = [IDENT] * 4
    pd, _, _, _, best, _ = _run(T, [0, 1, 2, 3], 0, (3, 0, 4), desc=[c, z, a, b])
    assert best == 1 and np.array_equal(pd, z)
    pd, _, _, _, best, _ = _run(T, [0, 1, 2, 3], 0, (3, 0, 4), desc=[c, b, a, z])
    assert best == 1 and np.array_equal(pd, b)
    assert MP.distinctive_descriptor(np.stack([a])) == 0 and MP.distinctive_descriptor(np.stack([a, z])) == 0


# ---- reference against reference ------------------------------------------------------------------------------------------------
def test_distinctive_descriptor_equals_the_oracle_on_the_golden_groups(oracle):
    bg = np.load(os.path.join(os.path.dirname(__file__), "golden", "bow_golden.npz"))
    d1 = oracle.OracleExtractor(800, 1.2, 8, 20, 7).extract(synth_frame(21, 640, 480))[1]
    groups = [d1[i:i + 2 + (i % 9)] for i in range(0, 300, 11)]
    want = np.array([oracle.distinctive_descriptor(g) for g in groups], np.int32)
    assert np.array_equal(want, bg["distinct"])
    assert np.array_equal(np.array([MP.distinctive_descriptor(g) for g in groups], np.int32), want)
    # longer and tie-rich lists: the observation lists of the random scene
    S = random_scene()
    for p in range(0, NPTS, 3):
        o0, o1 = S["obs_start"][p], S["obs_start"][p + 1]
        if o1 > o0:
            D = S["desc"][S["obs_kf"][o0:o1], S["obs_idx"][o0:o1]]
            assert MP.distinctive_descriptor(D) == oracle.distinctive_descriptor(np.ascontiguousarray(D)), p


def literal_against_f64(S, ref):
    """Largest deviation of the literal layer from the fp64 layer over the points that were refreshed."""
    pd, nrm, mx, mn, best, status = ref
    dev = dict(normal=0.0, max_dist_rel=0.0, min_dist_rel=0.0)
    n = 0
    for p in range(NPTS):
        if status[p] not in (MP.UPDATED, MP.NO_DESCRIPTOR):
            continue
        o0, o1 = S["obs_start"][p], S["obs_start"][p + 1]
        obs = list(zip(S["obs_kf"][o0:o1].tolist(), S["obs_idx"][o0:o1].tolist()))
        n64, mx64, mn64 = MP.normal_and_depth_f64(S["scam"], S["T"], S["keys"], obs, int(S["ref_obs"][p]), S["world"][p])
        dev["normal"] = max(dev["normal"], float(np.abs(nrm[p].astype(f64) - n64).max()))
        dev["max_dist_rel"] = max(dev["max_dist_rel"], abs(float(mx[p]) - mx64) / mx64)
        dev["min_dist_rel"] = max(dev["min_dist_rel"], abs(float(mn[p]) - mn64) / mn64)
        n += 1
    return dev, n


def test_literal_layer_against_the_f64_layer_on_the_random_scene():
    S, ref = scene_and_reference(BOTH)
    total, tie, other = assert_scene_is_not_vacuous(S, ref)
    dev, n = literal_against_f64(S, ref)
    print("literal vs f64 over %d points: %s; %d lists with N >= 3, %d tied, %d not won by the first" % (n, dev, total, tie, other))
    assert n > 200
    for k, v in dev.items():
        assert v <= BOUND[k], (k, v, BOUND[k])
        assert v > 0                      # the two layers are not the same computation


def test_masks_are_independent():
    S, both = scene_and_reference(BOTH)
    _, d_only = scene_and_reference(MP.UPDATE_DESCRIPTOR)
    _, n_only = scene_and_reference(MP.UPDATE_NORMAL_DEPTH)
    s = sentinels(NPTS)
    assert np.array_equal(d_only[0], both[0]) and np.array_equal(d_only[4], both[4])
    assert all(np.array_equal(d_only[i].view(np.int32), s[i].view(np.int32)) for i in (1, 2, 3))
    assert all(np.array_equal(n_only[i].view(np.int32), both[i].view(np.int32)) for i in (1, 2, 3))
    assert np.array_equal(n_only[0], s[0]) and (n_only[4] == -1).all()
    assert (d_only[5] != MP.BAD_REF).all() and (n_only[5] != MP.NO_DESCRIPTOR).all()


# ---- C ABI without a device -------------------------------------------------------------------------------------------------
def test_update_entries_exist_and_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device: the entries are exported with the declared signatures and refuse a null
    handle, a bad mask and a bad count with ORBHIP_E_ARG without touching HIP or the outputs.  The checks against a live
    handle are in tests/test_mappoint_gpu.py."""
    from orb_slam2_comment_amd import capi
    names = [s[0] for s in capi.SYMBOLS]
    assert "orbhip_update_map_points" in names and "orbhip_update_map_points_device" in names
    assert (capi.UPDATE_DESCRIPTOR, capi.UPDATE_NORMAL_DEPTH) == (MP.UPDATE_DESCRIPTOR, MP.UPDATE_NORMAL_DEPTH) == (1, 2)
    assert (capi.MAPPOINT_UPDATED, capi.MAPPOINT_BAD, capi.MAPPOINT_NO_OBSERVATION, capi.MAPPOINT_NO_DESCRIPTOR,
            capi.MAPPOINT_BAD_REF, capi.MAPPOINT_TOO_MANY) == (MP.UPDATED, MP.BAD, MP.NO_OBSERVATION, MP.NO_DESCRIPTOR,
                                                              MP.BAD_REF, MP.TOO_MANY)
    L = capi.lib()
    p = capi.ptr
    cam = PC.make_cam()[0]
    T = np.ascontiguousarray(IDENT[:3]).reshape(1, 12)
    keys = np.zeros(4, capi.KP_DTYPE)
    desc = np.zeros((4, 32), np.uint8)
    view = capi.FrameView()
    view.n, view.keys, view.desc = 4, p(keys), p(desc)
    arr = (C.POINTER(capi.FrameView) * 1)(C.pointer(view))
    start, okf, oidx, ref = (np.array(a, np.int32) for a in ([0, 2], [0, 0], [1, 2], [0]))
    nk = np.array([4], np.int32)
    w, fg = np.ones((1, 3), np.float32), np.ones(1, np.uint8)
    pd, nrm, mx, mn = sentinels(1)
    best, st = np.full(1, -7, np.int32), np.full(1, 77, np.uint8)

    def host(m, what, n=1):
        return L.orbhip_update_map_points(m, C.byref(cam), what, 1, arr, p(T), None, n, p(start), p(okf), p(oidx), p(ref), p(w),
                                          p(fg), p(pd), p(nrm), p(mx), p(mn), p(best), p(st))

    def device(m, what, n=1, pcap=1):
        return L.orbhip_update_map_points_device(m, C.byref(cam), what, p(T), p(keys), p(desc), p(nk), 4, None, n, pcap, p(start),
                                                 p(okf), p(oidx), p(ref), p(w), p(fg), p(pd), p(nrm), p(mx), p(mn), p(best), p(st))

    for what in (0, 1, 2, 3, 4, 7, -1):
        assert host(None, what) == capi.E_ARG and device(None, what) == capi.E_ARG
    assert host(None, 3, n=-1) == capi.E_ARG and device(None, 3, n=-1) == capi.E_ARG and device(None, 3, n=2, pcap=1) == capi.E_ARG
    s = sentinels(1)
    assert all(np.array_equal(a, b) for a, b in zip((pd, nrm.view(np.int32), mx.view(np.int32), mn.view(np.int32)),
                                                    (s[0], s[1].view(np.int32), s[2].view(np.int32), s[3].view(np.int32))))
    assert best[0] == -7 and st[0] == 77


def test_mirrors_declare_the_update_interface():
    import orb_slam2_comment_amd as pkg
    for name in ("UpdateMapPoints", "UpdateMapPointsDevice"):
        assert callable(getattr(pkg.ORBmatcher, name))
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for sym in ("ORBHIP_UPDATE_DESCRIPTOR   1", "ORBHIP_UPDATE_NORMAL_DEPTH 2", "ORBHIP_MAPPOINT_UPDATED        0",
                "ORBHIP_MAPPOINT_BAD            1", "ORBHIP_MAPPOINT_NO_OBSERVATION 2", "ORBHIP_MAPPOINT_NO_DESCRIPTOR  3",
                "ORBHIP_MAPPOINT_BAD_REF        4", "ORBHIP_MAPPOINT_TOO_MANY       5"):
        assert "#define " + sym in hdr
    assert "int orbhip_update_map_points_device(" in hdr and "int orbhip_update_map_points(" in hdr
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for name in ("UpdateMapPoints", "UpdateMapPointsDevice"):
        assert name + "(" in hpp


if __name__ == "__main__":
    S_, ref_ = scene_and_reference(BOTH)
    print(assert_scene_is_not_vacuous(S_, ref_))
    print(literal_against_f64(S_, ref_))
