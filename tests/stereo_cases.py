"""Constructed stereo pairs for Frame::ComputeStereoMatches (k_stereo_sort, k_stereo_match, k_stereo_cull), for
test_stereo_cases_cpu.py (C oracle == sequential reference) and test_stereo_cases_gpu.py (the kernels == sequential
reference, through the host and the device entry).

An extraction of a pair leaves the pair's pyramid in the extractor handle; both ComputeStereoMatches entries then take
key points and descriptors as plain arguments.  The key points here are not extracted: they sit where the kernels make a
choice -- the row reach R, the packed record of k_stereo_sort, the (distance, index) key, the candidate loop past 64
lanes, the uR and level gates on the limit, roundf on half-integers, SAD totals near 2^16, the disparity clamp, every
branch of the two-level median select and the HBM path of the cull.

The contract of the device entry holds for every key point: 16 px inside its own level (level-0 right key points go to
the window-edge limit x = W - 12 / W - 11), right candidates at most one level from the left key point wherever the
refinement runs, all bytes the refinement reads in the interior of the level, row bands inside [0, rows).  seqref
asserts the last two.

Two kinds of match sites:
  textured  the left image shifted by `shift` px plus +-2 noise: "smooth" (random 6-px blocks, three passes of a 5-point
            box filter) or "noise" (3-tap averaged white noise).
  painted   paint_site: the left 11x11 patch is 255 with a 0 centre, the right window (21 x 11) is 255 with a 0 at the
            true position and `sad` grey levels taken off pixels that are never a window centre.  The SAD at the true
            shift is exactly `sad` (0 .. 28050), every other shift costs at least 120 * 255 = 30600, so the minimum, the
            parabola and the median multiset are chosen, not found.  (The issue proposed searching noise seeds for the
            wanted SADs; painting reaches the same values deterministically and every value is asserted from `info`.)

case(name) builds a case once; reference(name) runs seqref on it once per process, checks the case's precondition on
`info` and the reference output, and caches (n, mvuRight, mvDepth, info)."""
import math

import numpy as np

from seqref import extractor as SX
from seqref import matcher as SM

f32 = np.float32
KP_DTYPE = SM.KP_DTYPE
W, H = 320, 240
CONFIGS = {"std": (1.2, 8), "x2": (2.0, 3), "l12": (1.1, 12)}       # (scaleFactor, nlevels) of ORBextractor(1000, ., ., 20, 7)
TH_ORB = (SM.TH_HIGH + SM.TH_LOW) // 2
C21 = f32(f32(1.5) * f32(1.4))                                      # the 2.1 of the cull as the reference computes it

_TABLES, _CASES, _REFS = {}, {}, {}
BUILDERS = {}


def tables(cfg):
    if cfg not in _TABLES:
        _TABLES[cfg] = SX.tables(1000, *CONFIGS[cfg])
    return _TABLES[cfg]


# ---- images -----------------------------------------------------------------------------------------------------------
def _smooth(rng, h, w):
    t = np.kron(rng.integers(0, 256, ((h + 5) // 6, (w + 5) // 6)), np.ones((6, 6), np.int64))[:h, :w]
    for _ in range(3):
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) // 5
    return t.astype(np.uint8)


def _noise(rng, h, w):
    t = rng.integers(0, 256, (h, w)).astype(np.int64)
    return ((t + np.roll(t, 1, 1) + np.roll(t, 1, 0)) // 3).astype(np.uint8)


def pair(texture, seed, shift=10, h=H, noise=2):
    """(left, right): right[y, x] = left[y, x + shift[y]] + U{-noise .. noise}; `shift` an int or one int per row."""
    rng = np.random.default_rng(seed)
    tex = (_smooth if texture == "smooth" else _noise)(rng, h, W + 96)
    shift = np.broadcast_to(np.asarray(shift, np.int64), (h,))
    cols = 32 + shift[:, None] + np.arange(W)[None, :]
    left = np.ascontiguousarray(tex[:, 32:32 + W])
    right = tex[np.arange(h)[:, None], cols].astype(np.int64)
    if noise:
        right = right + rng.integers(-noise, noise + 1, (h, W))
    return left, np.ascontiguousarray(np.clip(right, 0, 255).astype(np.uint8))


def band_shift(bands, h=H):
    """one shift per row from [(first_row, shift), ...]"""
    s = np.zeros(h, np.int64)
    for r0, v in bands:
        s[r0:] = v
    return s


def paint_site(left, right, uL, uR, cy, sad, lean=0):
    """A painted site (module docstring) with the left patch at (uL, cy), the true right position at (uR, cy) and SAD `sad`
    there.  The grey levels come off the 110 window pixels outside row cy, evenly, so SAD(-1) == SAD(+1) and the parabola
    gives deltaR == 0 when sad is a multiple of 110 and lean == 0.  lean > 0 takes `lean` more levels off column uR - 5 (in
    the window of shift -1, not of +1: deltaR > 0), lean < 0 off column uR + 5 (deltaR < 0); they count in `sad`."""
    assert 0 <= sad <= 110 * 255 and 16 <= cy - 5 and cy + 5 < left.shape[0] - 1 and uR - 10 >= 3 and uR + 10 <= W - 2
    left[cy - 5:cy + 6, uL - 5:uL + 6] = 255
    left[cy, uL] = 0
    right[cy - 5:cy + 6, uR - 10:uR + 11] = 255
    right[cy, uR] = 0
    cells = [(y, x) for y in range(cy - 5, cy + 6) if y != cy for x in range(uR - 5, uR + 6)]
    rest = sad - abs(lean)
    assert rest >= 0 and abs(lean) <= 200
    q, r = divmod(rest, len(cells))
    for k, (y, x) in enumerate(cells):
        right[y, x] -= q + (k < r)
    if lean:
        y, x = cy - 5, uR - 5 if lean > 0 else uR + 5
        assert right[y, x] >= abs(lean)
        right[y, x] -= abs(lean)


def paint_ceiling(left, right, uL, uR, cy):
    """Left patch 255 with a 0 centre; right 0 over rows cy +- 5, columns uR - 10 .. uR + 10, 255 on row cy over columns
    uR +- 5 and one 255 at (cy - 2, uR): the 11 SADs are 59670 .. 58395 .. 59670, every one above 50000."""
    left[cy - 5:cy + 6, uL - 5:uL + 6] = 255
    left[cy, uL] = 0
    right[cy - 5:cy + 6, uR - 10:uR + 11] = 0
    right[cy, uR - 5:uR + 6] = 255
    right[cy - 2, uR] = 255


CEILING_SADS = [59670, 59415, 59160, 58905, 58650, 58395, 58650, 58905, 59160, 59415, 59670]


# ---- key points and descriptors ------------------------------------------------------------------------------------------
def keys(xy, octave=0):
    k = np.zeros(len(xy), KP_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy, f32).reshape(-1, 2).T
    k["octave"], k["angle"], k["size"], k["response"], k["class_id"] = octave, 0.0, 31.0, 20.0, -1
    return k


def desc(nbits):
    bits = np.zeros(256, np.uint8)
    bits[:nbits] = 1
    return np.packbits(bits)


def random_descs(rng, n):
    """n descriptors pairwise at least TH_ORB apart: a site matches its own partner only"""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n > 1:
        dist = np.unpackbits(d[:, None, :] ^ d[None, :, :], axis=2).sum(2) + 256 * np.eye(n, dtype=np.int64)
        assert dist.min() >= TH_ORB + 10
    return d


def _case(cfg, left, right, kl, dl, kr, dr, check, mbf=40.0, mb=1.0, **extra):
    dl = np.ascontiguousarray(np.asarray(dl, np.uint8).reshape(-1, 32))
    dr = np.ascontiguousarray(np.asarray(dr, np.uint8).reshape(-1, 32))
    assert len(kl) == len(dl) and len(kr) == len(dr) and left.shape == right.shape and left.shape[1] == W
    return dict(extra, cfg=cfg, left=left, right=right, kl=kl, dl=dl, kr=kr, dr=dr, mbf=float(f32(mbf)), mb=float(f32(mb)),
                check=check)


def builder(*names):
    def deco(fn):
        for n in names:
            BUILDERS[n] = fn
        return fn
    return deco


def case(name):
    if name not in _CASES:
        c = BUILDERS[name](name)
        c["name"] = name
        _CASES[name] = c
    return _CASES[name]


def pyramids(c):
    """the unpadded levels of the case's two images, as test_seqref_gpu.py computes them; kept with the case"""
    if "pyramids" not in c:
        inv = tables(c["cfg"])["inv_scale"]
        c["pyramids"] = (SX.compute_pyramid(c["left"], inv)[0], SX.compute_pyramid(c["right"], inv)[0])
    return c["pyramids"]


def seqref_args(c, kl=None, dl=None, kr=None, dr=None, mbf=None):
    t = tables(c["cfg"])
    lv_l, lv_r = pyramids(c)
    return (c["kl"] if kl is None else kl, c["dl"] if dl is None else dl, c["kr"] if kr is None else kr,
            c["dr"] if dr is None else dr, lv_l, lv_r, t["scale"], t["inv_scale"], c["mbf"] if mbf is None else mbf, c["mb"])


def solo(c, iL, iR):
    """(mvuRight, info) of left key point iL against right key point iR alone"""
    info = {}
    n, ur, dp = SM.compute_stereo_matches(*seqref_args(c, c["kl"][[iL]], c["dl"][[iL]], c["kr"][[iR]], c["dr"][[iR]]), info=info)
    return float(ur[0]), info


def ballast(c):
    """Append copies of the accepted left key point with the largest SAD, one more than there are accepted ones: the median
    is then that SAD and the cull removes nothing, so that every site of the case shows in the output.  (Textured SADs
    grow with the level; without this the coarse sites of a mixed-level case fall to the cull.)"""
    info = {}
    SM.compute_stereo_matches(*seqref_args(c), info=info)
    acc = info["accepted"]
    top = max(acc, key=lambda i: acc[i]["sad"])
    extra = [top] * (len(acc) + 1)
    c["kl"] = np.concatenate([c["kl"], c["kl"][extra]])
    c["dl"] = np.concatenate([c["dl"], c["dl"][extra]])
    c["ballast"] = len(extra)
    return c


def reference(name):
    """(n, mvuRight, mvDepth, info) of seqref, computed and checked against the case's precondition once per process"""
    if name not in _REFS:
        c = case(name)
        info = {}
        n, ur, dp = SM.compute_stereo_matches(*seqref_args(c), info=info)
        ur.setflags(write=False)
        dp.setflags(write=False)
        c["check"](c, n, ur, dp, info)
        _REFS[name] = (n, ur, dp, info)
    return _REFS[name]


def _accepted(info, iL, iR=None):
    a = info["accepted"].get(iL)
    return a is not None and (iR is None or a["idx_r"] == iR)


# ---- 1. the row reach R = ceil(2 * max scale) + 1 and the packed record ---------------------------------------------------
def band(cfg, y, octave):
    """[floor(y - r), ceil(y + r)], r = 2 * scale[octave]: the rows a right key point is a candidate on (Frame.cc:483-493)"""
    r = f32(f32(2.0) * tables(cfg)["scale"][octave])
    return int(math.floor(f32(f32(y) - r))), int(math.ceil(f32(f32(y) + r)))


@builder("reach")
def _reach(name):
    """Right key point (140, 100.9) at octave 7: r = 7.166, band [93, 109], 109 = floor(y) + R with R = 9, the largest reach
    there is; its mirror (140, 160.1): band [152, 168], 152 = floor(y) - 8, the largest downward reach.  Left key points at
    x = 150 on the first and last row of each band and one row outside, octaves 5 (level gate), 6 and 7."""
    left, right = pair("smooth", 11)
    assert band("std", 100.9, 7) == (93, 109) and band("std", 160.1, 7) == (152, 168)
    ys = [92.9, 93.0, 100.0, 109.9, 110.0, 151.9, 152.0, 160.0, 168.9, 169.0]
    kl = keys([(150.0, y) for o in (5, 6, 7) for y in ys], np.repeat([5, 6, 7], len(ys)))
    kr = keys([(140.0, 100.9), (140.0, 160.1)], 7)

    def check(c, n, ur, dp, info):
        for i, k in enumerate(kl):
            inside = 93 <= int(k["y"]) <= 109 or 152 <= int(k["y"]) <= 168
            if not inside:
                assert info["exit"][i] == "no_candidates", (i, info["exit"].get(i))
            elif k["octave"] == 5:
                assert info["exit"][i] == "best_dist", (i, info["exit"].get(i))
            else:
                assert _accepted(info, i) and ur[i] > 0, (i, k, info["exit"].get(i))
        assert info["count"]["level_gate"] == 6 and info["count"]["no_candidates"] == 12 and info["count"]["median_cull"] == 0
    return ballast(_case("std", left, right, kl, np.zeros((len(kl), 32)), kr, np.zeros((2, 32)), check))


@builder("reach_x2")
def _reach_x2(name):
    """Scale factor 2.0, 3 levels: r = 2 * 4 is the integer 8, y = 100.5 gives the band [92, 109] and 109 = floor(y) + R."""
    left, right = pair("smooth", 12)
    assert band("x2", 100.5, 2) == (92, 109)
    ys = [91.9, 92.0, 100.0, 109.9, 110.0]
    kl = keys([(150.0, y) for o in (0, 1, 2) for y in ys], np.repeat([0, 1, 2], len(ys)))
    kr = keys([(140.0, 100.5)], 2)

    def check(c, n, ur, dp, info):
        for i, k in enumerate(kl):
            if not 92 <= int(k["y"]) <= 109:
                assert info["exit"][i] == "no_candidates", i
            elif k["octave"] == 0:
                assert info["exit"][i] == "best_dist", i
            else:
                assert _accepted(info, i) and ur[i] > 0, (i, k, info["exit"].get(i))
    return ballast(_case("x2", left, right, kl, np.zeros((len(kl), 32)), kr, np.zeros((1, 32)), check))


def _octave_sites(name, cfg, rows, seed):
    """One right key point per octave and its left partner at the same octave: the octave field and both band fields of
    the record carry a value per level."""
    left, right = pair("smooth", seed)
    n = CONFIGS[cfg][1]
    octs = list(range(n))
    kl = keys([(150.0, rows[o]) for o in octs], octs)
    kr = keys([(140.0, rows[o] + 0.25) for o in octs], octs)
    d = random_descs(np.random.default_rng(seed), n)

    def check(c, nm, ur, dp, info):
        bands = [band(cfg, kr["y"][o], o) for o in octs]
        assert len({b[0] for b in bands}) == n and len({b[1] for b in bands}) == n
        ok = [o for o in octs if _accepted(info, o, o) and ur[o] > 0]
        c["matched_octaves"] = ok
        assert ok == octs, (ok, info["exit"])
    return ballast(_case(cfg, left, right, kl, d, kr, d, check))


@builder("octaves8")
def _octaves8(name):
    return _octave_sites(name, "std", [20 + 22 * o for o in range(8)], 13)


@builder("octaves12")
def _octaves12(name):
    """Scale factor 1.1, 12 levels: octaves 8 .. 11 need the fourth bit of the record's octave field."""
    return _octave_sites(name, "l12", [50 + 12 * o for o in range(12)], 14)


# ---- 2. more than 64 candidates in one row range ---------------------------------------------------------------------------
def _crowd(seed, nrows, specials, extra_right=0):
    """One left key point (150, 100) and 64 right key points on each of the rows 98 .. 98 + nrows - 1, x spread over
    [110, 150]: every one passes the row, level and uR gates, and row k of them fills round k + 1 of the 64-lane candidate
    loop exactly (the order sorts by row and no right key point lies above).  Fillers are 80 .. 179 bits from the left
    descriptor; specials = [(row, x, bits)] replace the filler of that row nearest to x.  The right array is permuted,
    except that the specials come in the given order at the indices chosen by the seed, ascending."""
    left, right = pair("smooth", 21)
    rng = np.random.default_rng(seed)
    xs = (f32(110) + np.arange(64, dtype=f32) * f32(40) / f32(63)).astype(f32)
    xs[-1] = 150.0
    pts = [[float(x), float(98 + r), 80 + int(rng.integers(0, 100))] for r in range(nrows) for x in xs]
    where = []
    for row, x, bits in specials:
        k = (row - 98) * 64 + int(np.argmin(np.abs(xs - f32(x))))
        assert k not in where
        pts[k] = [float(x), float(row), bits]
        where.append(k)
    rest = [k for k in rng.permutation(len(pts)) if k not in where]
    slots = sorted(int(s) for s in rng.choice(len(pts), len(where), replace=False))
    order = []
    it, sp = iter(rest), iter(where)
    for i in range(len(pts)):
        order.append(next(sp) if i in slots else next(it))
    pts = [pts[k] for k in order]
    # right key points in rows no left key point looks at: they only lengthen the strided loops of the sort
    far = [[float(40 + (i * 7) % 240), float(150 + (i * 5) % 70), 128] for i in range(extra_right)]
    pts = pts + far
    kr = keys([(p[0], p[1]) for p in pts])
    dr = np.stack([desc(p[2]) for p in pts])
    return left, right, keys([(150.0, 100.0)]), np.zeros((1, 32), np.uint8), kr, dr, slots


@builder("crowd_round2", "crowd_round3", "crowd_round4", "crowd_round5_nr400")
def _crowd_winner(name):
    rnd = int(name.split("round")[1][0])
    nrows = 5 if rnd == 5 else 4
    left, right, kl, dl, kr, dr, slots = _crowd(30 + rnd, nrows, [(98 + rnd - 1, 140.0, 10)], 80 if rnd == 5 else 0)

    def check(c, n, ur, dp, info):
        assert len(kr) == (400 if rnd == 5 else 256) and info["count"]["level_gate"] == 0 and info["count"]["ur_range"] == 0
        assert _accepted(info, 0, slots[0]) and ur[0] > 0 and kr["y"][slots[0]] == 98 + rnd - 1
        d = SM.descriptor_distance(dl[0], dr)
        assert (d < TH_ORB).sum() == 1
    return _case("std", left, right, kl, dl, kr, dr, check)


# ---- 3. distance ties: the smallest index wins ----------------------------------------------------------------------------
@builder("ties")
def _ties(name):
    """Per site one left key point (150, y) and right key points with ONE descriptor: at the true position x = 140 and at
    x = 125, 120 (another SAD, another uR or none).  The reference keeps the first index that reaches the minimum."""
    left, right = pair("smooth", 31)
    sites = [  # (y, bits, [(x, dy) in index order])
        (24, 20, [(140.0, 0), (125.0, 0)]),                      # the true one first
        (48, 20, [(125.0, 0), (140.0, 0)]),                      # the false one first
        (72, 20, [(120.0, 0), (140.0, 0), (125.0, 0)]),          # three
        (96, 20, [(140.0, 2), (125.0, -2)]),                     # the smallest index in a later row bucket
        (120, 20, [(125.0, 2), (140.0, -2)]),
        (144, 20, [(125.0, 1), (140.0, -1), (120.0, 2)]),
        (168, 74, [(125.0, 0), (140.0, 0)]),                     # ties at the best distance there is
        (192, 74, [(140.0, 1), (125.0, -1)]),
        (210, 75, [(140.0, 0)]),                                 # alone at thOrbDist: rejected
        (223, 74, [(140.0, 0)]),                                 # alone one below: accepted
    ]
    kl = keys([(150.0, float(y)) for y, _, _ in sites])
    rxy, rd, first = [], [], []
    for y, bits, rs in sites:
        first.append(len(rxy))
        for x, dy in rs:
            rxy.append((x, float(y + dy)))
            rd.append(desc(bits))
    kr = keys(rxy)

    def check(c, n, ur, dp, info):
        for i, (y, bits, rs) in enumerate(sites):
            if bits == 75:
                assert info["exit"][i] == "best_dist" and ur[i] == -1
                continue
            outcomes = [solo(c, i, first[i] + k)[0] for k in range(len(rs))]
            true = outcomes[[x for x, _ in rs].index(140.0)]
            assert true > 0 and outcomes.count(true) == 1, (i, outcomes)       # the other candidates give another result
            if i in info["accepted"]:
                assert info["accepted"][i]["idx_r"] == first[i], i
            else:
                assert info["exit"][i] != "best_dist" and outcomes[0] == -1, i
            assert (ur[i] == true) == (rs[0][0] == 140.0), (i, ur[i], outcomes)
    return _case("std", left, right, kl, np.zeros((len(kl), 32)), kr, np.stack(rd), check)


@builder("ties_rounds_late", "ties_rounds_early")
def _ties_rounds(name):
    """Two tied candidates in different rounds of the candidate loop (rows 98 and 101 of the crowd: rounds 1 and 4); the
    smaller index sits in round 4 (late) or in round 1 (early), once at the true position and once away from it."""
    late = name.endswith("late")
    sp = [(101, 140.0, 20), (98, 125.0, 20)] if late else [(98, 125.0, 20), (101, 140.0, 20)]
    left, right, kl, dl, kr, dr, slots = _crowd(41 + late, 4, sp)

    def check(c, n, ur, dp, info):
        a, b = solo(c, 0, slots[0])[0], solo(c, 0, slots[1])[0]
        assert a != b and slots[0] < slots[1] and kr["x"][slots[0]] == sp[0][1] and kr["y"][slots[0]] == sp[0][0]
        assert ur[0] == a
        if late:
            assert _accepted(info, 0, slots[0]) and ur[0] > 0
    return _case("std", left, right, kl, dl, kr, dr, check)


# ---- 4. the gates on their limits -----------------------------------------------------------------------------------------
@builder("gates")
def _gates(name):
    """maxD = 40.  Rows < 80 are shifted by 38 px, rows 80 .. 159 by 2 px, the rest by 10 px, so that a right key point
    exactly on uL - maxD or on uL still leads to an accepted match (SAD minimum at inc = +2 / -2)."""
    left, right = pair("smooth", 41, band_shift([(0, 38), (80, 2), (160, 10)]))
    lo, hi = f32(110.0), f32(150.0)
    L, R = [], []      # (x, y, octave), site i: left i against right i with descriptor i

    def site(l, r):
        L.append(l)
        R.append(r)
        return len(L) - 1
    at_min = site((150.0, 30.0, 0), (lo, 30.0, 0))
    below_min = site((150.0, 50.0, 0), (np.nextafter(lo, f32(0)), 50.0, 0))
    at_max = site((150.0, 100.0, 0), (hi, 100.0, 0))
    above_max = site((150.0, 120.0, 0), (np.nextafter(hi, f32(1000)), 120.0, 0))
    lvl = {d: site((x, y, 2), (x - 10.0, y, 2 + d)) for d, x, y in ((-1, 100.0, 175.0), (1, 220.0, 175.0), (-2, 100.0, 200.0),
                                                                     (2, 220.0, 200.0))}
    trunc = site((150.0, 60.999, 0), (112.0, 58.0, 0))          # row = (int)vL = 60, the last row of the band [56, 60]
    kl = keys([p[:2] for p in L], [p[2] for p in L])
    kr = keys([p[:2] for p in R], [p[2] for p in R])
    d = random_descs(np.random.default_rng(41), len(L))
    # a second candidate for `trunc` on the band [61, 65]: found by a kernel that rounds vL, with the smaller index it
    # would win there.  And a left key point whose row no band covers.
    kr = np.concatenate([keys([(125.0, 63.0)]), kr])
    dr = np.concatenate([d[[trunc]], d])
    kl = np.concatenate([kl, keys([(150.0, 140.0)])])
    dl = np.concatenate([d, d[[0]]])

    def check(c, n, ur, dp, info):
        assert f32(c["mbf"]) / f32(c["mb"]) == 40 and band("std", 58.0, 0) == (56, 60) and band("std", 63.0, 0) == (61, 65)
        for i in (at_min, at_max, lvl[-1], lvl[1], trunc):
            assert _accepted(info, i, i + 1) and ur[i] > 0, (i, info["exit"].get(i))
        for i in (below_min, above_max, lvl[-2], lvl[2]):
            assert info["exit"][i] == "best_dist" and ur[i] == -1, (i, info["exit"].get(i))
        assert info["accepted"][at_min]["vd"].index(info["accepted"][at_min]["sad"]) == 5 + 2
        assert info["accepted"][at_max]["vd"].index(info["accepted"][at_max]["sad"]) == 5 - 2
        assert info["exit"][len(kl) - 1] == "no_candidates"
        assert info["count"]["level_gate"] >= 2 and info["count"]["ur_range"] >= 2
    return _case("std", left, right, kl, dl, kr, dr, check)


# ---- 5. half-integer coordinates ------------------------------------------------------------------------------------------
def exact_halves(cfg, level, lo, hi):
    """[(k, x)]: float32 x in [lo, hi] whose float32 product with inv_scale[level] is exactly k + 0.5"""
    t = tables(cfg)
    sf, inv = t["scale"][level], t["inv_scale"][level]
    out = []
    for k in range(int(lo / sf), int(hi / sf) + 1):
        x0 = f32(f32(k + 0.5) * sf)
        for x in (np.nextafter(x0, f32(0)), x0, np.nextafter(x0, f32(1e9))):
            if lo <= x <= hi and f32(x * inv) == f32(k + 0.5):
                out.append((k, float(x)))
                break
    return out


@builder("halves")
def _halves(name):
    """roundf (half away from zero), not round-half-even: level-0 key points on x.5 / y.5 with even and odd integer parts
    on both sides, and at octaves 1 .. 3 the x and y whose float32 product with inv_scale is exactly k + 0.5 (found for
    every one of the three levels: `found` lists them; an even k is the one rintf would round down)."""
    left, right = pair("smooth", 51)
    L, R = [], []
    y = 24.0
    for lx in (150.5, 151.5):
        for rx in (140.5, 141.5):
            for fy in (0.5, 1.5):                                     # 24.5 -> 25 (rintf: 24), 47.5 -> 48 (both)
                L.append((lx, y + fy, 0))
                R.append((rx, y + fy, 0))
                y += 20.0
    found = {}
    for level in (1, 2, 3):
        xs = exact_halves("std", level, 60.0, 280.0)
        ys = exact_halves("std", level, 185.0, 205.0)
        found[level] = (len(xs), len(ys))
        ev = [x for k, x in xs if k % 2 == 0]
        if ev and ys:
            xl = min(ev, key=lambda x: abs(x - (70.0 + 60.0 * level)))
            xr = min(ev, key=lambda x: abs(x - (xl - 10.0)))
            yy = [v for k, v in ys if k % 2 == 0] or [v for k, v in ys]
            L.append((xl, yy[0], level))
            R.append((xr, yy[0], level))
    kl = keys([p[:2] for p in L], [p[2] for p in L])
    kr = keys([p[:2] for p in R], [p[2] for p in R])
    d = random_descs(np.random.default_rng(51), len(L))

    def check(c, n, ur, dp, info):
        c["found"] = found
        inv = tables("std")["inv_scale"]
        half = lambda v, l: f32(f32(v) * inv[l]) % 1 == 0.5  # noqa: E731
        assert all(half(k["x"], k["octave"]) and half(k["y"], k["octave"]) for k in kl)
        assert all(half(k["x"], k["octave"]) for k in kr)
        ok = [i for i in range(len(kl)) if _accepted(info, i, i) and ur[i] > 0]
        assert set(ok) >= set(range(8)), (ok, info["exit"])
        assert len(kl) == 8 + sum(1 for l in found if found[l][0] and found[l][1])
        assert len(ok) >= len(kl) - 1, (ok, info["exit"])
    return _case("std", left, right, kl, d, kr, d, check)


# ---- 6. / 7. SAD near its ceiling, the disparity clamp and the disparity range --------------------------------------------
@builder("sad_ceiling", "disparity_zero")
def _ceiling(name):
    zero = name == "disparity_zero"
    left, right = pair("noise", 61)
    uL = 140 if zero else 150
    paint_ceiling(left, right, uL, 140, 100)

    def check(c, n, ur, dp, info):
        a = info["accepted"][0]
        assert a["vd"] == CEILING_SADS and min(a["vd"]) > 50000 and a["sad"] == 58395 and a["delta"] == 0
        if zero:
            assert info["count"]["clamp"] == 1 and ur[0] == f32(140 - 0.01) and dp[0] == f32(f32(40) / f32(0.01)) == 4000
        else:
            assert info["count"]["clamp"] == 0 and ur[0] == 140 and dp[0] == 4 and n == 1
    return _case("std", left, right, keys([(float(uL), 100.0)]), np.zeros((1, 32)), keys([(140.0, 100.0)]), np.zeros((1, 32)), check)


@builder("disparity_negative", "disparity_tiny", "disparity_below_maxd", "disparity_at_maxd")
def _disparity(name):
    """Painted sites whose parabola leans: uL == uR with deltaR > 0 (disparity < 0: rejected) and deltaR < 0 (a tiny positive
    disparity: accepted, not clamped); uL - uR = 10 with deltaR < 0 and maxD one float above the disparity (accepted) and
    equal to it (rejected: disparity < maxD is strict)."""
    left, right = pair("noise", 62)
    same = name in ("disparity_negative", "disparity_tiny")
    uL = 140 if same else 150
    paint_site(left, right, uL, 140, 100, 1100 + 150, lean=150 if name == "disparity_negative" else -150)
    c = _case("std", left, right, keys([(float(uL), 100.0)]), np.zeros((1, 32)), keys([(140.0, 100.0)]), np.zeros((1, 32)), None)
    if not same:
        info = {}
        SM.compute_stereo_matches(*seqref_args(c), info=info)
        a = info["accepted"][0]
        disp = f32(f32(150) - f32(f32(1) * f32(f32(f32(140) + f32(0)) + a["delta"])))
        assert a["delta"] < 0 and disp > 10
        c["mbf"] = float(np.nextafter(disp, f32(100))) if name == "disparity_below_maxd" else float(disp)
        c["disp"] = disp

    def check(c, n, ur, dp, info):
        if name == "disparity_negative":
            assert info["exit"][0] == "disparity_range" and n == 0
        elif name == "disparity_tiny":
            a = info["accepted"][0]
            assert a["delta"] < 0 and a["sad"] == 1250 and info["count"]["clamp"] == 0 and 139.5 < ur[0] < 140 and n == 1
        elif name == "disparity_below_maxd":
            assert _accepted(info, 0) and n == 1 and f32(c["mbf"]) == np.nextafter(c["disp"], f32(100))
            assert dp[0] == f32(f32(c["mbf"]) / c["disp"])
        else:
            assert info["exit"][0] == "disparity_range" and n == 0 and info["count"]["ur_range"] == 0
    c["check"] = check
    return c


# ---- 8. the window edge at level 0, the SAD minimum on the edge of the search ---------------------------------------------
@builder("window_edge")
def _window_edge(name):
    """Rows < 80 shifted by 3 px: right key points at x = W - 12 (endu = W - 1: accepted) and W - 11 (endu >= cols: rejected),
    the pair of test_edge_stereo_disparity_range_and_window_edges.  Rows >= 80 shifted by 10 px: right key points 5 px off
    the true position (SAD minimum at inc = +-5: rejected) and 4 px off (accepted)."""
    left, right = pair("noise", 8, band_shift([(0, 3), (80, 10)]))
    xy = [(W - 12.0, 20.0, W - 12.0), (W - 11.0, 40.0, W - 11.0), (150.0, 100.0, 135.0), (150.0, 120.0, 136.0),
          (150.0, 140.0, 145.0), (150.0, 160.0, 144.0)]
    kl = keys([(u, v) for u, v, _ in xy])
    kr = keys([(r, v) for _, v, r in xy])

    def check(c, n, ur, dp, info):
        assert _accepted(info, 0, 0) and info["exit"][1] == "window_edge" and ur[1] == -1
        assert info["exit"][2] == "sad_edge" and info["exit"][4] == "sad_edge"
        for i, inc in ((3, 4), (5, -4)):
            a = info["accepted"][i]
            assert a["vd"].index(a["sad"]) == 5 + inc and ur[i] > 0
        assert ur[0] > 0
    return _case("std", left, right, kl, np.zeros((6, 32)), kr, np.zeros((6, 32)), check)


# ---- 9. / 10. / 11. the median select and the cull -------------------------------------------------------------------------
def site_grid(h=H):
    """(uR, cy) of the painted sites: 32 px apart in a row, rows 16 px apart; the rows between carry no site"""
    return [(30 + 32 * i, 24 + 16 * j) for j in range((h - 24 - 17) // 16 + 1) for i in range(9)]


def th_dist(median):
    return f32(C21 * f32(median))


def _multiset(name, sads, seed, nr_fill=0, h=H, ys=None):
    """Painted sites with the SADs of `sads` = [(sad, multiplicity)]: one right key point per site, `multiplicity` copies of
    the left one (duplicated key points are legal input; every copy yields the same SAD), in shuffled order.  nr_fill more
    right key points lie on the rows between the sites, where no left key point looks."""
    left, right = pair("noise", seed, h=h)
    rng = np.random.default_rng(seed)
    grid = site_grid(h)
    pick = rng.permutation(len(grid))[:len(sads)] if ys is None else None
    d = random_descs(rng, len(sads))
    L, Ld, vals = [], [], []
    R = []
    for s, (sad, mult) in enumerate(sads):
        if ys is None:
            uR, cy = grid[pick[s]]
            y = float(cy)
        else:
            uR, y = 30 + 32 * s, ys[s]
            cy = SX.std_round(f32(y))
        paint_site(left, right, uR + 10, uR, cy, sad)
        R.append((float(uR), y))
        L += [(float(uR + 10), y)] * mult
        Ld += [d[s]] * mult
        vals += [sad] * mult
    order = rng.permutation(len(L))
    kl = keys([L[i] for i in order])
    dl = np.stack([Ld[i] for i in order])
    vals = np.array([vals[i] for i in order])
    fill = [(float(20 + (i * 13) % 280), float(16 + 16 * ((i * 7) % ((h - 40) // 16)))) for i in range(nr_fill)]
    kr = keys(R + fill)
    dr = np.concatenate([d, rng.integers(0, 256, (nr_fill, 32), dtype=np.uint8)]) if nr_fill else d
    want_median = int(np.sort(vals)[len(vals) // 2])

    def check(c, n, ur, dp, info):
        assert len(info["accepted"]) == len(kl) and all(info["accepted"][i]["sad"] == vals[i] for i in range(len(kl)))
        assert info["median"] == want_median
        th = th_dist(want_median)
        culled = [i for i in range(len(kl)) if not f32(vals[i]) < th]
        assert info["culled"] == culled and n == len(kl) - len(culled)
        assert (ur[np.array(culled, np.int64)] == -1).all() and (np.delete(ur, culled) > 0).all()
        c["median"], c["culled_sads"], c["kept_sads"] = want_median, sorted({int(vals[i]) for i in culled}), \
            sorted(set(vals.tolist()) - {int(vals[i]) for i in culled})
    return _case("std", left, right, kl, dl, kr, dr, check, vals=vals)


def integer_threshold(lo=2, hi=13000):
    """the smallest median m in [lo, hi] whose threshold fl(2.1f * m) is an integer: a SAD can then EQUAL the threshold"""
    for m in range(lo, hi):
        t = th_dist(m)
        if t == np.floor(t) and t <= 110 * 255:
            return m, int(t)
    raise AssertionError("no integer threshold")


def below(median):
    """(largest integer SAD below the threshold of `median`: kept, smallest not below it: culled)"""
    t = float(th_dist(median))
    up = int(np.ceil(t))
    return up - 1, up


MEDIANS = {
    # name: (multiset, median, what it is for)
    "median_nd1": ([(300, 1)], 300),
    "median_nd2": ([(100, 1), (250, 1)], 250),                                  # the larger of two; 250 >= 2.1 * 100
    "median_odd": ([(100, 2), (200, 1), (419, 1), (420, 1)], 200),              # nd = 5
    "median_even": ([(100, 2), (300, 2)], 300),                                 # nd = 4: element 2; 300 >= 2.1 * 100
    "median_run_first": ([(100, 3), (200, 3), (419, 1)], 200),                  # rank 3 = first of the run 3 .. 5
    "median_run_last": ([(100, 1), (200, 3), (450, 3)], 200),                   # rank 3 = last of the run 1 .. 3
    "median_high_byte_0": ([(10, 1), (100, 3), below(100)[0:1] + (1,), below(100)[1:2] + (1,), (900, 1)], 100),
    "median_bin_0_of_4": ([(1000, 2), (1061, 3), (below(1061)[0], 1), (below(1061)[1], 1)], 1061),       # high byte 4
    "median_bin_3_of_4": ([(1700, 2), (1992, 3), (below(1992)[0], 1), (below(1992)[1], 1)], 1992),       # high byte 7
    "median_one_high_byte": ([(1290, 2), (1300, 1), (1400, 2), (1530, 2), (below(1400)[0], 1), (below(1400)[1], 1)], 1400),
}


@builder(*MEDIANS)
def _median(name):
    sads, med = MEDIANS[name]
    c = _multiset(name, sads, 90 + sorted(MEDIANS).index(name))
    inner = c["check"]

    def check(c, n, ur, dp, info):
        inner(c, n, ur, dp, info)
        assert c["median"] == med
        if name == "median_nd2":
            assert c["culled_sads"] == [] and not f32(250) < th_dist(100)
        if name == "median_even":
            assert c["culled_sads"] == [] and not f32(300) < th_dist(100)
        if name == "median_odd":
            assert c["culled_sads"] == [420] and 419 in c["kept_sads"]
        if name == "median_run_first":
            assert c["kept_sads"] == [100, 200, 419] and not f32(419) < th_dist(100)
        if name == "median_run_last":
            assert c["culled_sads"] == [450] and f32(450) < th_dist(450)
        if name.startswith("median_high") or name.startswith("median_bin") or name == "median_one_high_byte":
            lo, hi = below(med)
            assert c["culled_sads"][0] == hi and lo in c["kept_sads"] and f32(lo) < th_dist(med) <= f32(hi)
        if name == "median_high_byte_0":
            assert med >> 8 == 0
        if name == "median_bin_0_of_4":
            assert (med >> 8) % 4 == 0
        if name == "median_bin_3_of_4":
            assert (med >> 8) % 4 == 3
        if name == "median_one_high_byte":
            assert {v >> 8 for v in (1290, 1300, 1400, 1530)} == {5}
    c["check"] = check
    return c


@builder("median_equals_threshold")
def _median_equal(name):
    """A SAD exactly ON the threshold (fl(2.1f * m) is an integer for m = integer_threshold()): culled, `<` is strict."""
    m, t = integer_threshold()
    c = _multiset(name, [(m, 3), (t - 1, 1), (t, 1)], 77)
    inner = c["check"]

    def check(c, n, ur, dp, info):
        inner(c, n, ur, dp, info)
        assert c["median"] == m and th_dist(m) == f32(t) and c["culled_sads"] == [t] and t - 1 in c["kept_sads"]
    c["check"] = check
    return c


@builder("median_zero")
def _median_zero(name):
    """A noise-free pair: every SAD is 0, thDist = 0 and every match is culled -- the reference's behaviour."""
    left, right = pair("smooth", 71, noise=0)
    xy = [(float(x), float(y)) for y in range(20, 221, 8) for x in range(60, 301, 12)]
    kl = keys(xy)
    kr = keys([(x - 10.0, y) for x, y in xy])
    d = np.random.default_rng(71).integers(0, 256, (len(xy), 32), dtype=np.uint8)

    def check(c, n, ur, dp, info):
        acc = info["accepted"]
        assert len(acc) >= 400 and all(a["sad"] == 0 for a in acc.values()) and all(acc[i]["idx_r"] == i for i in acc)
        assert info["median"] == 0 and info["th_dist"] == 0 and n == 0 and (ur == -1).all() and len(info["culled"]) == len(acc)
    return _case("std", left, right, kl, d, kr, d, check)


HBM = {"cull_4096": (4096, 0), "cull_4097": (4097, 0), "cull_4097_nr5000": (4097, 4995), "cull_5000": (5000, 0),
       "cull_5000_nr5000": (5000, 4995)}


@builder(*HBM)
def _hbm(name):
    """The SAD list of k_stereo_cull is copied to LDS up to 4096 entries and read from HBM above: nl = 4096 (the last LDS
    size), 4097 and 5000 (no multiple of 256), each of the two also against 5000 right key points."""
    nl, fill = HBM[name]
    a = nl * 3 // 10
    lo, hi = below(200)
    c = _multiset(name, [(100, a), (200, nl - 2 * a - 200), (lo, 100), (hi, 100), (900, a)], 80 + sorted(HBM).index(name), fill)
    inner = c["check"]

    def check(c, n, ur, dp, info):
        inner(c, n, ur, dp, info)
        assert len(c["kl"]) == nl and len(c["kr"]) == 5 + fill and c["median"] == 200 and c["culled_sads"] == [hi, 900]
    c["check"] = check
    return c


@builder("rows257")
def _rows257(name):
    """320 x 257: k_stereo_sort scans two rows per thread with the upper half of the threads idle.  Sites on the first and
    the last legal rows (y = 16 .. 240.9, patch rows up to 246, band up to 243) with empty rows between."""
    ys = [21.0, 21.4, 60.5, 130.0, 131.0, 239.0, 240.9, 240.4]
    lo, hi = below(300)
    c = _multiset(name, [(100, 2), (300, 3), (lo, 1), (hi, 1), (250, 1), (301, 2), (700, 1), (150, 1), (299, 2)][:len(ys)], 111,
                  h=257, ys=ys)
    inner = c["check"]

    def check(c, n, ur, dp, info):
        inner(c, n, ur, dp, info)
        assert c["left"].shape == (257, W) and c["median"] == 300 and c["culled_sads"] == [hi, 700]
        assert max(band("std", y, 0)[1] for y in ys) == 243 and int(max(ys)) == 240
    c["check"] = check
    return c


CASES = list(BUILDERS)
# the cases of one image size and extractor configuration that the device-entry batch test interleaves in one handle
BATCH = ("ties", "median_run_last", "crowd_round4", "gates")
