"""The rotation-consistency cull of the matcher (rot_bin / three_maxima / "takes no part"), pinned through the entries
whose cull is the stand-alone body (host SearchByBoW, host SearchForTriangulation, CreateNewMapPointsDevice) and, for
matches without a bin, through the fused epilogue of SearchByBoWDevice.

Every scene is built so that the match set BEFORE the cull is known by construction: query i and train keypoint perm[i]
share a position and a random 256-bit descriptor (distance 0, every other pair ~128 > TH_LOW), so matches12[i] is
perm[i] unless the cull drops it; the unchanged oracle's search with the orientation check off confirms that pre-cull
set.  The cull is then computed here from tests/seqref/matcher.py (rotation_bin, compute_three_maxima), never from
the device."""
import numpy as np
import pytest

from helpers import frame_bounds
from seqref import matcher as SR

pytestmark = pytest.mark.gpu

IMG = np.zeros((480, 640), np.uint8)
SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)
F_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)   # epipolar line of (x, y) is the row y: twins pass
FAR = (-1.0e5, -1.0e5)                                               # epipole far outside: its gate rejects nothing


def bin_or_none(a1, a2):
    """The project's rule (comment in rot_bin, orbhip_matcher.hip): the reference's bin, and a match whose bin falls
    outside [0, HISTO_LENGTH) -- caller-supplied angle far outside [0, 360), or NaN -- takes no part: it is neither
    histogrammed nor culled.  The sequential reference asserts there and the oracle would index out of bounds, so the
    extension is made here: seqref's rotation_bin, with its assertion turned into None."""
    if not (np.isfinite(a1) and np.isfinite(a2)):
        return None
    try:
        return SR.rotation_bin(a1, a2)
    except AssertionError:
        return None


def expected(perm, qa, ta, check_ori=True):
    m12 = np.asarray(perm, np.int32).copy()
    bins = [bin_or_none(qa[i], ta[m12[i]]) for i in range(len(m12))]
    if check_ori:
        sizes = [sum(1 for b in bins if b == k) for k in range(SR.HISTO_LENGTH)]
        keep = SR.compute_three_maxima(sizes)
        for i, b in enumerate(bins):
            if b is not None and b not in keep:
                m12[i] = -1
    return int((m12 >= 0).sum()), m12, bins


def query_side(pkg, q_bins, rng, q_angle_override=()):
    """n = len(q_bins) queries.  ta[i] is the angle query i's twin will carry; query i's angle = ta[i] + 30 * q_bins[i]
    (so its bin is q_bins[i]).  q_angle_override: (query, angle) pairs; their twins get angle 0."""
    n = len(q_bins)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    k1 = np.zeros(n, pkg.KP_DTYPE)
    k1["x"] = rng.uniform(20, 350, n); k1["y"] = rng.uniform(20, 220, n)
    ta = rng.integers(0, 40, n).astype(np.float32)
    for i, _ in q_angle_override:
        ta[i] = 0
    k1["angle"] = ta + np.float32(30) * np.asarray(q_bins, np.float32)
    for i, a in q_angle_override:
        k1["angle"][i] = a
    return k1, desc, ta


def train_side(k1, desc, ta, rng):
    """The twins of the queries, shuffled: train keypoint perm[i] is query i's."""
    n = len(k1)
    perm = rng.permutation(n).astype(np.int32)
    k2, d2 = np.zeros_like(k1), np.zeros_like(desc)
    k2["x"][perm] = k1["x"]; k2["y"][perm] = k1["y"]; k2["angle"][perm] = ta
    d2[perm] = desc
    return perm, k2, d2


class Scene:
    def __init__(self, pkg, O, q_bins, rng, q_angle_override=()):
        self.pkg, self.O, self.keep = pkg, O, []
        self.k1, self.d1, ta = query_side(pkg, q_bins, rng, q_angle_override)
        self.perm, self.k2, self.d2 = train_side(self.k1, self.d1, ta, rng)
        self.qa, self.ta = self.k1["angle"].copy(), self.k2["angle"].copy()
        n = len(self.perm)
        self.bow_node1 = np.arange(n, dtype=np.uint32)        # one node per pair: exactly one candidate per query
        self.bow_node2 = np.zeros(n, np.uint32); self.bow_node2[self.perm] = self.bow_node1
        self.tri_node = np.zeros(n, np.uint32)                # a single vocabulary node

    def views(self, make):
        return make(self.k1, self.d1), make(self.k2, self.d2)

    def gpu(self):
        return self.views(lambda k, d: self.pkg.FrameView(k, d, SF, frame_bounds(IMG)))

    def ora(self):
        return self.views(lambda k, d: self.O.make_frame(k, d, None, frame_bounds(IMG), SF, self.keep))

    def bow(self, ori=True):
        o1, o2 = self.ora()                                   # the pre-cull set, from the oracle with the check off
        on, om12 = self.O.search_by_bow(o1, self.bow_node1, None, o2, self.bow_node2, None, 50, 0.75, False)
        assert on == len(self.perm) and np.array_equal(om12, self.perm)
        g1, g2 = self.gpu()
        return self.pkg.ORBmatcher(0.75, ori).SearchByBoW(g1, self.bow_node1, None, g2, self.bow_node2, None, 50)

    def tri(self, ori=True):
        o1, o2 = self.ora()
        on, om12 = self.O.search_for_triangulation(o1, self.tri_node, None, o2, self.tri_node, None, F_ROWS, FAR[0], FAR[1],
                                                   SF * SF, False, False)
        assert on == len(self.perm) and np.array_equal(om12, self.perm)
        g1, g2 = self.gpu()
        return self.pkg.ORBmatcher(0.6, ori).SearchForTriangulation(g1, self.tri_node, None, g2, self.tri_node, None, F_ROWS,
                                                                    FAR, SF * SF)


@pytest.mark.parametrize("nq", [1, 63, 65, 1023, 1025])
def test_row_lengths_around_the_workgroup(oracle, nq):
    """Host SearchForTriangulation, rows of 1 / 63 / 65 / 1023 / 1025 matches: the wavefront histogram add with a partial
    last wavefront, and the loops that stride by the workgroup size (1024).  From 63 up four bins are populated
    (4 : 3 : 2 : 1) and the smallest loses."""
    import orb_slam2_comment_amd as pkg
    rng = np.random.default_rng(nq)
    q_bins = [(2, 2, 2, 2, 5, 5, 5, 9, 9, 11)[i % 10] for i in range(nq)]
    sc = Scene(pkg, oracle, q_bins, rng)
    en, em12, _ = expected(sc.perm, sc.qa, sc.ta)
    n, m12 = sc.tri()
    print("nq", nq, "kept", n, "expected", en)
    assert n == en and np.array_equal(m12, em12)
    if nq >= 63:
        assert 0 < en < nq                           # the scene does cull
    n0, m0 = sc.tri(ori=False)                       # check_ori off: count only, nothing culled
    assert n0 == nq and np.array_equal(m0, sc.perm)


NO_PART_BINS = [2] * 12 + [4] * 10 + [6] * 9 + [8] * 5 + [0] * 4   # bin 8 loses; the last four angles are overridden


ODD = ((36, 400.0), (37, 1000.0), (38, -1000.0), (39, np.nan))


def check_no_part(tag, n, m12, perm, qa, ta):
    en, em12, bins = expected(perm, qa, ta)
    assert bins[36] == 13 and bins[37] is None and bins[38] is None and bins[39] is None
    assert en == 12 + 10 + 9 + 3
    print(tag, "kept", n, "expected", en, "odd rows", m12[36:], "expected", em12[36:])
    assert (m12[37:] == perm[37:]).all()                             # without a bin: survive
    assert (m12[31:36] == -1).all() and m12[36] == -1                # the losing bins are gone
    assert n == en and np.array_equal(m12, em12)


@pytest.mark.parametrize("entry", ["bow", "tri", "bow_device", "cnmp"])
def test_matches_without_a_bin_take_no_part(oracle, entry):
    """40 matches: bins 2 / 4 / 6 / 8 hold 12 / 10 / 9 / 5, and four queries carry angles a caller should not pass:
      400.0  -> rot = 400 - angle2 still rounds to a bin below 30 (13 here): by the bin function it takes part, alone in
                its bin, and is culled like any other loser;
      1000.0 and -1000.0 -> bin 33 / -21: outside the histogram, takes no part, survives;
      NaN    -> no bin, takes no part, survives.
    Expected from bin_or_none above (the rule of the rot_bin comment).
    Before the cull had one home, host SearchByBoW and SearchByBoWDevice dropped every match without a bin, and every
    entry put a NaN angle into bin 0 (the int conversion of NaN).
    bow_device: the fused epilogue of SearchByBoWDevice.  cnmp: CreateNewMapPointsDevice, K = 2, monocular, the twin scene
    written into frame rows of capacity 48: current key frame = row 2, neighbours = rows 0 and 1 (two different shuffles),
    cameras one unit to either side, so the epipolar line of a key point is its own row; nmatches is the count the
    triangulation kernel makes after the cull."""
    import orb_slam2_comment_amd as pkg
    rng = np.random.default_rng(40)
    sc = Scene(pkg, oracle, NO_PART_BINS, rng, ODD)
    if entry in ("bow", "tri"):
        n, m12 = sc.bow() if entry == "bow" else sc.tri()
        check_no_part(entry, n, m12, sc.perm, sc.qa, sc.ta)
        return
    import torch
    dev = torch.device("cuda:0")
    nq, cap = len(sc.perm), 48
    perm_b, k2b, d2b = train_side(sc.k1, sc.d1, sc.k2["angle"][sc.perm], rng)      # a second shuffle of the same twins
    rows = [(sc.k2, sc.d2), (k2b, d2b), (sc.k1, sc.d1)]
    kps, desc = np.zeros((3, cap), pkg.KP_DTYPE), np.zeros((3, cap, 32), np.uint8)
    for f, (k, d) in enumerate(rows):
        kps[f, :nq], desc[f, :nq] = k, d
    d_k = torch.from_numpy(kps.view(np.uint8).reshape(3, cap, 28)).to(dev)
    d_d = torch.from_numpy(desc).to(dev)
    d_n = torch.tensor([nq] * 3, dtype=torch.int32, device=dev)
    m = pkg.ORBmatcher(0.75 if entry == "bow_device" else 0.6, True)
    if entry == "bow_device":
        node = np.full((3, cap), 0xFFFFFFFF, np.uint32)
        node[2, :nq] = sc.bow_node1
        node[0, :nq] = sc.bow_node2
        node[1, perm_b] = sc.bow_node1
        d_node = torch.from_numpy(node.view(np.int32)).to(dev)
        d_m12 = torch.full((2, cap), -5, dtype=torch.int32, device=dev)
        d_nm = torch.full((2,), -5, dtype=torch.int32, device=dev)
        side = (d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), d_node.data_ptr())
        m.SearchByBoWDevice(2, cap, side, 2, 0, side, 0, 1, d_m12.data_ptr(), d_nm.data_ptr(), 50, 0, 0)
        m.sync()
    else:
        d_node = torch.zeros((3, cap), dtype=torch.int32, device=dev)
        T = np.zeros((3, 3, 4), np.float32)
        T[:, :, :3] = np.eye(3, dtype=np.float32)
        T[0, 0, 3], T[1, 0, 3] = 1.0, -1.0
        cam = pkg.matcher.make_camera(250.0, 250.0, 188.0, 120.0, (0.0, 0.0, 376.0, 240.0), SF, mbf=22.5, mb=0.09)
        d_m12 = torch.full((2, cap), -5, dtype=torch.int32, device=dev)
        d_nm = torch.full((2,), -5, dtype=torch.int32, device=dev)
        d_x3d = torch.zeros((2, cap, 3), dtype=torch.float32, device=dev)
        d_st = torch.zeros((2, cap), dtype=torch.uint8, device=dev)
        d_sk = torch.full((2,), 9, dtype=torch.uint8, device=dev)
        d_idx = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        d_T = torch.from_numpy(T.reshape(3, 12)).to(dev)
        d_med = torch.tensor([10.0, 10.0], dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.CreateNewMapPointsDevice(2, 2, d_idx, cam, d_T, d_k, d_d, d_n, cap, d_node, SF * SF, d_m12, d_nm, d_x3d, d_st,
                                   d_sk, d_median_depth=d_med)
        m.sync()
        assert (d_sk.cpu().numpy() == 0).all()
    got, gn = d_m12.cpu().numpy(), d_nm.cpu().numpy()
    for k, (perm, k2) in enumerate(((sc.perm, sc.k2), (perm_b, k2b))):
        check_no_part("%s row %d" % (entry, k), int(gn[k]), got[k, :nq], perm, sc.qa, k2["angle"])
        assert (got[k, nq:] == (-1 if entry == "bow_device" else -5)).all()     # beyond n: cleared / untouched


@pytest.mark.parametrize("sizes", [(10, 1, 1), (11, 1, 1), (5, 5, 5, 5)])
def test_three_maxima_thresholds(oracle, sizes):
    """Host SearchByBoW.  (10, 1, 1): the small bins hold exactly 0.1 * max1, which is not "<": kept.  (11, 1, 1): both
    dropped.  (5, 5, 5, 5): ties keep the first three bins in index order."""
    import orb_slam2_comment_amd as pkg
    rng = np.random.default_rng(sum(sizes))
    q_bins = [b for k, s in enumerate(sizes) for b in [3 + 2 * k] * s]
    sc = Scene(pkg, oracle, q_bins, rng)
    en, em12, _ = expected(sc.perm, sc.qa, sc.ta)
    assert en == {(10, 1, 1): 12, (11, 1, 1): 11, (5, 5, 5, 5): 15}[sizes]
    n, m12 = sc.bow()
    print(sizes, "kept", n, "expected", en)
    assert n == en and np.array_equal(m12, em12)
