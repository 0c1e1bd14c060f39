"""k_stereo_sort, k_stereo_match and k_stereo_cull against the sequential reference on the constructed pairs of
stereo_cases.py, through the host entry (one extractor per side) and the device entry (one interleaved handle): n,
mvuRight and mvDepth byte for byte, no tolerance.  An extraction of the case's images puts their pyramid into the
handle; what it extracts is ignored, the key points and descriptors of the call are the constructed ones."""
import numpy as np
import pytest

import stereo_cases as SC
from seqref import matcher as SM

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
_EXT = {}


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd import matcher as M
    return pkg, M


def extractors(pkg, cfg):
    """(left, right, interleaved) extractor handles of a configuration, made once"""
    if cfg not in _EXT:
        sf, nl = SC.CONFIGS[cfg]
        _EXT[cfg] = tuple(pkg.ORBextractor(1000, sf, nl, 20, 7) for _ in range(3))
    return _EXT[cfg]


def same(got, want, what):
    n, ur, dp = got
    wn, wur, wdp = want
    bad = np.flatnonzero((ur.view(np.uint32) != wur.view(np.uint32)) | (dp.view(np.uint32) != wdp.view(np.uint32)))
    assert n == wn and ur.tobytes() == wur.tobytes() and dp.tobytes() == wdp.tobytes(), \
        "%s: n %d / %d, %d rows differ, first %s" % (what, n, wn, len(bad), [(int(i), float(ur[i]), float(wur[i])) for i in bad[:4]])


@pytest.mark.parametrize("name", SC.CASES)
def test_host_entry_equals_seqref(env, name):
    pkg, M = env
    want = SC.reference(name)[:3]
    c = SC.case(name)
    eL, eR, _ = extractors(pkg, c["cfg"])
    eL(c["left"])
    eR(c["right"])
    got = pkg.ORBmatcher().ComputeStereoMatches(eL, eR, c["kl"], c["dl"], c["kr"], c["dr"], c["mbf"], c["mb"])
    same(got, want, name)


def run_device(pkg, cases, counts=None, slack=3):
    """The pairs of `cases` as frames (L0, R0, L1, R1, ...) of ONE extractor handle through
    orbhip_compute_stereo_matches_device, then each pair through the host entry on the same handle (frame_l / frame_r).
    counts[p] = (n_l, n_r) shortens a pair.  cap exceeds every count; the key-point and descriptor rows behind the counts
    are 0xFF bytes (NaN coordinates, octave -1) and the outputs start as a sentinel.  Returns per pair
    (device (n, ur, dp), host (n, ur, dp), ur row, depth row)."""
    import torch
    dev = torch.device("cuda:0")
    P = len(cases)
    cfg = cases[0]["cfg"]
    assert all(c["cfg"] == cfg and c["left"].shape == cases[0]["left"].shape for c in cases)
    counts = counts or [(len(c["kl"]), len(c["kr"])) for c in cases]
    cap = max(max(a, b) for a, b in counts) + slack
    ext = extractors(pkg, cfg)[2]
    frames = np.stack([im for c in cases for im in (c["left"], c["right"])])
    B, H, W = frames.shape
    xcap = ext.capacity(H, W)
    d_img = torch.from_numpy(frames).to(dev)
    x_k = torch.zeros((B, xcap, 7), dtype=torch.int32, device=dev)
    x_d = torch.zeros((B, xcap, 32), dtype=torch.uint8, device=dev)
    x_n = torch.zeros(B, dtype=torch.int32, device=dev)
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, x_k.data_ptr(), x_d.data_ptr(), xcap, x_n.data_ptr())
    ext.sync()
    kb = np.full((B, cap, 28), 0xFF, np.uint8)
    db = np.full((B, cap, 32), 0xFF, np.uint8)
    nb = np.zeros(B, np.int32)
    for p, c in enumerate(cases):
        for side, (k, d) in enumerate(((c["kl"], c["dl"]), (c["kr"], c["dr"]))):
            n = counts[p][side]
            kb[2 * p + side, :n] = np.ascontiguousarray(k[:n]).view(np.uint8).reshape(n, 28)
            db[2 * p + side, :n] = d[:n]
            nb[2 * p + side] = n
    d_k, d_d, d_n = torch.from_numpy(kb).to(dev), torch.from_numpy(db).to(dev), torch.from_numpy(nb).to(dev)
    d_ur = torch.full((P, cap), SENTINEL, dtype=torch.float32, device=dev)
    d_dp = torch.full((P, cap), SENTINEL, dtype=torch.float32, device=dev)
    d_nm = torch.full((P,), -5, dtype=torch.int32, device=dev)
    m = pkg.ORBmatcher()
    mbf, mb = cases[0]["mbf"], cases[0]["mb"]
    assert all((c["mbf"], c["mb"]) == (mbf, mb) for c in cases)
    m.ComputeStereoMatchesDevice(ext, 0, 2, ext, 1, 2, P, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr(), d_k.data_ptr(),
                                 d_d.data_ptr(), d_n.data_ptr(), cap, mbf, mb, d_ur.data_ptr(), d_dp.data_ptr(), d_nm.data_ptr())
    m.sync()
    ur, dp, nm = d_ur.cpu().numpy(), d_dp.cpu().numpy(), d_nm.cpu().numpy()
    out = []
    for p, c in enumerate(cases):
        nl, nr = counts[p]
        host = m.ComputeStereoMatches(ext, ext, c["kl"][:nl], c["dl"][:nl], c["kr"][:nr], c["dr"][:nr], mbf, mb,
                                      frame_l=2 * p, frame_r=2 * p + 1)
        out.append(((int(nm[p]), ur[p, :nl].copy(), dp[p, :nl].copy()), host, ur[p], dp[p]))
    return out


@pytest.mark.parametrize("name", SC.CASES)
def test_device_entry_equals_seqref(env, name):
    pkg, M = env
    want = SC.reference(name)[:3]
    c = SC.case(name)
    (got, host, ur_row, dp_row), = run_device(pkg, [c])
    same(got, want, name + " device entry")
    same(host, want, name + " host entry on the interleaved handle")
    nl = len(c["kl"])
    assert (ur_row[nl:] == SENTINEL).all() and (dp_row[nl:] == SENTINEL).all() and len(ur_row) > nl


def test_device_batch_of_four_pairs(env):
    """(n_l, n_r) = (0, k), (k, 0), (small, large), (large, small) in one call: every pair equals seqref, an empty pair
    counts 0 matches, and behind n_l the sentinel survives in u_right and depth."""
    pkg, M = env
    ties, crowd, big = SC.case("ties"), SC.case("crowd_round4"), SC.case("cull_4097")
    cases = [ties, ties, crowd, big]
    counts = [(0, len(ties["kr"])), (len(ties["kl"]), 0), (len(crowd["kl"]), len(crowd["kr"])), (len(big["kl"]), len(big["kr"]))]
    assert counts[2] == (1, 256) and counts[3] == (4097, 5)
    none = np.zeros(0, np.float32)
    want = [(0, none, none), SM.compute_stereo_matches(*SC.seqref_args(ties, kr=ties["kr"][:0], dr=ties["dr"][:0])),
            SC.reference("crowd_round4")[:3], SC.reference("cull_4097")[:3]]
    assert want[1][0] == 0 and (want[1][1] == -1).all() and want[2][0] == 1 and want[3][0] > 2000
    out = run_device(pkg, cases, counts)
    for p, (got, host, ur_row, dp_row) in enumerate(out):
        same(got, want[p], "pair %d" % p)
        same(host, want[p], "pair %d, host entry" % p)
        nl = counts[p][0]
        assert len(ur_row) == 4100 and (ur_row[nl:] == SENTINEL).all() and (dp_row[nl:] == SENTINEL).all()
    assert out[0][0][0] == 0 and out[1][0][0] == 0
