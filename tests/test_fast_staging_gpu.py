"""k_fast_cells stages exactly the rows a cell has, lane = row * SW + dword column, 64 / SW rows per instruction, the
last row group based at rows - 64 / SW.  These tests walk every residue of the cell height modulo the rows per instruction
at four of the kernel's five LDS strides, with pyramid-plane and caller's-image sources, and the paths around the staging
(internal frame slots of the chunked host entry, the band path of dense cells).  Everything is bit for bit against the CPU
oracle: per-level candidate lists, final keypoints, descriptors."""
import math
import os
import zlib

import numpy as np
import pytest

from helpers import assert_kps_equal, assert_stagewise_equal, synth_frame

EDGE = 19                      # EDGE_THRESHOLD
TINY_WIDTHS = (65, 76, 84, 90)
TINY_HEIGHTS = tuple(range(62, 69))


def level0_cells(W, H):
    """Pure-Python mirror of the extractor's level-0 cell grid (ORBextractor.cc:781-829) and of the rule that picks the
    FAST kernel's LDS row stride from the widest cell: (stride, cell widths, cell heights), borders of 3 px included."""
    minB, maxBX, maxBY = EDGE - 3, W - EDGE + 3, H - EDGE + 3
    width, height = float(maxBX - minB), float(maxBY - minB)
    nCols, nRows = int(width / 30), int(height / 30)
    wCell, hCell = math.ceil(width / nCols), math.ceil(height / nRows)
    ws = [min(minB + j * wCell + wCell + 6, maxBX) - (minB + j * wCell) for j in range(nCols) if minB + j * wCell < maxBX - 6]
    hs = [min(minB + i * hCell + hCell + 6, maxBY) - (minB + i * hCell) for i in range(nRows) if minB + i * hCell < maxBY - 3]
    need = max((1 + w + 3) >> 2 for w in ws) + 1          # staged dwords (1-px lead) + one real dword on the left
    stride = next(s for s in (11, 13, 15, 17, 21) if need <= s)
    return stride, ws, hs


def test_tiny_frames_reach_four_strides_and_every_height_residue():
    """No GPU run: it pins what the tiny-frame tests below cover.  Stride 21 needs a cell wider than 63 px; with
    30-px cells a single column is at most 59 px wide (two columns start at 60) and a cell of a wider grid at most
    ceil(width / nCols) + 6 <= 51, so no image size reaches it: that instantiation is covered by no test of this file."""
    strides = [level0_cells(W, 64)[0] for W in TINY_WIDTHS]
    assert strides == [11, 13, 15, 17] and len(set(strides)) == 4
    assert [level0_cells(W, 64)[1] for W in TINY_WIDTHS] == [[33], [44], [52], [58]]
    heights = [level0_cells(65, H)[2] for H in TINY_HEIGHTS]
    assert heights == [[h] for h in range(30, 37)]
    for rpi in (3, 4, 5):                                  # rows per staging instruction at strides 17 / 13, 15 / 11
        assert {h[0] % rpi for h in heights} == set(range(rpi))
    assert all(level0_cells(W, H)[0] < 21 for W in range(62, 400) for H in (62, 100))


def tiny_image(W, H, seed):
    """Coarse random blocks plus fine noise: corners in every row of a 30-px cell, its last ones included."""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 2, ((H + 4) // 5, (W + 4) // 5)), np.ones((5, 5), np.int64))[:H, :W] * 110 + 60
    return np.clip(blocks + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def mods(oracle):
    import orb_slam2_comment_amd as pkg
    return pkg, oracle


@pytest.mark.gpu
@pytest.mark.parametrize("W", TINY_WIDTHS)
def test_one_cell_frames_every_height(mods, W):
    """One-level extractors on frames of one cell: the cell is the frame.  Heights 62 .. 68 give cell heights 30 .. 36:
    every residue modulo 3, 4 and 5, with and without an overlapping last row group."""
    pkg, O = mods
    ext = pkg.ORBextractor(200, 1.2, 1, 20, 7)
    ora = O.OracleExtractor(200, 1.2, 1, 20, 7)
    last_rows = 0
    for H in TINY_HEIGHTS:
        assert level0_cells(W, H)[1:] == ([W - 32], [H - 32])
        img = tiny_image(W, H, 100 * W + H)
        kps, desc = ext(img)
        okps, odesc = ora.extract(img)
        what = "%dx%d" % (W, H)
        assert_stagewise_equal(ext, ora, 1, what)
        assert_kps_equal(kps, okps, what)
        assert np.array_equal(desc, odesc), what
        ox, oy, _ = ora.level_candidates(0)
        assert len(ox) >= 5, what
        last_rows += int((np.asarray(oy) == H - 32 - 4).sum())      # bottom detection row: its ring reaches the cell's last row
    assert last_rows > 0


@pytest.mark.gpu
@pytest.mark.parametrize("W", TINY_WIDTHS)
def test_one_cell_frames_read_from_the_callers_image(mods, W):
    """The same sizes with a lazy level 0: the cells are staged from the caller's image, here a view with an odd row stride
    that starts at an odd address, so that source rows begin at byte offsets 0, 1, 2 and 3.  A lazy level 0 needs a second
    level (a one-level handle keeps materialising); at these sizes level 1 is too small to have a cell."""
    import torch
    pkg, O = mods
    ext = pkg.ORBextractor(200, 1.2, 2, 20, 7)
    ext.set_lazy_level0(True)
    ora = O.OracleExtractor(200, 1.2, 2, 20, 7)
    stride = W + 9 if W % 2 == 0 else W + 8
    assert stride % 2 == 1
    for H in TINY_HEIGHTS:
        img = tiny_image(W, H, 100 * W + H)
        big = np.full((H + 4, stride), 0x5A, np.uint8)
        big[2:2 + H, 3:3 + W] = img
        d_big = torch.from_numpy(big).cuda()
        cap = ext.capacity(H, W)
        d_k = torch.zeros((1, cap, 7), dtype=torch.int32, device="cuda")
        d_d = torch.zeros((1, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_s = torch.zeros(1, dtype=torch.int32, device="cuda")
        ext.extract_batch_device(d_big.data_ptr() + 2 * stride + 3, 1, H, W, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(),
                                 d_s.data_ptr(), stride=stride, frame_stride=big.size)
        ext.sync()
        assert int(d_s.item()) == 0
        n = int(d_n.item())
        kps = d_k.cpu().numpy().view(pkg.KP_DTYPE).reshape(1, cap)[0, :n]
        okps, odesc = ora.extract(img)
        what = "%dx%d lazy" % (W, H)
        gx, gy, gs = ext.level_candidates(0)
        ox, oy, orr = ora.level_candidates(0)
        assert np.array_equal(gx, ox.astype(np.int32)) and np.array_equal(gy, oy.astype(np.int32)) \
            and np.array_equal(gs, orr.astype(np.int32)), what
        assert_kps_equal(kps, okps, what)
        assert np.array_equal(d_d.cpu().numpy()[0, :n], odesc), what
        assert len(ox) >= 5, what


@pytest.mark.gpu
def test_chunked_host_batch_second_chunk_at_a_nonzero_frame_slot(mods):
    """320 x 240, 8 levels, three different frames repeated to the 33 that the host entry runs as 16-frame chunks: the
    second and third chunk stage their cells from internal frame slots 16 and 32."""
    pkg, O = mods
    ext = pkg.ORBextractor(500, 1.2, 8, 20, 7)
    ora = O.OracleExtractor(500, 1.2, 8, 20, 7)
    uniq = [synth_frame(40 + s, 320, 240) for s in range(3)]
    res = ext.extract_batch(np.stack([uniq[b % 3] for b in range(33)]))
    for s in range(3):
        okps, odesc = ora.extract(uniq[s])
        for b in range(s, 33, 3):
            assert_kps_equal(res[b][0], okps, "frame %d" % b)
            assert np.array_equal(res[b][1], odesc), b
    ora.extract(uniq[32 % 3])
    for l in range(8):
        gx, gy, gs = ext.level_candidates(l, frame=32)
        ox, oy, orr = ora.level_candidates(l)
        assert np.array_equal(gx, ox.astype(np.int32)) and np.array_equal(gy, oy.astype(np.int32)) \
            and np.array_equal(gs, orr.astype(np.int32)), l


@pytest.mark.gpu
def test_headline_shape_pair_with_lazy_level0_equals_golden(mods):
    """A 1241 x 376 pair (stride-1241 rows: byte offsets 1, 2 and 3) with level 0 read from the image, against the
    committed oracle output for synth_frame(1) and the oracle itself for the second frame."""
    pkg, O = mods
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "extract_golden.npz"))
    gk = np.frombuffer(zlib.decompress(g["f_1_1241_376_1000_kps"].tobytes()), pkg.KP_DTYPE)
    gd = np.frombuffer(zlib.decompress(g["f_1_1241_376_1000_desc"].tobytes()), np.uint8).reshape(-1, 32)
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    ext.set_lazy_level0(True)
    pair = np.stack([synth_frame(1), synth_frame(2)])
    res = ext.extract_batch(pair)
    assert_kps_equal(res[0][0], gk, "frame 0")
    assert np.array_equal(res[0][1], gd)
    ora = O.OracleExtractor(1000, 1.2, 8, 20, 7)
    okps, odesc = ora.extract(pair[1])
    assert_kps_equal(res[1][0], okps, "frame 1")
    assert np.array_equal(res[1][1], odesc)
    for l in range(8):
        gx, gy, gs = ext.level_candidates(l, frame=1)
        ox, oy, orr = ora.level_candidates(l)
        assert np.array_equal(gx, ox.astype(np.int32)) and np.array_equal(gy, oy.astype(np.int32)) \
            and np.array_equal(gs, orr.astype(np.int32)), l


@pytest.mark.gpu
@pytest.mark.parametrize("kind,W,H,scale,nlev", [("checker3", 640, 480, 1.5, 4), ("noise", 333, 251, 1.2, 5)])
def test_dense_cells_still_run_in_row_bands(mods, kind, W, H, scale, nlev):
    """Images on which nearly every pixel passes the compass pre-test (the patterns of test_extractor_gpu.py): the first
    round of every cell overflows the survivor list -- larger now by what the staged image no longer takes, still far
    smaller than a cell -- and is repeated in row bands.  Same results from the plane and from the caller's image."""
    pkg, O = mods
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "checker3":
        img = ((((xx // 3) + (yy // 3)) & 1) * 180 + 40).astype(np.uint8)
    else:
        img = np.random.default_rng(19).integers(0, 256, (H, W), dtype=np.uint8)
    img = np.ascontiguousarray(img)
    ext = pkg.ORBextractor(3000, scale, nlev, 20, 7)
    ora = O.OracleExtractor(3000, scale, nlev, 20, 7)
    k, d = ext(img)
    ok, od = ora.extract(img)
    assert_stagewise_equal(ext, ora, nlev, kind)
    assert_kps_equal(k, ok, kind)
    assert np.array_equal(d, od)
    ext.set_lazy_level0(True)
    k2, d2 = ext(img)
    assert_kps_equal(k2, ok, kind + " (lazy level 0)")
    assert np.array_equal(d2, od)
