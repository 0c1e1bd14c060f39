"""k_octree keeps the candidates of a (level, frame) in registers when there are at most T * kOctR of them (512 threads x
8 keys = 4,096 for a KITTI-shape image; orbhip_extractor.hip) and in the HBM workspace otherwise.  Both paths, and the
boundary between them, against the oracle -- bit exact, as in test_extractor_gpu.py.

The workspace path can be forced for every workgroup only in the development build of the library
(`make -C orb_slam2_comment_amd/csrc dev`, orbhip_dev_set_octree_variant); a process can load one build only, so that case
runs this file as a script in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import assert_kps_equal, assert_stagewise_equal, synth_frame  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 1241, 376
REG_CAP = 512 * 8          # T * kOctR of the instantiation a 1241x376 image runs
BELOW, ABOVE = 5230, 5240  # fine-texture rectangles of dense_frame(1, .): 4,086 and 4,098 level-0 candidates


def dense_frame(seed, n_small):
    """synth_frame with its fine-texture density (3,000 small rectangles at this size) as a parameter."""
    from orb_slam2_comment_amd.synth import _render, _scene
    grid, shapes = _scene(seed, W, H, 400, 200, n_small)
    return _render(grid, shapes, W, H, False, (seed << 8) + 1)


def empty_left_frame():
    """No corner in the left 45 % of the image: the first initial node of every level is empty."""
    img = synth_frame(3, W, H).copy()
    img[:, :W * 45 // 100] = 128
    return img


def check_frame(pkg, O, img, what, k0_range=None, first_node_empty=False):
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    ora = O.OracleExtractor(1000, 1.2, 8, 20, 7)
    kps, desc = ext(img)
    okps, odesc = ora.extract(img)
    assert_stagewise_equal(ext, ora, 8, what)
    if k0_range is not None:
        # K of level 0 = the sum of its cells' survivor counts = the candidates the accessor returns
        k0 = len(ext.level_candidates(0)[0])
        print("%s: level-0 K = %d" % (what, k0))
        assert k0 == len(ora.level_candidates(0)[0])
        assert k0_range[0] <= k0 <= k0_range[1], (what, k0, k0_range)
    if first_node_empty:
        for l in range(8):
            x = ext.level_candidates(l)[0]
            cols = ext.image_pyramid(l).shape[1]
            assert len(x) > 100 and x.min() > cols / 3, (l, len(x), x.min(), cols)   # at most 4 initial nodes per level
    assert_kps_equal(kps, okps, what)
    assert np.array_equal(desc, odesc), what
    assert len(kps) >= 900
    return ext


def check_batch(pkg, O, what):
    """The 64-frame KITTI-shape batch of test_full_size_batch_properties; every distinct frame against the oracle."""
    import torch
    B = 64
    frames = np.stack([synth_frame(100 + (s % 8)) for s in range(B)])
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = ext.capacity(H, W)
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(frames).to(dev)
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    d_st = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ext.extract_batch_device(d_img.data_ptr(), B, H, W, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), d_st.data_ptr())
    ext.sync()
    assert np.all(d_st.cpu().numpy() == 0)
    n, kps, desc = d_n.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    ora = O.OracleExtractor(1000, 1.2, 8, 20, 7)
    for s in range(8):
        ok, od = ora.extract(frames[s])
        for b in range(s, B, 8):
            assert_kps_equal(kps[b, :n[b]].copy().view(pkg.KP_DTYPE).reshape(-1), ok, "%s frame %d" % (what, b))
            assert np.array_equal(desc[b, :n[b]], od), (what, b)
    return ext


@pytest.fixture(scope="module")
def mods(oracle):
    import orb_slam2_comment_amd as pkg
    return pkg, oracle


def test_level0_just_below_the_register_capacity(mods):
    check_frame(*mods, dense_frame(1, BELOW), "below", k0_range=(REG_CAP - 64, REG_CAP))


def test_level0_just_above_the_register_capacity(mods):
    """Level 0 goes through the workspace path, the other seven levels of the same frame through the registers."""
    check_frame(*mods, dense_frame(1, ABOVE), "above", k0_range=(REG_CAP + 1, REG_CAP + 64))


def test_empty_initial_node_shifts_the_labels(mods):
    check_frame(*mods, empty_left_frame(), "empty initial node", first_node_empty=True)


def test_workspace_path_forced_on_the_kitti_batch():
    """Child process on the development build: every workgroup through the workspace path -- the 64-frame batch, the two
    frames at the capacity boundary and the empty-initial-node frame; then the batch once more with the choice free."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:], file=sys.stderr)
    assert r.returncode == 0, "child failed with status %d" % r.returncode
    assert "forced workspace path: all cases equal the oracle" in r.stdout


def _child():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), "dev"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    from orb_slam2_comment_amd import capi
    capi.use_library(os.path.join(ROOT, "tools", "_dev", "liborbhip_dev.so"))
    import orb_slam2_comment_amd as pkg
    from oracle import oracle_py as O
    L = capi.lib()
    real_init = pkg.ORBextractor.__init__
    variant = [1]

    def init(self, *a, **k):                    # every handle the checks create gets the switch
        real_init(self, *a, **k)
        capi.check(L.orbhip_dev_set_octree_variant(self._h, variant[0]), "orbhip_dev_set_octree_variant")
    pkg.ORBextractor.__init__ = init
    check_batch(pkg, O, "workspace")
    check_frame(pkg, O, dense_frame(1, BELOW), "workspace, below", k0_range=(REG_CAP - 64, REG_CAP))
    check_frame(pkg, O, dense_frame(1, ABOVE), "workspace, above", k0_range=(REG_CAP + 1, REG_CAP + 64))
    check_frame(pkg, O, empty_left_frame(), "workspace, empty initial node", first_node_empty=True)
    print("forced workspace path: all cases equal the oracle")
    variant[0] = 0
    check_batch(pkg, O, "registers")
    print("development build, free choice: the batch equals the oracle")


if __name__ == "__main__":
    _child()
