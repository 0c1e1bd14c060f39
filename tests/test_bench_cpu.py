"""bench.py --dump-outputs: the writer of the last timed step's outputs, on fabricated host arrays (no GPU)."""
import os

import numpy as np

import bench


def _outputs(B=512, cap=1500, seed=3):
    rng = np.random.default_rng(seed)
    n = rng.integers(600, cap + 1, B).astype(np.int32)
    kp = np.zeros((B, cap, 7), np.int32)
    kp[..., :5] = rng.uniform(0, 1000, (B, cap, 5)).astype(np.float32).view(np.int32)
    kp[..., 5] = rng.integers(0, 8, (B, cap))
    kp[..., 6] = -1
    d = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    a = rng.integers(-1, cap, (B // 2, cap)).astype(np.int32)
    m = rng.integers(100, 900, B // 2).astype(np.int32)
    st = np.zeros(B, np.int32)
    return kp, d, n, st, a, m


def test_dump_outputs_float32_bounded_and_reproducible(tmp_path):
    kp, d, n, st, a, m = _outputs()
    nb = bench.dump_outputs(str(tmp_path / "a"), kp, d, n, st, a, m)
    bench.dump_outputs(str(tmp_path / "b"), kp, d, n, st, a, m)
    assert nb <= bench.DUMP_LIMIT_BYTES
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(["keypoints", "descriptors", "match_assign", "sample_pairs", "keypoint_counts", "status",
                            "match_counts"])
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
    assert sum(v.nbytes for v in got.values()) == nb
    for k, v in got.items():
        assert v.dtype == np.float32, k
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))), k     # same inputs -> same files
    assert np.array_equal(got["keypoint_counts"], n) and np.array_equal(got["match_counts"], m)
    sample = got["sample_pairs"].astype(np.int64)
    assert len(sample) == bench.DUMP_PAIRS and np.all(np.diff(sample) > 0)
    for i, p in enumerate(sample[:5]):
        for j, f in enumerate((2 * p, 2 * p + 1)):
            c = n[f]
            assert np.array_equal(got["keypoints"][i, j, :c, :5], kp[f, :c, :5].view(np.float32))
            assert np.array_equal(got["keypoints"][i, j, :c, 5:], kp[f, :c, 5:])
            assert np.array_equal(got["descriptors"][i, j, :c], d[f, :c])
            assert not got["keypoints"][i, j, c:].any() and not got["descriptors"][i, j, c:].any()
        c = n[2 * p + 1]
        assert np.array_equal(got["match_assign"][i, :c], a[p, :c]) and np.all(got["match_assign"][i, c:] == -1)


def test_dump_outputs_shrinks_the_sample_to_the_limit(tmp_path):
    kp, d, n, st, a, m = _outputs(B=128, cap=4000)
    nb = bench.dump_outputs(str(tmp_path), kp, d, n, st, a, m)
    assert nb <= bench.DUMP_LIMIT_BYTES
    assert 0 < len(np.load(tmp_path / "sample_pairs.npy")) < bench.DUMP_PAIRS
