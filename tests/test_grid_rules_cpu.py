"""The frame-grid scene of grid_cases.py on the CPU: building it runs the property asserts (every rounding tie, border
exit, strict edge and long list really occurs on the sequential reference), and the sequential reference must agree with
the C oracle wherever the oracle has the function."""
import numpy as np

import grid_cases as G
from seqref import matcher as SM
from seqref import projection as P


def test_scene_has_every_situation_it_claims():
    c = G.scene()
    assert len(c["k"]) <= 400 and len(c["q"]) <= 48
    G.expected()
    G.padded(c)


def _oracle_frame(oracle, c, bounds, keep):
    return oracle.make_frame(c["k"], c["d"], c["ur"], bounds, G.SF, keep)


def test_grid_and_windows_equal_the_oracle(oracle):
    c, keep = G.scene(), []
    for bounds, name in ((G.BOUNDS, "grid"), (G.BOUNDS_OTHER, "grid_other")):
        O = _oracle_frame(oracle, c, bounds, keep)
        for got, want in zip(oracle.assign_features_to_grid(O), G.expected()[name]):
            assert np.array_equal(got, want), name
    O, q = _oracle_frame(oracle, c, G.BOUNDS, keep), c["q"]
    for i in range(len(q)):
        a = (q["u"][i], q["v"][i], q["radius"][i], int(q["min_level"][i]), int(q["max_level"][i]))
        assert np.array_equal(oracle.features_in_area(O, *a), SM.features_in_area(c["S"], *a)), i


def test_searches_equal_the_oracle(oracle):
    c, w, keep = G.scene(), G.expected(), []
    O, q, qd = _oracle_frame(oracle, c, G.BOUNDS, keep), c["q"], c["qd"]
    for ori in (True, False):
        n, a = oracle.search_by_projection_frame(O, q, qd, c["taken"], ori)
        assert n == w["frame", ori][0] and np.array_equal(a, w["frame", ori][1]), ori
    n, a = oracle.search_by_projection_points(O, q, qd, c["taken"], G.NNRATIO)
    assert n == w["points"][0] and np.array_equal(a, w["points"][1])
    G.init_frame(c)
    O1 = oracle.make_frame(c["k1"], qd, None, G.BOUNDS, G.SF, keep)
    prev = np.stack([q["u"], q["v"]], 1).astype(np.float32)
    for window in (8, 600):
        n, m12, pm = oracle.search_for_initialization(O1, O, prev, window, 0.9, True)
        sn, sm12, spm = w["init", window]
        assert n == sn and np.array_equal(m12, sm12) and np.array_equal(pm, spm), window


def test_best_in_window_and_fuse_prologue_equal_the_oracle(oracle):
    c, w, keep = G.scene(), G.expected(), []
    q, qd = c["q"], c["qd"]
    for bounds, name in ((G.BOUNDS, "fuse"), (G.BOUNDS_OTHER, "fuse_other")):
        O = _oracle_frame(oracle, c, bounds, keep)
        if name == "fuse":
            for gate in (False, True):
                bi, bd = oracle.search_best_in_window(O, q, qd, G.INV_SIGMA2 if gate else None)
                assert np.array_equal(bi, w["best", gate][0]) and np.array_equal(bd, w["best", gate][1]), gate
        for sim3 in (False, True):
            args = (c["T"], None, c["X"], c["nrm"], c["max_d"], c["min_d"], c["flags"], G.TH)
            qf = oracle.keyframe_queries(c["cam"], 0, sim3, *args)
            sq = P.keyframe_queries(c["scam"], 0, sim3, *args)
            for f in ("valid", "u", "v", "radius", "min_level", "max_level", "ur", "level_aux"):
                assert np.array_equal(qf[f], sq[f]), f
            bi, bd = oracle.search_best_in_window(O, qf, qd, None if sim3 else G.INV_SIGMA2)
            assert np.array_equal(bi, w[name, sim3][0]) and np.array_equal(bd, w[name, sim3][1]), (name, sim3)
