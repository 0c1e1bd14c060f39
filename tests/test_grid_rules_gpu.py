"""The frame-grid scene of grid_cases.py through every kernel that applies the grid rules (grid_cell, cell_window,
window_candidate, fuse_candidate in orbhip_matcher.hip), each compared for equality with the sequential reference:
AssignFeaturesToGrid (host and device entry), SearchByProjectionFrame / Points (16 lanes per query; the device entries keep
the invalid query inside the kernel), SearchForInitialization (64 lanes), SearchBestInWindow with and without the
chi-square gate, Fuse, and FuseBatch with one target on the camera's grid (the batch launch) and one on another grid (the
single-frame path)."""
import numpy as np
import pytest

import grid_cases as G

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    c = G.scene()
    views = {b: pkg.FrameView(c["k"], c["d"], G.SF, b, c["ur"]) for b in (G.BOUNDS, G.BOUNDS_OTHER)}
    return pkg, c, G.expected(), views


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i, np.nonzero(np.atleast_1d(g) != np.atleast_1d(w))[0][:8])


def _up(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,)).copy() if a.dtype.names else a.copy()).to("cuda:0")


def test_assign_features_to_grid_host_and_device(env):
    torch = pytest.importorskip("torch")
    pkg, c, want, views = env
    m, n = pkg.ORBmatcher(), len(c["k"])
    cap = n + 7
    d_k, d_n = _up(torch, np.concatenate([c["k"], np.zeros(7, c["k"].dtype)])[None]), _up(torch, np.array([n], np.int32))
    for bounds, name in ((G.BOUNDS, "grid"), (G.BOUNDS_OTHER, "grid_other")):
        _same(m.AssignFeaturesToGrid(views[bounds]), want[name], name)
        d_cell = torch.full((1, cap), -9, dtype=torch.int32, device="cuda:0")
        d_items = torch.full((1, cap), -9, dtype=torch.int32, device="cuda:0")
        d_start = torch.full((1, G.COLS * G.ROWS + 1), -9, dtype=torch.int32, device="cuda:0")
        m.AssignFeaturesToGridDevice(1, d_k.data_ptr(), d_n.data_ptr(), cap, bounds, d_cell.data_ptr(), d_start.data_ptr(),
                                     d_items.data_ptr())
        m.sync()
        cell_of, start, items = want[name]
        _same((d_cell.cpu().numpy()[0, :n], d_start.cpu().numpy()[0], d_items.cpu().numpy()[0, :len(items)]), want[name],
              name + " (device)")
        assert (d_cell.cpu().numpy()[0, n:] == -9).all() and (d_items.cpu().numpy()[0, len(items):] == -9).all()


def test_projection_searches_host_entries(env):
    pkg, c, want, views = env
    v = views[G.BOUNDS]
    for ori in (True, False):
        _same(pkg.ORBmatcher(0.9, ori).SearchByProjectionFrame(v, c["q"], c["qd"], c["taken"]), want["frame", ori], ("frame", ori))
    _same(pkg.ORBmatcher(G.NNRATIO, True).SearchByProjectionPoints(v, c["q"], c["qd"], c["taken"]), want["points"], "points")


def test_projection_searches_on_the_two_pass_grid_build(env):
    """The same scene behind 700 key points outside the grid: more than 1024 key points, so k_grid_build reads its keys
    twice instead of keeping them in registers; the answers are the scene's own."""
    pkg, c, _, _ = env
    k, d, ur, taken, want = G.padded(c)
    v = pkg.FrameView(k, d, G.SF, G.BOUNDS, ur)
    _same(pkg.ORBmatcher(0.9, False).SearchByProjectionFrame(v, c["q"], c["qd"], taken), want[0], "frame, two-pass grid")
    _same(pkg.ORBmatcher(G.NNRATIO, True).SearchByProjectionPoints(v, c["q"], c["qd"], taken), want[1], "points, two-pass grid")


def test_projection_searches_device_entries(env):
    """One pair, cap and qcap past the counts; the invalid query shares a 16-lane group's wavefront with valid ones."""
    torch = pytest.importorskip("torch")
    pkg, c, want, _ = env
    n, nq = len(c["k"]), len(c["q"])
    cap, qcap = n + 5, nq + 3
    pad = lambda a, m: np.concatenate([a, np.zeros((m - len(a),) + a.shape[1:], a.dtype)])[None]  # noqa: E731
    q = pad(c["q"], qcap)
    q["valid"][0, nq:] = 1                                # beyond nq: never looked at
    t_k, t_d, t_ur, t_tk = (_up(torch, pad(c[s], cap)) for s in ("k", "d", "ur", "taken"))
    t_q, t_qd = _up(torch, q), _up(torch, pad(c["qd"], qcap))
    t_n, t_nq = _up(torch, np.array([n], np.int32)), _up(torch, np.array([nq], np.int32))
    for mode, ori in (("frame", True), ("frame", False), ("points", True)):
        m = pkg.ORBmatcher(0.9 if mode == "frame" else G.NNRATIO, ori)
        t_a = torch.full((1, cap), -7, dtype=torch.int32, device="cuda:0")
        t_nm = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        fn = m.SearchByProjectionFrameDevice if mode == "frame" else m.SearchByProjectionPointsDevice
        fn(1, t_k.data_ptr(), t_d.data_ptr(), t_n.data_ptr(), cap, G.BOUNDS, t_q.data_ptr(), t_qd.data_ptr(), t_nq.data_ptr(),
           qcap, t_a.data_ptr(), t_nm.data_ptr(), d_u_right=t_ur.data_ptr(), d_taken=t_tk.data_ptr())
        m.sync()
        w = want["frame", ori] if mode == "frame" else want["points"]
        _same((int(t_nm.cpu().numpy()[0]), t_a.cpu().numpy()[0, :n]), w, (mode, ori, "device"))


@pytest.mark.parametrize("window", [8, 600])
def test_search_for_initialization_from_the_query_centres(env, window):
    pkg, c, want, views = env
    v1 = pkg.FrameView(c["k1"], c["qd"], G.SF, G.BOUNDS)
    prev = np.stack([c["q"]["u"], c["q"]["v"]], 1).astype(f32)
    _same(pkg.ORBmatcher(0.9, True).SearchForInitialization(v1, views[G.BOUNDS], prev, window), want["init", window], window)


@pytest.mark.parametrize("gate", [False, True], ids=["no gate", "chi-square gate"])
def test_search_best_in_window(env, gate):
    pkg, c, want, views = env
    got = pkg.ORBmatcher().SearchBestInWindow(views[G.BOUNDS], c["q"], c["qd"], G.INV_SIGMA2 if gate else None)
    _same(got, want["best", gate], gate)


@pytest.mark.parametrize("sim3_form", [False, True])
def test_fuse_and_fuse_batch(env, sim3_form):
    pkg, c, want, views = env
    m = pkg.ORBmatcher()
    pts = (c["X"], c["nrm"], c["max_d"], c["min_d"])
    for bounds, name in ((G.BOUNDS, "fuse"), (G.BOUNDS_OTHER, "fuse_other")):
        got = m.Fuse(views[bounds], c["cam"], c["T"], *pts, c["flags"], c["qd"], G.TH, G.INV_SIGMA2, sim3_form)
        _same(got, want[name, sim3_form], (name, sim3_form))
    bi, bd = m.FuseBatch([views[G.BOUNDS], views[G.BOUNDS_OTHER]], c["cam"], [c["T"]] * 2, *pts, np.stack([c["flags"]] * 2),
                         c["qd"], G.TH, G.INV_SIGMA2, sim3_form)
    _same((bi[0], bd[0]), want["fuse", sim3_form], ("batch launch", sim3_form))
    _same((bi[1], bd[1]), want["fuse_other", sim3_form], ("single-frame path", sim3_form))
