"""Pose optimisation on the device against the sequential reference (tests/seqref/poseopt.py), byte for byte.

The cases are built in test_poseopt_cpu.py and their reference answers are computed once per process: scenes A and B, a
batch with different edge counts (one frame with n = 0, one without any point), 65 edges (the second wavefront of the team
holds a single edge), 300 edges at cap = 512 (every wavefront busy, 44 lanes hold two edges), the nine-edge, two-edge and zero-depth cases, the three modes with their flags, world_row NULL and the per-frame
layout, and the same frame alone and inside a batch.  Every output, in/out array and report must equal the reference through
the device form and through the host form; what a call must not write keeps the sentinel the test put there."""
import numpy as np
import pytest

import test_poseopt_cpu as K

pytestmark = pytest.mark.gpu
f32, i32, u8 = np.float32, np.int32, np.uint8


@pytest.fixture(scope="module")
def env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(*K.CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=K.CAM[4])
    yield dict(pkg=pkg, m=m, cam=cam)
    m.close()


def run_device(env, b):
    import torch
    dev = torch.device("cuda")
    o = K.prefilled(b)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_in = [up(b[k]) for k in ("kps", "n", "u_right", "world", "point_flags", "world_row")]
    d_out = {k: up(o[k]) for k in o}
    torch.cuda.synchronize()
    env["m"].PoseOptimizationDevice(b["frames"], d_in[0], d_in[1], b["cap"], d_in[2], d_in[3], d_in[4], b["wrows"], b["pcap"], d_in[5],
                                    env["cam"], K.INV_SIGMA2, d_out["Tcw"], d_out["frame_point"], d_out["outlier"], d_out["discarded"],
                                    d_out["report"], mode=b["mode"], flags=b["flags"])
    env["m"].sync()
    return {k: d_out[k].cpu().numpy().view(o[k].dtype).reshape(o[k].shape) for k in o}


def run_host(env, b):
    o = K.prefilled(b)
    return env["m"].PoseOptimization(b["kps"], b["n"], b["u_right"], b["world"], b["point_flags"], b["world_row"], env["cam"],
                                     K.INV_SIGMA2, o["Tcw"], o["frame_point"], outlier=o["outlier"], mode=b["mode"], flags=b["flags"],
                                     fill=K.SENTINEL)


@pytest.mark.parametrize("name", K.CASES)
def test_device_equals_seqref(env, name):
    K.assert_same(run_device(env, K.case(name)), K.reference(name), name)


@pytest.mark.parametrize("name", K.CASES)
def test_host_form_equals_seqref(env, name):
    K.assert_same(run_host(env, K.case(name)), K.reference(name), name)


def test_frame_alone_equals_row_of_a_batch(env):
    alone, batch = run_device(env, K.case("A_alone")), run_device(env, K.case("batch3"))
    for k in ("report", "outlier", "frame_point", "Tcw", "discarded"):
        assert alone[k][0].tobytes() == batch[k][3].tobytes(), k


def test_plain_mode_without_optional_arrays(env):
    b = dict(K.case("B"), point_flags=None)
    got, ref = run_device(env, b), K.reference("B")
    K.assert_same(got, ref, "B without point_flags")
    import torch
    dev = torch.device("cuda")
    o = K.prefilled(b)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(u8).reshape(-1).copy()).to(dev)  # noqa: E731
    d = {k: up(o[k]) for k in ("Tcw", "frame_point", "outlier", "report")}
    d_in = [up(b[k]) for k in ("kps", "n", "world")]
    torch.cuda.synchronize()
    env["m"].PoseOptimizationDevice(1, d_in[0], d_in[1], b["cap"], None, d_in[2], None, 1, b["pcap"], None, env["cam"], K.INV_SIGMA2,
                                    d["Tcw"], d["frame_point"], d["outlier"], None, d["report"])
    env["m"].sync()
    for k in d:
        assert d[k].cpu().numpy().tobytes() == np.ascontiguousarray(ref[k]).tobytes(), k


def test_refusals_with_a_live_handle(env):
    from orb_slam2_comment_amd import capi
    b = K.case("A")
    for bad in (dict(mode=5), dict(flags=8)):
        with pytest.raises(capi.OrbHipError) as ei:
            run_host(env, dict(b, **bad))
        assert ei.value.code == capi.E_ARG
    fp = b["frame_point"].copy()
    fp[0, 0] = b["pcap"]
    with pytest.raises(capi.OrbHipError) as ei:
        run_host(env, dict(b, frame_point=fp))
    assert ei.value.code == capi.E_ARG
    empty = dict(b, frames=0, kps=b["kps"][:0], n=b["n"][:0], u_right=b["u_right"][:0], Tcw=b["Tcw"][:0], frame_point=b["frame_point"][:0])
    o = run_host(env, empty)                                                    # frames == 0: success, nothing written
    assert all(v.size == 0 for v in o.values())
