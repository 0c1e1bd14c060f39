"""orbhip_fuse_device / orbhip_fuse_batch without a device: the symbols are exported and declared, and bad arguments are
refused before any device work.  The checks against a live handle and the oracle are in tests/test_fuse_batch_gpu.py."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    from orb_slam2_comment_amd import capi
    from orb_slam2_comment_amd.matcher import make_camera
    cam = make_camera(500.0, 500.0, 320.0, 240.0, (0, 0, 640, 480), [1.0, 1.2])
    a = dict(idx=np.zeros(2, np.int32), T=np.zeros((2, 12), np.float32), k=np.zeros((2, 8), capi.KP_DTYPE),
             d=np.zeros((2, 8, 32), np.uint8), n=np.zeros(2, np.int32), w=np.zeros((4, 3), np.float32),
             f4=np.zeros(4, np.float32), pd=np.zeros((4, 32), np.uint8), fl=np.zeros((2, 4), np.uint8),
             sig=np.ones(2, np.float32), bi=np.full((2, 4), -7, np.int32), bd=np.full((2, 4), -7, np.int32))
    return capi, cam, a


def _device(L, p, h, cam, a, K=2, cap=8, np_=4, pcap=4):
    return L.orbhip_fuse_device(h, K, p(a["idx"]), C.byref(cam), p(a["T"]), 0, p(a["k"]), p(a["d"]), p(a["n"]), cap, None, None,
                                None, np_, pcap, p(a["w"]), p(a["w"]), p(a["f4"]), p(a["f4"]), p(a["pd"]), p(a["fl"]), 3.0,
                                p(a["sig"]), p(a["bi"]), p(a["bd"]), None)


def test_fuse_batch_entries_refuse_bad_arguments_before_any_device_work():
    """No handle can be created without a device.  A null handle is ORBHIP_E_ARG; the other checks come before the handle
    is looked at, so a block of zero bytes stands in for it: were any of them to reach the device work, the call could not
    return the expected status."""
    capi, cam, a = _args()
    L, p = capi.lib(), capi.ptr
    assert _device(L, p, None, cam, a) == capi.E_ARG
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    assert _device(L, p, h, cam, a, K=-1) == capi.E_ARG
    assert _device(L, p, h, cam, a, np_=5, pcap=4) == capi.E_ARG
    assert _device(L, p, h, cam, a, np_=-1) == capi.E_ARG
    assert _device(L, p, h, cam, a, cap=0) == capi.E_ARG
    for levels in (0, 17):
        cam.n_levels = levels
        assert _device(L, p, h, cam, a) == capi.E_ARG
    cam.n_levels = 2
    assert _device(L, p, h, cam, a, cap=4097) == capi.E_CAPACITY
    assert b"4096" in L.orbhip_last_error()
    assert (a["bi"] == -7).all() and (a["bd"] == -7).all() and fake.raw == bytes(4096)
    # host entry
    view = capi.FrameView()
    arr = (C.POINTER(capi.FrameView) * 2)(C.pointer(view), C.pointer(view))

    def host(hh, K=2, n=4):
        return L.orbhip_fuse_batch(hh, K, arr, C.byref(cam), p(a["T"]), 0, n, p(a["w"]), p(a["w"]), p(a["f4"]), p(a["f4"]),
                                   p(a["fl"]), p(a["pd"]), 3.0, p(a["sig"]), p(a["bi"]), p(a["bd"]))
    assert host(None) == capi.E_ARG
    assert host(h, K=-1) == capi.E_ARG and host(h, n=-1) == capi.E_ARG
    cam.n_levels = 17
    assert host(h) == capi.E_ARG
    assert (a["bi"] == -7).all() and (a["bd"] == -7).all()


def test_mirrors_and_header_declare_the_batched_fuse():
    import orb_slam2_comment_amd as pkg
    for name in ("FuseDevice", "FuseBatch", "AssignFeaturesToGridDevice"):
        assert callable(getattr(pkg.ORBmatcher, name))
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    for sym in ("int orbhip_fuse_device(orbhip_matcher *m, int K,", "int orbhip_fuse_batch(orbhip_matcher *m, int K,"):
        assert sym in hdr
    for cite in ("src/ORBmatcher.cc:825-950", ":975-1075", "src/LocalMapping.cc:454-515", "src/LoopClosing.cc:585-610"):
        assert cite in hdr
    hpp = open(os.path.join(ROOT, "include", "orbhip", "ORBextractor.hpp")).read()
    for name in ("FuseDevice", "FuseBatch"):
        assert "void " + name + "(" in hpp
