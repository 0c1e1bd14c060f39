"""The map-maintenance cases at real bank sizes (map_scale_cases.py), without a GPU: the table of kernel-private sizes against
the sources it quotes, the precondition of every case on its reference alone, that every threshold of the table is crossed
by some case, the fast graph conversion against seqref's own, and that the scenes of test_covisibility_cpu.py,
test_localmap_cpu.py and test_culling_cpu.py (whose cull_scene gained parameters for these cases) are what they were.

Reference time per case, one CPU thread, scene included (paid once per session): cv_blocks2 0.01 s, cv_blocks8 0.25 s (its
host-entry list 0.1 s more), cv_wide 0.05 s, cv_full4096 0.8 s, the reader lists 0.6 s for the eight of them, children 0.01 s,
lm_rows1100 0.15 s, lm_cap4096 0.3 s, lm_rows65536 0.05 s, cu_rows1100 1.2 s, cu_full4096 6 s (UpdateConnections of 4096 rows
in cull_scene and the rows x rows loop of Graph.from_dense in reference_key_frames), upd_long 1.9 s."""
import ctypes
import hashlib
import os
import re
import types

import numpy as np
import pytest

import map_scale_cases as C
import test_covisibility_cpu as CC
import test_culling_cpu as KC
import test_localmap_cpu as LC
from seqref import covisibility as CV

CSRC = os.path.join(CC.ROOT, "orb_slam2_comment_amd", "csrc")


def _source(path):
    return open(os.path.join(CSRC, path)).read()


def _constant(path, name):
    m = re.search(r"constexpr int %s = ([A-Za-z0-9_ */+-]+?);" % name, _source(path))
    assert m, "%s: no constexpr int %s" % (path, name)
    return m.group(1).strip()


def test_the_table_of_sizes_is_what_the_sources_say():
    want = [("orbhip_covisibility.hip", "kCvGroup", C.GROUP), ("orbhip_localmap.hip", "kLmGroup", C.GROUP),
            ("orbhip_culling.hip", "kCuGroup", C.GROUP), ("orbhip_covisibility.hip", "kCvMaxRows", C.CV_MAX_ROWS),
            ("orbhip_culling.hip", "kCuMaxRows", C.CU_MAX_ROWS), ("orbhip_covisibility.hip", "kCvTh", C.CV_TH),
            ("orbhip_localmap.hip", "kLmPosBlocks", C.LM_POS_BLOCKS), ("orbhip_localmap.hip", "kLmMaxKf", C.LM_MAX_KF),
            ("orbhip_matcher.hip", "kUpdLongBlocks", C.UPD_LONG_BLOCKS), ("orbhip_matcher.hip", "kUpdGroup", C.UPD_GROUP)]
    for path, name, value in want:
        assert _constant(path, name) == str(value), (path, name)
    assert _constant("orbhip_localmap.hip", "kLmStampWords") == "%d / 32" % C.LM_MAX_ROWS
    assert "slot_blocks = std::max(1, std::min(%d, (A.cap + %d) / %d));" % (C.CV_MAX_BLOCKS, C.CV_BLOCK_SLOTS - 1, C.CV_BLOCK_SLOTS) \
        in _source("orbhip_covisibility.hip")
    assert "slot_blocks = std::max(1, std::min(%d, (A.cap + %d) / %d));" % (C.CU_MAX_BLOCKS, C.CU_BLOCK_SLOTS - 1, C.CU_BLOCK_SLOTS) \
        in _source("orbhip_culling.hip")
    for path, kernels in (("orbhip_covisibility.hip", ("k_cv_counters", "k_cv_summary", "k_cv_apply", "k_cv_children")),
                          ("orbhip_localmap.hip", ("k_lm_votes", "k_lm_keyframes", "k_lm_first", "k_lm_points", "k_lm_scan")),
                          ("orbhip_culling.hip", ("k_kf_apply", "k_kf_step"))):
        for k in kernels:
            assert re.search(r"__launch_bounds__\(%d\) void %s\(" % (C.WG, k), _source(path)), k
    assert re.search(r"__launch_bounds__\(%d\) void k_cv_targets\(" % C.WAVE, _source("orbhip_covisibility.hip"))
    assert re.search(r"__launch_bounds__\(%d\) void k_update_points_long\(" % C.WAVE, _source("orbhip_matcher.hip"))
    assert [C.cv_slot_blocks(c) for c in (64, 128, 129, 256, 896, 897, 2048, 4096)] == [1, 1, 2, 2, 7, 8, 8, 8]
    assert [C.cu_slot_blocks(c) for c in (64, 256, 257, 1536, 4096)] == [1, 1, 2, 6, 16]
    assert [C.sort_size(r) for r in (1, 2, 3, 512, 513, 1100, 4096)] == [2, 2, 4, 512, 1024, 2048, 4096]
    assert C.where(200) == (0, 3, 8) and C.where(516) == (2, 0, 4) and C.where(556) == (2, 0, 44) and C.where(453) == (1, 3, 5)


@pytest.mark.parametrize("name", C.CASES)
def test_the_case_reaches_what_it_is_named_for(name):
    C.preconditions(name)


@pytest.mark.parametrize("case,nn,nn2", C.TARGET_CASES, ids=lambda v: str(v))
def test_the_reader_lists_are_as_long_as_the_case_says(case, nn, nn2):
    C.target_preconditions(case, nn, nn2)


def test_every_threshold_is_crossed_and_no_case_is_left_out():
    crossed = {t for ts in C.CROSSES.values() for t in ts}
    assert crossed == set(C.THRESHOLDS), (crossed ^ set(C.THRESHOLDS))
    assert C.CASES == list(C.CROSSES) and all(C.CROSSES[n] for n in C.CASES)
    # what the GPU module runs, from its parametrize marks; no test of it carries another mark than parametrize and gpu
    import test_map_scale_gpu as GM
    import test_mappoint_gpu as MG
    tests = {k: v for k, v in vars(GM).items() if k.startswith("test_") and callable(v)}

    def params(fn):
        marks = getattr(fn, "pytestmark", [])
        assert all(m.name == "parametrize" for m in marks), (fn.__name__, [m.name for m in marks])
        return [v for m in marks for v in m.args[1]]
    assert GM.pytestmark.name == "gpu"
    device = set(params(tests["test_update_connections_device_equals_seqref"])) | set(params(tests["test_update_local_map_device_equals_seqref"])) \
        | set(params(tests["test_cull_key_frames_device_equals_seqref"]))
    assert device == set(C.CASES) - {"children", "upd_long"}, device ^ set(C.CASES)
    assert params(tests["test_children_from_parents"]) == ["rows4096", "rows1025"]
    assert params(tests["test_covisible_targets_equal_seqref"]) == C.TARGET_CASES
    assert set(params(tests["test_update_connections_host_entry_equals_seqref_and_the_device_entry"])) >= {"cv_blocks8_host"}
    assert params(tests["test_second_run_after_the_scratch_is_filled_with_a5"]) == ["cv_blocks8", "lm_rows1100", "cu_rows1100"]
    for name in ("test_update_local_map_host_entry_equals_seqref_and_the_device_entry", "test_track_local_map_equals_the_three_entries",
                 "test_cull_map_points_device_equals_seqref", "test_cull_host_entries_equal_seqref"):
        assert params(tests[name]) == []
    assert params(MG.test_more_long_points_than_workgroups_of_the_worklist_kernel) == []


def test_the_fast_graph_conversion_is_from_dense():
    for name in (("random", 65), ("strides", 40)):
        S = CC.scene_and_reference(name)
        for A in (S["state"], S["out"]):
            G, H = CV.Graph.from_dense(A), C.graph_from_dense(A)
            assert (G.conn, G.ord_kf, G.ord_w, G.first_conn, G.parent) == (H.conn, H.ord_kf, H.ord_w, H.first_conn, H.parent)
            assert all(type(v) is int for c in H.conn for kv in c.items() for v in kv) and all(type(v) is int for l in H.ord_kf for v in l)
        out, rep, touched = C.run_reference(S["T"], S["state"], S["upd"], S["id0"])
        assert touched == S["touched"] and np.array_equal(rep, S["report"])
        assert all(np.array_equal(out[k], S["out"][k]) for k in S["out"])


def test_cv_tables_gives_the_counts_it_is_asked_for():
    T, state = C.cv_tables(12, 32, [(3, {0: 4, 5: 7, 11: 7}, 2), (5, {1: 2}, 1)], 1)
    out, rep, _ = C.run_reference(T, state, [3, 5], -1)
    assert out["conn_w"][3].tolist() == [4, 0, 0, 0, 0, 7, 0, 0, 0, 0, 0, 7]
    assert out["conn_w"][5][1] == 2 and out["conn_w"][5][3] == 7          # and what it shares with the other rows of row 3's points
    assert rep[0].tolist()[:5] == [CV.OK, 3, 1, 5, 7] and (T["flags"][:T["np"]] == 0).sum() == 10


# ---- the scenes of the three modules are what they were -------------------------------------------------------------------------
def _feed(h, obj):
    if isinstance(obj, np.ndarray):
        a = np.ascontiguousarray(obj)
        h.update(("A%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    elif isinstance(obj, dict):
        for k in sorted(obj, key=repr):
            h.update(("K%r" % (k,)).encode())
            _feed(h, obj[k])
    elif isinstance(obj, (list, tuple)):
        h.update(("L%d" % len(obj)).encode())
        for x in obj:
            _feed(h, x)
    elif isinstance(obj, (set, frozenset)):
        _feed(h, sorted(obj))
    elif isinstance(obj, (int, float, str, bool, type(None), np.integer, np.floating)):
        h.update(("S%r" % (obj,)).encode())
    elif isinstance(obj, ctypes.Structure):
        h.update(("C%s" % type(obj).__name__).encode())
        h.update(bytes(obj))
    elif isinstance(obj, types.SimpleNamespace):
        h.update(b"N")
        _feed(h, vars(obj))
    else:
        raise TypeError("a cached scene holds a %s, which the digest does not know how to read" % type(obj).__name__)


def digest(obj):
    """Every array (type, shape, bytes), number and name of a cached scene_and_reference result."""
    h = hashlib.sha256()
    _feed(h, obj)
    return h.hexdigest()[:16]


# of the scenes as the commit before cull_scene gained cap, big_at and hub_row builds them
DIGESTS = {
    "cv random-1": "b2e3f1a63ac519ca", "cv random-2": "e0dd0638d3383020", "cv random-63": "e3bd7ccfff4e625d",
    "cv random-64": "156a26f467bfda05", "cv random-65": "5900e83b3fa60d50", "cv random-257": "f51d16880d510412",
    "cv strides-40": "8ee76d61772b14ce", "lm A": "179586f4d6f7b3f2", "lm B": "c2fde0af7d9a44ea", "lm C": "3ed9b14337d28783",
    "cu r2": "49f1faa0389b7e28", "cu r12": "6443ceed69ad3fc9", "cu r65": "7d31c41d127fd364", "cu r257": "8c732c3247d83e99"}


def test_the_existing_scenes_are_unchanged():
    got = {}
    for n in [("random", r) for r in (1, 2, 63, 64, 65, 257)] + [("strides", 40)]:
        got["cv %s-%d" % n] = digest(CC.scene_and_reference(n))
    for n in LC.SCENES:
        got["lm " + n] = digest(LC.scene_and_reference(n))
    for n in KC.GPU_SCENES:
        got["cu " + n] = digest(KC.scene_and_reference(n))
    assert got == DIGESTS
