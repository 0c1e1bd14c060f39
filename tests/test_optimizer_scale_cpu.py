"""The optimiser cases past one chunk, one grid and one tile block (optimizer_scale_cases.py), without a GPU: the table of
kernel-private sizes against the sources it quotes, the precondition of every case on its reference's report, and the one-thread
host build of each shared core against tests/seqref, byte for byte on every output, on every case whose reference is the seqref.
Those are the cases that cross the chunk thresholds (more than 1024 points, rows or edges per pass), the wave-loop thresholds
(40 free poses in the local, 70 in the global adjustment, more than 960 essential-graph edges) and a pivot that fails in the
second panel; they are what makes the host program a sound reference for the larger cases of test_optimizer_scale_gpu.py, where
the seqref is too slow (REFERENCE in optimizer_scale_cases.py says which case has which).

Measured on the CPU: the host reference of the capacity case of the global adjustment (full512: 512 vertices, 511 free poses,
n = 3066, one iteration with one trial) takes 10 s, of which the compilation of the host program is 1.5 s; f250 0.9 s; e61k 1.4 s
with the run that reads its first gain ratio; the local adjustment's f128 1.1 s and e31k 1.6 s; the essential graph's f150 2.7 s.
The slowest seqref references are the essential graph's e960 (6 s: 991 edges with 29 evaluations each per linearisation) and the
local adjustment's pts1100 and f40 (4 s each, with the LDLt's trailing update in numpy: see lba_reference)."""
import os
import re

import numpy as np
import pytest

import optimizer_scale_cases as C
import test_essgraph_cpu as KE
import test_gba_cpu as KG
import test_lba_cpu as KL
from orb_slam2_comment_amd import capi
from seqref import essgraph as E
from seqref import gba as G
from seqref import lba as L

CSRC = os.path.join(KL.ROOT, "orb_slam2_comment_amd", "csrc")
ALL = [(kind, name) for kind in ("gba", "lba", "eg") for name in C.REFERENCE[kind]]
SEQREF = [(kind, name) for kind, name in ALL if C.REFERENCE[kind][name] == "seqref"]


def _constant(path, name):
    text = open(os.path.join(CSRC, path)).read()
    m = re.search(r"constexpr int [^;]*\b%s = ([A-Za-z0-9_ */+-]+?)[,;]" % name, text)
    assert m, "%s: no constexpr int %s" % (path, name)
    return m.group(1).strip()


def test_the_table_of_sizes_is_what_the_sources_say():
    want = [("orbhip_gba.hip", "kBig", C.CHUNK), ("orbhip_essgraph.hip", "kBig", C.CHUNK), ("orbhip_lba.hip", "kSetupThreads", C.CHUNK),
            ("orbhip_gba.hip", "kItem", C.ITEM), ("orbhip_essgraph.hip", "kItem", C.ITEM), ("orbhip_lba.hip", "kItemThreads", C.ITEM),
            ("orbhip_ldlt.h", "kItem", C.ITEM), ("orbhip_ldlt.h", "kTile", C.TILE), ("orbhip_lba_core.h", "kLbaWave", C.WAVE),
            ("orbhip_essgraph_core.h", "kEgWave", C.WAVE), ("orbhip_lba.hip", "kItemBlocks", C.LBA_ITEM_BLOCKS),
            ("orbhip_lba.hip", "kSchurBlocks", C.LBA_SCHUR_BLOCKS), ("orbhip_gba.hip", "kItemBlocks", C.GBA_ITEM_BLOCKS),
            ("orbhip_gba.hip", "kSchurBlocks", C.GBA_SCHUR_BLOCKS), ("orbhip_essgraph.hip", "kItemBlocks", C.EG_ITEM_BLOCKS)]
    for path, name, value in want:
        assert _constant(path, name) == str(value), (path, name)
    assert _constant("orbhip_gba_core.h", "kGbaPanel") == str(C.GBA_NB // 6) and _constant("orbhip_gba_core.h", "kGbaNb") == "6 * kGbaPanel"
    assert _constant("orbhip_essgraph_core.h", "kEgNb") == "7 * kEgPanel" and C.EG_NB == 7 * 4
    assert re.search(r"#define ORBHIP_EG_PANEL 4\b", open(os.path.join(CSRC, "orbhip_essgraph_core.h")).read())
    assert (capi.LBA_MAX_LOCAL, capi.GBA_MAX_KF, capi.EG_MAX_KF) == (L.MAX_LOCAL, G.MAX_KF, E.MAX_KF)
    # the thresholds the docstrings of the cases quote
    assert (C.LBA_ITEMS, C.GBA_ITEMS, C.LBA_SCHUR_WAVES, C.GBA_SCHUR_WAVES, C.EG_TEAMS, C.LBA_SETUP_WAVES) == (30720, 61440, 1024, 4096, 960, 16)
    assert C.bwd_block1_free(C.GBA_NB, 6) == 45 and C.bwd_block1_free(C.EG_NB, 7) == 41


@pytest.mark.parametrize("kind,name", ALL)
def test_the_case_reaches_what_it_is_named_for(kind, name):
    getattr(C, kind + "_preconditions")(name)


def test_every_listed_case_has_a_reference_and_the_refusals_keep_their_sentinels():
    assert C.GBA_CASES == list(C.REFERENCE["gba"]) and C.LBA_CASES == list(C.REFERENCE["lba"]) and C.EG_CASES == list(C.REFERENCE["eg"])
    for name in ("pts_points_plus_one", "pts_edges_plus_one"):
        b, r = C.gba_case(name), C.gba_reference(name)
        o = KG.prefilled(b)
        for k in ("TcwGBA", "posGBA", "kf_mark", "pt_mark", "point_list"):
            assert np.ascontiguousarray(r[k]).tobytes() == o[k].tobytes(), (name, k)
        assert r["report"][9] == 0 and r["report"][10] == 0
    b, r = C.lba_case("f129"), C.lba_reference("f129")
    o = KL.prefilled(b)
    for k in ("local_kf", "fixed_kf", "local_point", "erase"):
        assert r[k].tobytes() == o[k].tobytes(), k
    assert r["Tcw"].tobytes() == b["tables"]["Tcw"].tobytes() and r["world"].tobytes() == b["tables"]["world"].tobytes()


def run_host_program(kind, name, tmp_path, fill=0):
    if kind == "gba":
        return KG.run_host(C.gba_case(name), tmp_path, name, fill=fill)
    if kind == "lba":
        return KL.run_host(C.lba_case(name), tmp_path, name, fill=fill)
    return KE.run_host(C.eg_case(name), tmp_path, name, fill=fill)


def assert_same(kind, got, ref, what):
    {"gba": KG.assert_same, "lba": KL.assert_same, "eg": KE.assert_same}[kind](got, ref, what)


@pytest.mark.parametrize("kind,name", SEQREF)
def test_host_build_matches_seqref(kind, name, tmp_path):
    assert_same(kind, run_host_program(kind, name, tmp_path), getattr(C, kind + "_reference")(name), name)


@pytest.mark.parametrize("fill", [0xA5, 0xFF])
def test_host_build_with_a_failed_pivot_in_the_second_panel_on_a_filled_workspace(fill, tmp_path):
    assert_same("gba", run_host_program("gba", "pivot", tmp_path, fill=fill), C.gba_reference("pivot"), "pivot")


def test_bulk_observe_is_scene_observe():
    """The same observations through Scene.observe and through bulk_observe: the same tables but for the noise drawn."""
    def scene():
        sc = KL.Scene(3, 8, 4, 5)
        KL._line_of_cameras(sc, range(3))
        for X in ([0.5, 0.1, 9.0], [1.0, -0.3, 7.0], [0.2, 0.4, 12.0], [1.5, 0.0, 8.0]):
            sc.point(X)
        return sc
    pts, rows, stereo = [0, 0, 1, 2, 2, 2, 3], [0, 2, 1, 0, 1, 2, 1], [False, True, True, False, False, True, False]
    a, b = scene(), scene()
    for p, r, s in zip(pts, rows, stereo):
        a.observe(p, r, stereo=s, noise=0.0)
    C.bulk_observe(b, pts, rows, stereo, noise=0.0)
    assert a.obs == b.obs and a.n.tolist() == b.n.tolist() and np.array_equal(a.slot_point, b.slot_point)
    for r in range(3):
        k = int(a.n[r])
        assert np.allclose(a.kps["x"][r, :k], b.kps["x"][r, :k], rtol=0, atol=1e-3) and np.allclose(a.kps["y"][r, :k], b.kps["y"][r, :k], rtol=0, atol=1e-3)
        assert np.allclose(a.ur[r, :k], b.ur[r, :k], rtol=0, atol=1e-3) and np.array_equal(a.ur[r, :k] < 0, b.ur[r, :k] < 0)
