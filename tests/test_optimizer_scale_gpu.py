"""LocalBundleAdjustment, BundleAdjustment and OptimizeEssentialGraph on the device past one chunk, one grid and one tile
block, byte for byte against the references of optimizer_scale_cases.py, through the device form and the host form of the C ABI.
The outputs are full of sentinel bytes before a call, so what a call must not write is checked too, and every test first
checks on the reference's report that its case reaches the path it is named for.

Reference per case (REFERENCE in optimizer_scale_cases.py): tests/seqref for the cases marked seqref; the one-thread host
programs tests/cpp/{lba,gba,essgraph}_host.cpp for the others, which test_optimizer_scale_cpu.py pins to the seqref on every
case of the first kind.  The host program is sequential exactly where the device is parallel: the setup, the scans, the Schur
pairs, and an unblocked LDLt against the panel kernels.

Global adjustment
  pts, pts_perm, pts_null    1500 listed points (1108 included) in two chunks of k_gba_setup, every chunk with ordinary points,
                             points without a usable observation and points with observations skipped through maxKFid: the
                             carries of the point and edge scans, the counters across chunks; a permuted point list; null
                             vertices (device form only: the host form refuses them)
  pts_points_plus_one, pts_edges_plus_one   max_points / max_edges exceeded by one past the first chunk: only the report
  rows1100                   1100 listed rows, 38 good ones in both chunks, the row of mnId 0 in the second
  f70                        70 free poses: the second pass of k_gba_schur, block 1 of k_bwd_upd, seven trailing tile rows
  pivot                      a pivot that fails in the second panel on the first trial, on a workspace filled with 0xFF
  f250                       250 free poses: the strided cov zeroing of k_gba_index, 63 panels               (host program)
  e61k                       124 000 edges, 62 000 points over 41 rows: the second pass of every item loop, team sums of 480 edges
                             per lane; the first gain ratio is not clamped, so the trial's sum reaches the outputs  (host program)
  full512                    512 vertices, the capacity: 511 free poses, n = 3066; its reference takes 10 s    (host program)
Local adjustment
  pts1100                    1100 local points: the candidate and edge scans carry, erase rows and fixed cameras from the second chunk
  f40                        40 free poses: the edge-index wave loop past 16, the Schur loop past 1024 pairs
  f128, f129                 the capacity filled (128 free poses and the row of mnId 0; host program) and exceeded by one
  e31k                       64 000 edges, 32 000 points, 1 % gross outliers: the second pass of the item loops       (host program)
  (scene M of test_lba_cpu.py already crosses the K loop of k_lba_setup and the 1024 edges of k_lba_finish)
Essential graph
  rows1100                   40 good rows among 1100 in both chunks, the loop key frame in the second: the row scans of both passes
  e960                       991 edges over 46 free vertices: the team stride of k_eg_eval / k_eg_blocks, block 1 of k_bwd_upd;
                             again on the build with panels of 8 poses, in a child process (a process loads one build)
  pts1100                    pcap 1103: the point list and the point correction of k_eg_finish past one chunk
  f150                       150 free vertices, n = 1050                                                       (host program)
Left out on purpose: the full essential graph of 512 vertices (n = 3577 costs about 15 s per trial on the host) and more than
61 440 essential-graph edges."""
import os
import subprocess
import sys

import pytest

if __name__ == "__main__":                                                      # the child process of the panel-8 test
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import optimizer_scale_cases as C  # noqa: E402
import test_essgraph_cpu as KE  # noqa: E402
import test_gba_cpu as KG  # noqa: E402
import test_lba_cpu as KL  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = KL.ROOT
PANEL8 = os.path.join(ROOT, "tools", "_dev", "liborbhip_egpanel8.so")


def _make_env():
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd.matcher import make_camera
    m = pkg.ORBmatcher(0.6, True)
    cam = make_camera(*KL.CAM[:4], (0.0, 0.0, 1241.0, 376.0), [1.2 ** l for l in range(8)], mbf=KL.CAM[4])
    return dict(pkg=pkg, m=m, cam=cam)


@pytest.fixture(scope="module")
def env():
    e = _make_env()
    yield e
    e["m"].close()


# ---------------------------------------------------------------------------------------------------------------------
# global bundle adjustment
def _gba_device(env, name, what):
    import test_gba_gpu as DG
    b, ref = C.gba_case(name), C.gba_reference(name)
    KG.assert_same(DG.run_device(env, b), ref, what)
    syncs, launches = env["m"].GlobalBACounters()
    trials = int(ref["report"][10])
    assert syncs == 1 + trials + 1 and launches >= 4, (syncs, trials, launches)      # the relation test_gba_gpu.py asserts


@pytest.mark.parametrize("name", C.GBA_CASES)
def test_gba_device_form(env, name):
    C.gba_preconditions(name)
    _gba_device(env, name, name)


@pytest.mark.parametrize("name", [n for n in C.GBA_CASES if n != "pts_null"])
def test_gba_host_form(env, name):
    import test_gba_gpu as DG
    C.gba_preconditions(name)
    KG.assert_same(DG.run_host(env, C.gba_case(name)), C.gba_reference(name), name)


def test_gba_host_form_refuses_the_null_vertices(env):
    import test_gba_gpu as DG
    from orb_slam2_comment_amd import capi
    C.gba_preconditions("pts_null")
    with pytest.raises(capi.OrbHipError) as ei:
        DG.run_host(env, C.gba_case("pts_null"))
    assert ei.value.code == capi.E_ARG


def test_gba_failed_pivot_in_the_second_panel_on_a_filled_workspace(env):
    """The first run grows the slots; then every slot holds 0xFF (NaN, -1) when the first trial's factorisation fails in its
    second panel, so whatever a later launch of that trial reads without `due()` shows."""
    import test_gba_gpu as DG
    C.gba_preconditions("pivot")
    _gba_device(env, "pivot", "pivot, first run")
    assert env["m"].FillScratch(0xFF) > 0
    _gba_device(env, "pivot", "pivot, filled")
    env["m"].FillScratch(0xFF)
    KG.assert_same(DG.run_host(env, C.gba_case("pivot")), C.gba_reference("pivot"), "pivot, filled, host form")


# ---------------------------------------------------------------------------------------------------------------------
# local bundle adjustment
@pytest.mark.parametrize("name", C.LBA_CASES)
def test_lba_device_form(env, name):
    import test_lba_gpu as DL
    C.lba_preconditions(name)
    KL.assert_same(DL.run_device(env, C.lba_case(name)), C.lba_reference(name), name)


@pytest.mark.parametrize("name", C.LBA_CASES)
def test_lba_host_form(env, name):
    import test_lba_gpu as DL
    C.lba_preconditions(name)
    KL.assert_same(DL.run_host(env, C.lba_case(name)), C.lba_reference(name), name)


# ---------------------------------------------------------------------------------------------------------------------
# essential graph
def _eg_device(env, name):
    import test_essgraph_gpu as DE
    b, ref = C.eg_case(name), C.eg_reference(name)
    KE.assert_same(DE.run_device(env, b), ref, name)
    syncs, launches = env["m"].EssentialGraphCounters()
    assert syncs == 1 + int(ref["report"][9]) + 1 and launches > syncs, (syncs, launches)   # the relation test_essgraph_gpu.py asserts


@pytest.mark.parametrize("name", C.EG_CASES)
def test_eg_device_form(env, name):
    C.eg_preconditions(name)
    _eg_device(env, name)


@pytest.mark.parametrize("name", C.EG_CASES)
def test_eg_host_form(env, name):
    import test_essgraph_gpu as DE
    C.eg_preconditions(name)
    KE.assert_same(DE.run_host(env, C.eg_case(name)), C.eg_reference(name), name)


def test_eg_more_than_960_edges_on_the_build_with_panels_of_eight_poses():
    """Child process on the build with -DORBHIP_EG_PANEL=8 (make egpanel8): the panel is no part of the arithmetic."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:], file=sys.stderr)
    assert r.returncode == 0, "child failed with status %d" % r.returncode
    assert "panel 8: e960 ok" in r.stdout


def _child():
    import test_essgraph_gpu as DE
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"), "egpanel8"], check=True)
    from orb_slam2_comment_amd import capi
    capi.use_library(PANEL8)
    C.eg_preconditions("e960")
    assert int(C.eg_reference("e960")["report"][1]) - 1 > 4 * 8, "fewer than five panels of eight poses"
    env = _make_env()
    _eg_device(env, "e960")
    KE.assert_same(DE.run_host(env, C.eg_case("e960")), C.eg_reference("e960"), "e960 host form")
    env["m"].close()
    print("panel 8: e960 ok")


if __name__ == "__main__":
    _child()
