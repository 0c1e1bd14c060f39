"""Every stage of the matcher handle against its reference on a workspace that is not what a fresh handle finds.

The handle's 30 scratch slots are allocated uninitialised, grow only, and are carved by the sizes of the call, so in a
running system every call starts on the bytes an earlier call of other sizes left behind.  The stage modules run their
cases on a fresh handle in one fixed order; here ONE handle serves the whole file and every stage ("The
matcher's scratch slots") goes through three protocols on it:

  filled    the case once (the warm-up grows the slots), then after FillScratch(0xFF) (floats NaN, ints -1) and after
            FillScratch(0xA5) (ints large and negative, floats finite garbage): every run must equal the same reference,
            sentinel regions included.  A stage that owns a slot must have grown it: FillScratch reports more bytes after
            the warm-up of its largest case than before.
  residue   the stage's largest case, its smallest, the smallest, the largest, with no fill in between: live values of a
            call of other sizes under fields whose offsets moved.
  cross     one small case per stage round the table, FillScratch(0xFF), then round again in reverse: the only protocol
            that reuses S_OUT, S_MISC, S_ORD, S_CNT, S_CAND, S_CSR and S_Q across stages with different layouts.

Nothing is restated here: a case is a call of what the stage's own modules already have -- the case builders and cached
references of test_*_cpu.py, the run / check helpers and the test bodies of test_*_gpu.py -- with the shared handle in
the place of theirs.  `SharedPkg` hands every `pkg.ORBmatcher(nnratio, ori)` of such a body a view of the shared handle
(the two settings live in the Python object, not in the handle); `FillBetween` fills the workspaces between a solver's
setup and each of its iterate calls.  The count assertions of the bodies (GlobalBACounters: syncs == 1 + trials + 1, the
essential graph's one synchronisation per trial) therefore hold after a fill as well."""
import numpy as np
import pytest

import bow_cases as Cs
import test_covisibility_gpu as CG
import test_culling_gpu as KG
import test_essgraph_gpu as EG
import test_fuse_batch_gpu as FB
import test_gba_gpu as GG
import test_lba_cpu as LBK
import test_lba_gpu as LG
import test_localmap_gpu as MG
import test_mappoint_gpu as PG
import test_matcher_gpu as TM
import test_pnp_gpu as NG
import test_poseopt_cpu as POK
import test_poseopt_gpu as OG
import test_projection_gpu as TP
import test_seqref_bow_gpu as SB
import test_seqref_gpu as TS
import test_seqref_projection_cpu as PC
import test_seqref_projection_gpu as SP
import test_sim3_gpu as RG
import test_sim3opt_gpu as SG
import test_stereo_cases_gpu as TC
import test_triangulate_gpu as TR
import test_window_search_groups_gpu as WG
from seqref import mappoint as MP
from seqref import matcher as SM
from seqref import pnp as PNP
# the stage modules' own fixtures, under names of this module: their cameras, uploaded banks and cached expectations
from test_essgraph_gpu import env as eg_env  # noqa: F401
from test_fuse_batch_gpu import env as fuse_batch_env  # noqa: F401
from test_gba_gpu import env as gba_env  # noqa: F401
from test_lba_gpu import env as lba_env  # noqa: F401
from test_mappoint_gpu import env as mappoint_env  # noqa: F401
from test_pnp_gpu import env as pnp_env  # noqa: F401
from test_poseopt_gpu import env as poseopt_env  # noqa: F401
from test_sim3_gpu import env as sim3_env  # noqa: F401
from test_sim3opt_gpu import env as sim3opt_env  # noqa: F401
from test_triangulate_gpu import env as triangulate_env  # noqa: F401

pytestmark = pytest.mark.gpu

BYTES = (0xFF, 0xA5)


class SharedPkg:
    """The package with ORBmatcher(nnratio, ori) answered by a view of one shared handle."""

    def __init__(self, pkg, base):
        self._pkg, self._base = pkg, base

    def __getattr__(self, name):
        return getattr(self._pkg, name)

    def ORBmatcher(self, nnratio=0.6, checkOri=True, device=0):
        base = self._base

        class View(type(base)):
            def __init__(self):
                self._lib, self._h = base._lib, base._h
                self.mfNNratio, self.mbCheckOrientation = float(nnratio), bool(checkOri)

            def close(self):                                    # the handle is the file's, not the view's
                pass
        return View()


class FillBetween:
    """A matcher whose solver iterations each start on filled workspaces: what setup left in the handle is gone."""

    def __init__(self, m, byte):
        self._m, self._byte = m, byte

    def __getattr__(self, name):
        return getattr(self._m, name)

    def Sim3Iterate(self, *a, **k):
        self._m.FillScratch(self._byte)
        return self._m.Sim3Iterate(*a, **k)

    def PnpIterate(self, *a, **k):
        self._m.FillScratch(self._byte)
        return self._m.PnpIterate(*a, **k)


@pytest.fixture(scope="module")
def ctx(oracle, eg_env, fuse_batch_env, gba_env, lba_env, mappoint_env, pnp_env, poseopt_env, sim3_env, sim3opt_env, triangulate_env):
    import torch
    import orb_slam2_comment_amd as pkg
    from orb_slam2_comment_amd import matcher as M
    m = pkg.ORBmatcher(0.6, True)
    shared = SharedPkg(pkg, m)
    on = lambda env: dict(env, m=m, pkg=shared)  # noqa: E731
    plain = dict(pkg=shared, torch=torch, dev=torch.device("cuda:0"), m=m)
    PC.key_frames(oracle)
    tri = dict(triangulate_env, pkg=shared, m0=shared.ORBmatcher(0.6, False), m1=shared.ORBmatcher(0.6, True))
    tri["run"] = TR.Run(tri)
    c = dict(m=m, pkg=shared, torch=torch, M=M, O=oracle, tup2=(shared, M), tup3=(shared, M, oracle), plain=plain,
             seqproj=dict(plain, O=oracle, G=SP.DeviceAsOracle(shared, oracle)), fuse_batch=on(fuse_batch_env), tri=tri,
             mappoint=on(mappoint_env), sim3=on(sim3_env), pnp=on(pnp_env), poseopt=on(poseopt_env), sim3opt=on(sim3opt_env),
             lba=on(lba_env), eg=on(eg_env), gba=on(gba_env), between=None, init_want=[],
             bow={x["name"]: x for x in Cs.bow_constructed_cases() + Cs.bow_random_cases()},
             trs={x["name"]: x for x in Cs.tri_constructed_cases() + Cs.tri_random_cases()})
    yield c
    m.close()


# ---- the stages ---------------------------------------------------------------------------------------------------------
class Stage:
    """cases: [(id, run(ctx))], the smallest first and the largest last; a run raises unless every output equals its
    reference.  owns: an entry point with a slot of its own, which the warm-up of the largest case must grow."""

    def __init__(self, name, cases, owns=False):
        self.name, self.owns = name, owns
        self.cases = [(ident, self._on_own_stream(run)) for ident, run in cases]

    @staticmethod
    def _on_own_stream(run):
        def go(c):
            try:
                run(c)
            finally:
                c["m"].set_stream(None)                         # some bodies move their matcher to torch's stream
        return go

    small = property(lambda self: self.cases[0])
    large = property(lambda self: self.cases[-1])


def _window(name, build):
    def run(c):
        case = build()
        WG.same(WG.run_case(c["pkg"], case), WG.want_case(name, case), name)
    return name, run


def _init_host(c):
    if not c["init_want"]:
        k1, d1, k2, d2 = WG.case_init()
        prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
        F1, F2 = SM.Frame(k1, d1, None, WG.BOUNDS, WG.SF), SM.Frame(k2, d2, None, WG.BOUNDS, WG.SF)
        c["init_want"].append(SM.search_for_initialization(F1, F2, prev, 100, 0.9, True))
    got, want = WG.run_init(c["pkg"]), c["init_want"][0]
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def _bow(name):
    def run(c):
        for form in ("frame", "kf"):
            SB._bow_both_entries(c["pkg"], c["torch"], c["bow"][name], form)
    return name, run


def _tri_search(name):
    return name, (lambda c: SB.test_search_for_triangulation_host_entry(c["pkg"], c["trs"][name]))


def _tri_in_new_points(name):
    return name, (lambda c: SB.test_search_inside_create_new_map_points_device(c["pkg"], c["torch"], c["trs"][name]))


def _sim3_ransac(name, mode):
    def run(c):
        env = c["sim3"] if c["between"] is None else dict(c["sim3"], m=FillBetween(c["m"], c["between"]))
        RG.test_device_equals_seqref(env, name, mode)
    return "%s-%d" % (name, mode), run


def _pnp_ransac(name, form):
    def run(c):
        env = c["pnp"] if c["between"] is None else dict(c["pnp"], m=FillBetween(c["m"], c["between"]))
        NG.test_device_equals_seqref(env, name, form)
    return "%s-%d" % (name, form), run


def _eg_device(name):
    def run(c):
        EG.test_device_equals_seqref(c["eg"], name)
        if name == "p9":
            EG.test_the_call_synchronises_once_per_trial(c["eg"])
    return name, run


def call(fn, key, *args, ident=None):
    """(id, run): the stage module's own body `fn` on ctx[key] and `args`."""
    return (ident or "-".join(str(a) for a in args) or fn.__name__), (lambda c: fn(c[key], *args))


# the optimisers' cases: the smallest, a capacity exceeded by one, a failed factorisation or a stale solver x, the largest
LBA_CASES = ("S", "points_plus_one", "zero_depth", "M")
GBA_CASES = ("base", "edges_plus_one", "f9", "wide")
POSE_CASES = ("A", "stale_step", "comeback", "batch3")
assert set(LBA_CASES) <= set(LBK.CASES) and set(POSE_CASES) <= set(POK.CASES)

STAGES = [
    # the windowed searches: CSR grid, window search, resolve (S_CAND, S_CNT, S_CCAND, S_CSR, S_Q, S_TAKEN, S_OUT); the last case has 5000
    # train key points, above kResolveMax = 4096, so the resolve state lives in S_STATE
    Stage("window-host", [_window("borders", WG.case_borders), _window("lengths", WG.case_lengths),
                          _window("wide300", lambda: WG.case_wide(300)),
                          call(TM.test_projection_searches_have_no_size_limit, "tup3", 5000, 3000, 0.9, ident="hbm5000")], owns=True),
    Stage("window-device", [call(WG.test_device_entries_equal_host_entries, "pkg", ident="entries"),
                            call(WG.check_track, "pkg", (15.0,), ident="track15")]),
    Stage("init-host", [call(TS.test_constructed_edge_cases_equal_seqref, "tup2", ident="edges"), ("init100", _init_host)]),
    Stage("init-device", [call(TP.test_search_for_initialization_device_matches_oracle, "tup3", ident="pairs3")]),
    Stage("bow", [_bow("th"), _bow("cull"), _bow("sparse"), _bow("nodes40")]),
    Stage("triangulation-search", [_tri_search(n) for n in ("tie", "th_low", "tri_a")]),
    Stage("descriptor-distance", [call(TM.test_descriptor_distance_matrix, "tup3", ident="300x257")]),
    # not in the list of stages to pin, but on the same slots (S_OUT, S_MISC, S_ORD, S_CNT): the frame glue and the stereo matcher
    Stage("frame-glue", [call(TM.test_undistort_keypoints, "tup3", ident="undistort"),
                         call(TM.test_distinctive_descriptors, "tup3", ident="distinctive"),
                         call(TM.test_frame_glue_grid_and_rgbd, "tup3", ident="grid-rgbd")]),
    # ties: 240 rows and 20 right key points, so the row table and the record array of S_ORD and the SAD list of S_CNT shrink
    Stage("stereo-matches", [call(TC.test_host_entry_equals_seqref, "tup2", "ties", ident="ties"),
                             call(TM.test_compute_stereo_matches, "tup3", 3, 752, 480, 1000, ident="752x480"),
                             call(TM.test_device_batched_stereo_equals_host_api, "tup3", ident="device-batch")]),
    Stage("fuse", [call(SP.test_fuse_ties_borders_and_gates_through_every_entry, "seqproj", False, False, ident="edges-mono"),
                   call(SP.test_fuse_ties_borders_and_gates_through_every_entry, "seqproj", True, True, ident="edges-stereo-sim3"),
                   call(FB.test_host_entry_equals_single_calls_and_the_oracle, "fuse_batch", ident="host-batch"),
                   call(FB.test_rows_equal_the_oracle_per_key_frame, "fuse_batch", False, 3.0, ident="device-batch")]),
    Stage("search-by-sim3", [call(SP.test_search_by_sim3_equals_literal, "seqproj", 0.8, 11),
                             call(SP.test_search_by_sim3_equals_literal, "seqproj", 1.3, 13)]),
    Stage("new-points-device", [_tri_in_new_points("tie"),
                                call(TR.test_odd_counts, "tri", 1, ident="n1"),
                                call(TR.test_monocular_rows_with_the_sequential_search, "tri", ident="mono"),
                                call(TR.test_stereo_rows_with_the_sequential_search, "tri", False, True, ident="stereo")], owns=True),
    Stage("new-points-host", [call(TR.test_host_twin_equals_the_device_call, "tri", ident="twin")]),
    Stage("update-map-points", [call(PG.test_a_prefix_of_the_points_and_no_bad_key_frames, "mappoint", ident="prefix37"),
                                call(PG.test_limit_of_2048_observations, "mappoint", ident="limit2048"),
                                call(PG.test_random_scene_device_and_host_equal_seqref, "mappoint", MP.UPDATE_DESCRIPTOR,
                                     ident="descriptor"),
                                call(PG.test_random_scene_device_and_host_equal_seqref, "mappoint", PG.BOTH, ident="both")], owns=True),
    Stage("local-map-device", [call(MG.test_update_local_map_device_equals_seqref, "plain", n) for n in ("C", "B", "A")], owns=True),
    Stage("local-map-host", [call(MG.test_host_entry_equals_the_device_entry, "plain", n) for n in ("C", "A")]),
    Stage("connections-device", [call(CG.test_update_connections_device_equals_seqref, "plain", n, ident="%s%d" % n)
                                 for n in (("random", 2), ("strides", 40), ("random", 65), ("random", 257))], owns=True),
    Stage("connections-host", [call(CG.test_host_entry_equals_the_device_entry, "plain", n, ident="%s%d" % n)
                               for n in (("random", 1), ("strides", 40), ("random", 65))]),
    Stage("cull-key-frames", [call(KG.test_cull_key_frames_device_equals_seqref, "plain", n) for n in ("r2", "r12", "r257")], owns=True),
    Stage("cull-map-points", [call(KG.test_cull_map_points_device_equals_seqref, "plain", n, R)
                              for n, R in (("r2", 1), ("r65", 65), ("r257", 1000))]),
    Stage("cull-host", [call(KG.test_host_entries_equal_the_device_entries, "plain", n) for n in ("r12", "r65")]),
    # the solvers: `between` fills the handle after setup and before every iterate call
    Stage("sim3-ransac-device", [_sim3_ransac("hand", 0), _sim3_ransac("unit", 3), _sim3_ransac("scene", 1), _sim3_ransac("batch", 0)],
          owns=True),
    Stage("sim3-ransac-host", [call(RG.test_host_form_equals_device_form, "sim3", ident="hand-batch")], owns=True),
    Stage("pnp-ransac-device", [_pnp_ransac("edge", PNP.MATCH_POINTS), _pnp_ransac("planar", PNP.MATCH_SLOTS),
                                _pnp_ransac("sizes", PNP.MATCH_POINTS), _pnp_ransac("large", PNP.MATCH_POINTS)], owns=True),
    Stage("pnp-ransac-host", [call(NG.test_host_form_equals_device_form, "pnp", ident="edge-plain")], owns=True),
    Stage("pose-optimization-device", [call(OG.test_device_equals_seqref, "poseopt", n) for n in POSE_CASES]),
    Stage("pose-optimization-host", [call(OG.test_host_form_equals_seqref, "poseopt", n) for n in POSE_CASES]),
    Stage("optimize-sim3-device", [call(SG.test_candidate_alone_equals_its_row_of_the_batch, "sim3opt", ident="A_alone"),
                                   call(SG.test_device_equals_seqref, "sim3opt", "A", 1),
                                   call(SG.test_device_equals_seqref, "sim3opt", "B", 3),
                                   call(SG.test_device_equals_seqref, "sim3opt", "B", 0)]),
    Stage("optimize-sim3-host", [call(SG.test_host_form_equals_seqref, "sim3opt", "A", 1),
                                 call(SG.test_host_form_equals_seqref, "sim3opt", "B", 0)]),
    # zero_depth: a NaN in the system, so the first factorisation of round 1 fails and the increments x_p, x_l are read as setup
    # left them
    Stage("lba-device", [call(LG.test_device_equals_seqref, "lba", n) for n in LBA_CASES], owns=True),
    Stage("lba-host", [call(LG.test_host_form_equals_seqref, "lba", n) for n in LBA_CASES]),
    Stage("essential-graph-device", [_eg_device(n) for n in ("r6", "bad9", "p9")], owns=True),
    Stage("essential-graph-host", [call(EG.test_host_form_equals_seqref, "eg", n) for n in ("r6", "bad9", "p9")]),
    Stage("gba-device", [call(GG.test_device_equals_seqref, "gba", n) for n in GBA_CASES], owns=True),
    Stage("gba-host", [call(GG.test_host_form_equals_seqref, "gba", n) for n in GBA_CASES]),
    Stage("apply-gba", [call(GG.test_apply_device_and_host_equal_seqref, "gba", ident="tree-no_bad")], owns=True),
]
assert all(1 <= len(s.cases) <= 4 for s in STAGES) and len({s.name for s in STAGES}) == len(STAGES)


def _runs():
    """(stage, case) in file order with the largest case of a stage first: it is the one whose warm-up must grow the slot."""
    return [pytest.param(s, k, id="%s-%s" % (s.name, s.cases[k][0])) for s in STAGES for k in reversed(range(len(s.cases)))]


@pytest.mark.parametrize("stage,k", _runs())
def test_filled(ctx, stage, k):
    m, (ident, run) = ctx["m"], stage.cases[k]
    before = m.FillScratch(0x00)
    run(ctx)                                                    # the warm-up: grows the slots, and checks the case
    after = m.FillScratch(BYTES[0])
    assert after >= before > 0 or before == 0
    if stage.owns and k == len(stage.cases) - 1:
        assert after > before, "%s: the warm-up of %s grew no workspace of the handle (%d bytes)" % (stage.name, ident, before)
    wrong = []                                                  # every byte is tried, so that a failure names all that expose it
    for byte in BYTES:
        assert m.FillScratch(byte) == after
        ctx["between"] = byte
        try:
            run(ctx)
        except AssertionError as e:
            wrong.append("after FillScratch(0x%02X): %s" % (byte, str(e)[:600]))
        finally:
            ctx["between"] = None
        assert m.FillScratch(byte) == after, "%s: the same case grew a slot on its second run" % stage.name
    assert not wrong, "%s %s\n%s" % (stage.name, ident, "\n".join(wrong))


@pytest.mark.parametrize("stage", [pytest.param(s, id=s.name) for s in STAGES])
def test_residue(ctx, stage):
    for ident, run in (stage.large, stage.small, stage.small, stage.large):
        run(ctx)


def test_cross_stage(ctx):
    for ident, run in [s.small for s in STAGES]:
        run(ctx)
    assert ctx["m"].FillScratch(0xFF) > 0
    for ident, run in [s.small for s in reversed(STAGES)]:
        run(ctx)


def test_fill_scratch_reports_and_refuses(ctx):
    """An empty handle has nothing to fill; a byte outside 0 .. 255 and a null handle are refused."""
    import ctypes as C
    pkg = ctx["pkg"]
    fresh = pkg._pkg.ORBmatcher()
    assert fresh.FillScratch(0xFF) == 0
    a = np.arange(64, dtype=np.uint8).reshape(2, 32)
    want = np.unpackbits(a[:, None, :] ^ a[None, :, :], axis=2).sum(2)
    assert np.array_equal(fresh.DescriptorDistance(a, a), want)
    grown = fresh.FillScratch(0xA5)
    assert grown >= 3 * 256 and np.array_equal(fresh.DescriptorDistance(a, a), want)
    for byte in (-1, 256):
        with pytest.raises(pkg.OrbHipError) as ei:
            fresh.FillScratch(byte)
        assert ei.value.code == pkg.capi.E_ARG
    assert pkg.capi.lib().orbhip_matcher_fill_scratch(None, 0, C.byref(C.c_ulonglong())) == pkg.capi.E_ARG
    fresh.close()
