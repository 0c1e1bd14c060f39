"""The constructed stereo pairs of stereo_cases.py on the CPU: every case's precondition holds on the sequential
reference (stereo_cases.reference asserts it from `info` before it hands out the answer), the C oracle agrees with the
reference bit for bit, and the figures quoted in DESIGN.md section 3 are re-measured here."""
import numpy as np
import pytest

import stereo_cases as SC
from seqref import matcher as SM

f32 = np.float32


@pytest.mark.parametrize("name", SC.CASES)
def test_oracle_equals_seqref(oracle, name):
    n, ur, dp, info = SC.reference(name)                        # the precondition of the case is asserted in there
    on, our, odp = oracle.compute_stereo_matches(*SC.seqref_args(SC.case(name)))
    assert on == n and our.tobytes() == ur.tobytes() and odp.tobytes() == dp.tobytes()


def test_info_changes_nothing_and_counts_every_exit():
    c = SC.case("gates")
    n, ur, dp, info = SC.reference("gates")
    pn, pur, pdp = SM.compute_stereo_matches(*SC.seqref_args(c))
    assert (pn, pur.tobytes(), pdp.tobytes()) == (n, ur.tobytes(), dp.tobytes())
    assert set(info["count"]) == set(SM.STEREO_EXITS)
    left_exits = [e for e in SM.STEREO_EXITS if e not in ("level_gate", "ur_range", "clamp")]
    assert sum(info["count"][e] for e in left_exits) == len(info["exit"])
    assert len(info["exit"]) + len(info["accepted"]) - info["count"]["median_cull"] == len(c["kl"])
    a = info["accepted"][0]
    assert len(a["vd"]) == 11 and min(a["vd"]) == a["sad"] and -1 <= a["delta"] <= 1 and a["idx_r"] == 1
    # every exit is taken by some case
    seen = {e for name in ("gates", "window_edge", "disparity_negative", "disparity_zero", "median_odd") for e, k in
            SC.reference(name)[3]["count"].items() if k}
    assert seen >= set(SM.STEREO_EXITS) - {"max_u_negative", "delta_range"}, seen


def test_measured_figures():
    """What DESIGN.md section 3 quotes."""
    c = SC.case("reach")
    n, ur, dp, info = SC.reference("reach")
    rows = {(int(k["octave"]), int(k["y"])): (i in info["accepted"]) for i, k in enumerate(c["kl"][:30])}
    for o in (6, 7):
        assert [rows[o, r] for r in (92, 93, 100, 109, 110, 151, 152, 160, 168, 169)] == [False, True, True, True, False] * 2
    assert not any(rows[5, r] for r in (93, 100, 109, 152, 160, 168))
    n, ur, dp, info = SC.reference("sad_ceiling")
    assert info["accepted"][0]["vd"] == SC.CEILING_SADS and (n, ur[0], dp[0]) == (1, 140.0, 4.0)
    n, ur, dp, info = SC.reference("disparity_zero")
    assert (n, ur[0], dp[0]) == (1, f32(139.99), f32(4000))
    n, ur, dp, info = SC.reference("median_zero")
    assert n == 0 and len(info["accepted"]) == 546 and info["th_dist"] == 0
    assert SC.integer_threshold() == (10, 21)
    SC.reference("halves")
    assert SC.case("halves")["found"] == {1: (162, 17), 2: (132, 14), 3: (115, 11)} and len(SC.case("halves")["kl"]) == 11
    assert SC.case("octaves12")["kr"]["octave"].max() == 11 and SC.reference("octaves12")[0] == len(SC.case("octaves12")["kl"])


def test_crowd_rows_fill_whole_rounds():
    """The winner of crowd_round<k> lies in round k of the 64-lane candidate loop: the order sorts by row bucket, the range
    of left row 100 starts at the first right key point there is, and every row before the winner's holds exactly 64."""
    for name, rnd in (("crowd_round2", 2), ("crowd_round3", 3), ("crowd_round4", 4), ("crowd_round5_nr400", 5)):
        c = SC.case(name)
        w = SC.reference(name)[3]["accepted"][0]["idx_r"]
        rows = np.floor(c["kr"]["y"]).astype(int)
        assert rows.min() == 98 and all((rows == r).sum() == 64 for r in range(98, int(rows[w]))) and rows[w] == 98 + rnd - 1
        assert (rows == rows[w]).sum() == 64


def test_painted_sad_is_the_requested_one():
    for sad, lean in ((0, 0), (1, 0), (255, 0), (1250, 150), (1250, -150), (28050, 0)):
        left, right = SC.pair("noise", 5)
        SC.paint_site(left, right, 150, 140, 100, sad, lean)
        c = SC._case("std", left, right, SC.keys([(150.0, 100.0)]), np.zeros((1, 32)), SC.keys([(140.0, 100.0)]),
                     np.zeros((1, 32)), None)
        info = {}
        SM.compute_stereo_matches(*SC.seqref_args(c), info=info)
        a = info["accepted"][0]
        assert a["sad"] == sad and min(v for k, v in enumerate(a["vd"]) if k != 5) >= 120 * 255
        if lean or sad % 110 == 0:                                  # an even spread leaves the parabola upright
            assert (a["delta"] > 0) == (lean > 0) and (a["delta"] < 0) == (lean < 0)
