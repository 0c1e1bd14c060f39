"""The sizing rule of the pyramid kernels' tables (orb_slam2_comment_amd/csrc/pyr_span.h: which dwords and rows of a padded
plane an extraction writes for a level >= 1, for an eager frame depth F), compiled alone with g++: the wavefront counts
at 1241x376 for F = 0 / 8 / 19, alignment, and F = 19 = the full-frame tables as they were ((kPadL + w + kEdge + 3) >> 2
dwords from dword 0, h + 2 kEdge rows from row 0).  build_pyr_tables itself allocates device memory and is covered by
tests/test_pyramid_frames_gpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE, PAD_L, ROWS = 19, 32, 4
LEVELS = [(1034, 313), (862, 261), (718, 218), (598, 181), (499, 151), (416, 126), (346, 105)]   # 1241x376, scale 1.2
# wavefronts per frame and level: ceil(words / 64) * ceil(rows / 4)
UNITS = {19: [440, 300, 256, 165, 144, 82, 72], 0: [395, 264, 165, 138, 76, 64, 54], 8: [415, 280, 177, 150, 126, 72, 62]}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pyr_span") / "pyr_span_check")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pyr_span_check.cpp"), "-o", exe], check=True)
    return exe


def spans(prog, F, levels=LEVELS):
    args = [prog, str(F), str(EDGE), str(PAD_L), str(ROWS)] + [str(v) for wh in levels for v in wh]
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split("\n")
    return [tuple(int(v) for v in line.split()) for line in out if line]


@pytest.mark.parametrize("F", [0, 8, 19])
def test_unit_counts(prog, F):
    got = spans(prog, F)
    assert [g[4] for g in got] == UNITS[F]
    assert sum(UNITS[F]) == {19: 1459, 0: 1156, 8: 1282}[F]
    for (col0, words, row0, rows, _), (w, h) in zip(got, LEVELS):
        # the span covers columns [-F, w + F) and padded rows [EDGE - F, EDGE + h + F), from a dword boundary, with less
        # than one dword of slack at either end (F = 19: from dword 0 of the row)
        assert row0 == EDGE - F and rows == h + 2 * F
        first, last = col0 * 4 - PAD_L, (col0 + words) * 4 - PAD_L
        assert first <= -F and last >= w + F and last - (w + F) < 4
        assert (-F - first < 4) if F < EDGE else col0 == 0


def test_full_frame_is_the_previous_table(prog):
    sizes = LEVELS + [(276, 131), (57, 42), (169, 127), (41, 40)]
    for (col0, words, row0, rows, units), (w, h) in zip(spans(prog, 19, sizes), sizes):
        pw = (PAD_L + w + EDGE + 3) >> 2
        assert (col0, words, row0, rows) == (0, pw, 0, h + 2 * EDGE)
        assert units == ((rows + 3) // 4) * ((pw + 63) // 64)


def test_two_column_chunks_at_276(prog):
    (col0, words, _, _, units), = spans(prog, 0, [(276, 131)])
    assert (col0, words) == (8, 69) and units == 2 * 33
