"""The staging bookkeeping of the matcher's host forms (orb_slam2_comment_amd/csrc/orbhip_stage.h: piece offsets and
alignment, the measuring pass and the real pass, the recorded outputs and their scatter), compiled alone with g++ and
driven against malloc'ed buffers by tests/cpp/stage_check.cpp.  The copies themselves and the buffers behind them
(stage_send, stage_fetch) need a device: the host forms' GPU tests cover them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage") / "stage_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "orb_slam2_comment_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "stage_check.cpp"), "-o", exe], check=True)
    return exe


# sizes: pieces of 0, 1, 255, 256, 257 bytes and 3 x 12 bytes -- measured total = end offset, 256-byte starts, an empty
#        piece takes no room;  fillers: once per piece, real pass only, with the piece's host address, never for an empty
#        piece;  outputs: the span from the first recorded piece to the end of the last with a plain piece between, the
#        scatter writes exactly the recorded bytes (guard bytes intact), a skipped optional output stays untouched;
# capacity: Stage::kMaxOut records work, one more is refused and reported by the measuring pass already
@pytest.mark.parametrize("case", ["sizes", "fillers", "outputs", "capacity"])
def test_stage_bookkeeping(prog, case):
    r = subprocess.run([prog, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
