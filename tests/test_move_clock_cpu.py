"""Which move's games-finished snapshot a drain may read (az_move_clock.h, the
rule behind az_selfplay_drain and az_chess_selfplay_drain) is a pure function
of the last move issued, the batch's first move and whether the last move has
finished on every lane.  This compiles the header for the host, without HIP,
and pins the rule on its five cases: no move issued since the batch began;
the last move finished; the last move running with a finished move of the
batch before it (that one, after a wait); the last move running as the
batch's first (nothing); and a batch begun after earlier batches' moves,
which never yields one of theirs."""
import os
import subprocess

import pytest

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_drainable_move_rule(tmp_path):
    exe = tmp_path / "move_clock_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-Wall", "-Werror", "-x", "c++",
                    "-I", os.path.join(R, "custom-alphazero_amd", "csrc"),
                    os.path.join(R, "tests", "native", "move_clock_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "0 failures", out.stdout
