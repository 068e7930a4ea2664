"""Writes tests/golden/solver_c4_7x6.npz: 256 seeded random-playout positions
of 7x6 Connect-4 with 18 to 36 stones (boards [256, 6, 7] int8, +1 the side to
move), their exact scores from tests/native/solver_check.cpp's independent
reference, and the node counts of the host build of csrc/az_solver.h on a cold
2^20-entry table (the GPU test sizes its node budget from them).

    python tests/golden/make_solver_fixture.py [path to a built solver_check]

tests/test_solver_cpu.py regenerates the records and compares them with the file.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(os.path.dirname(HERE), "native")
ARGS = ["random", "6", "7", "4", "256", "20261020", "18", "36"]
RECORD = np.dtype([("board", "i1", (6, 7)), ("score", "i1"), ("nodes", "<i8")])


def records(exe):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "records.bin")
        subprocess.run([exe, *ARGS, path], check=True, capture_output=True, timeout=900)
        return np.fromfile(path, RECORD)


def main():
    exe = sys.argv[1] if len(sys.argv) > 1 else os.path.join(NATIVE, "_build", "solver_check_plain")
    if not os.path.exists(exe):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(NATIVE, "solver_check.cpp"),
                        "-o", exe], check=True)
    r = records(exe)
    np.savez_compressed(os.path.join(HERE, "solver_c4_7x6.npz"), boards=r["board"],
                        scores=r["score"].astype(np.int32), nodes=r["nodes"].astype(np.int64))


if __name__ == "__main__":
    main()
