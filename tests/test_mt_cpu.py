"""The arithmetic both engines share, on the CPU against numpy:

* the MT19937 stream (csrc/az_mt.h: mt_seed, mt_twist through mt_next,
  mt_uniform, mt_skip on a word-major slot view) against
  np.random.RandomState: the seeded state, consecutive random_sample values
  across four regenerations, and the state after skipped words;
* pairwise_sum<128> / <256> (csrc/az_device.h) against np.add.reduce, on
  inputs whose left-to-right sum differs from numpy's.

tests/native/mt_check.cpp is the host program; with stride 3 the stream sits
between two sentinel-filled neighbours that must stay untouched.
"""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "mt_check")

SEEDS = [0, 1, 5489, 2 ** 32 - 1]
STRIDES = [1, 3]


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    os.path.join(NATIVE, "mt_check.cpp"), "-o", EXE], check=True, timeout=600)
    return EXE


def _run(exe, *args):
    """the program's output lines without the sentinel verdict (asserted here)"""
    lines = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True,
                           timeout=60).stdout.splitlines()
    assert lines[-1] == "neighbours untouched"
    return lines[:-1]


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_state_is_numpys(exe, seed, stride):
    lines = _run(exe, "seed", seed, stride)
    state = np.random.RandomState(seed).get_state()
    assert len(lines) == 625
    assert [int(v) for v in lines[:624]] == state[1].tolist()
    assert lines[624] == "index 624" and int(state[2]) == 624


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("seed", SEEDS)
def test_uniforms_across_four_regenerations(exe, seed, stride):
    n = 1300  # 2600 words: regenerations at words 0, 624, 1248, 1872 and 2496
    lines = _run(exe, "uniform", seed, stride, n)
    rs = np.random.RandomState(seed)
    want = rs.random_sample(n)
    got = np.array([float.fromhex(v) for v in lines[:n]])
    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()
    assert lines[n] == f"index {int(rs.get_state()[2])}"


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", [0, 1, 168, 623, 624, 625, 1248, 2000])  # 168 = 1 * 6 * 7 * 4: rand(1, H, W, 4)
def test_skip_leaves_the_state_n_draws_leave(exe, n, stride):
    for seed in SEEDS:
        index, u = _run(exe, "skip", seed, stride, n)
        rs = np.random.RandomState(seed)
        rs.randint(0, 2 ** 32, size=n, dtype=np.uint64)  # n single words
        assert index == f"index {int(rs.get_state()[2])}", (seed, n)
        assert float.fromhex(u) == rs.random_sample(), (seed, n)


SUM_N = [0, 1, 7, 8, 9, 127, 128, 129, 135, 136, 137, 255, 256]


@pytest.mark.parametrize("dtype,name", [(np.float32, "f32"), (np.float64, "f64")])
def test_pairwise_sum_is_numpys_add_reduce(exe, tmp_path, dtype, name):
    rng = np.random.RandomState(20)
    # mantissas in [1, 2) over 12 binades: small addends land in different
    # accumulators under different summation orders and change the bits
    a = (rng.uniform(1.0, 2.0, 256) * 2.0 ** rng.randint(-6, 6, 256)).astype(dtype)
    path = tmp_path / "values.bin"
    a.tofile(path)
    lines = subprocess.run([exe, "sum", name, str(path), *map(str, SUM_N)], capture_output=True, text=True,
                           check=True, timeout=60).stdout.splitlines()
    assert len(lines) == len(SUM_N)
    orders_differ = False
    for n, line in zip(SUM_N, lines):
        got_n, s256, s128 = line.split()
        want = np.add.reduce(np.ascontiguousarray(a[:n]))
        assert want.dtype == dtype and int(got_n) == n
        assert dtype(float.fromhex(s256)).tobytes() == want.tobytes(), n
        if n <= 128:
            assert dtype(float.fromhex(s128)).tobytes() == want.tobytes(), n
        else:
            assert s128 == "-"
        serial = dtype(0)
        for v in a[:n]:
            serial = dtype(serial + v)
        orders_differ |= n >= 16 and serial.tobytes() != want.tobytes()
    assert orders_differ, "left-to-right sums equal numpy's: these inputs cannot tell the orders apart"
