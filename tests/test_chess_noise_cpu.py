"""Dirichlet root noise for chess, the parts that need no GPU:

* tests/chess_noise_ref.py (the plain-Python MCTS the GPU tests compare the
  noisy engine with) equals the chess oracle with noise off -- trees and a
  whole game -- which is what licenses it as the reference with noise on;
* the attempt-indexed Dirichlet draw of the chess select kernel
  (csrc/az_dirichlet_wave.h), built for the host with its 64 lanes as a loop
  (tests/native/chess_noise_check.cpp), against numpy's legacy
  RandomState.dirichlet: every draw's bits and the stream position after it;
* the lane-parallel MT19937 regeneration in both lane orders;
* the Python surface that needs no device.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chess_noise_ref as R
import chess_oracle as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "chess_noise_check")

# tests/test_chess_tree_gpu.py's ROOTS[1] and [4] (that module is GPU-marked; the FENs are data)
ROOTS = [
    "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
    "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8",
]


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                    os.path.join(NATIVE, "chess_noise_check.cpp"), "-o", EXE], check=True, timeout=600)
    return EXE


# ------------------------------------------------ 1. the helper is the oracle
def _same_root(got, want, tag):
    assert got["moves"].tolist() == want["moves"].tolist(), tag
    assert got["prior"].view(np.uint64).tolist() == want["prior"].view(np.uint64).tolist(), tag
    assert got["w"].view(np.uint64).tolist() == want["w"].view(np.uint64).tolist(), tag
    assert got["n"].tolist() == want["n"].tolist(), tag
    assert got["child_n"].tolist() == want["child_n"].tolist(), tag


@pytest.mark.parametrize("fen", ROOTS)
def test_helper_without_noise_is_the_oracle_tree(fen):
    root = C.from_fen(fen)
    ref, mine = C.Tree(root), R.Tree(root)
    for step, (sims, u) in enumerate([(40, 0.37), (25, 0.81)]):
        ref.search(sims)
        mine.search(sims)
        _same_root(mine.root(), ref.root(), ("search", step))
        if step == 0:
            mv, oc, pa, pp = ref.play(u)
            mv2, oc2, pa2, pp2 = mine.play(u)
            assert (mv, oc) == (mv2, oc2)
            assert pa.tolist() == pa2.tolist()
            assert pp.view(np.uint64).tolist() == pp2.view(np.uint64).tolist()
            _same_root(mine.root(), ref.root(), "reuse")
    assert mine.expansions == ref.expansions


def test_helper_without_noise_is_the_oracle_game():
    ref = C.play_game(16, 7, 6)
    mine = R.play_game(16, 7, 6)
    assert mine["T"] == ref["T"] == 6
    assert (mine["result"], mine["termination"], mine["expansions"]) == \
        (ref["result"], ref["termination"], ref["expansions"])
    assert mine["positions"].tobytes() == ref["positions"].tobytes()
    assert mine["moves"].tolist() == ref["moves"].tolist()
    for t in range(ref["T"]):
        k = int(ref["policy_n"][t])
        assert int(mine["policy_n"][t]) == k
        assert mine["policy_actions"][t].tolist() == ref["policy_actions"][t, :k].tolist()
        assert mine["policy_probs"][t].view(np.uint64).tolist() == ref["policy_probs"][t, :k].view(np.uint64).tolist()


# ------------------------------------- 2. the attempt-indexed draw is numpy's
@pytest.mark.parametrize("alpha", [0.03, 0.3, 0.9, 1.0])
@pytest.mark.parametrize("k", [1, 2, 20, 63, 64, 65, 218])
def test_wave_draw_matches_numpy_legacy_dirichlet(exe, k, alpha):
    n = 40 if k == 218 else 200
    seed = 1000 * k + int(alpha * 100)
    lines = subprocess.run([exe, "draw", str(seed), str(k), repr(alpha), str(n)], capture_output=True, text=True,
                           check=True, timeout=120).stdout.splitlines()
    rs = np.random.RandomState(seed)
    wpa = 2 if alpha == 1.0 else 4  # MT19937 words per attempt
    li = 0
    beyond = 0  # draws that consumed more than their k attempts' words
    for i in range(n):
        before = int(rs.get_state()[2])
        want = rs.dirichlet(np.ones(k) * alpha)
        # words this draw consumed, from numpy's own positions: congruent to the
        # difference modulo 624 and at least wpa * k (never above the truth)
        used = (int(rs.get_state()[2]) - before) % 624
        while used < wpa * k:
            used += 624
        beyond += used > wpa * k
        got = np.array([float.fromhex(v) for v in lines[li].split()])
        li += 1
        assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist(), f"draw {i}"
        if i % 7 == 6:  # a random_sample between draws shifts the boundary alignment
            tag, u = lines[li].split()
            li += 1
            assert tag == "u" and float.fromhex(u) == rs.random_sample(), f"uniform after draw {i}"
    tag, u, pos, _regen = lines[li].split()
    assert tag == "next" and int(pos) == int(rs.get_state()[2])
    assert float.fromhex(u) == rs.random_sample()
    if alpha < 1.0:
        assert beyond > 0, "no rejection in this case: a sampler that ignored rejections would pass"
    else:
        assert beyond == 0


# ------------------------------------------ 3. the lane-parallel regeneration
@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1])
@pytest.mark.parametrize("reverse", [0, 1])
def test_lane_parallel_twist_is_genrand(exe, seed, reverse):
    for n in (1, 2, 3):
        words = subprocess.run([exe, "twist", str(seed), str(reverse), str(n)], capture_output=True, text=True,
                               check=True, timeout=60).stdout.split()
        rs = np.random.RandomState(seed)
        rs.randint(0, 2 ** 32, size=1 + 624 * (n - 1), dtype=np.uint64)  # one word past n - 1 full states
        assert np.array(words, np.uint64).tolist() == rs.get_state()[1].astype(np.uint64).tolist(), (seed, n)


# --------------------------------------------------------- 4. Python surface
def test_chess_selfplay_path_accepts_the_flag():
    from custom_alphazero.config import ConfigMCTS, check_mcts_config
    saved = ConfigMCTS.enable_dirichlet_noise
    try:
        ConfigMCTS.enable_dirichlet_noise = True
        check_mcts_config("chess_selfplay")
        with pytest.raises(NotImplementedError):
            check_mcts_config("chess")  # the Python MCTS class and the arena on chess boards
    finally:
        ConfigMCTS.enable_dirichlet_noise = saved


def test_chess_config_and_header_carry_the_noise_fields():
    from custom_alphazero import engine as az
    cfg = az.ChessConfig
    assert (cfg.dirichlet_noise.offset, cfg.dirichlet_alpha.offset, cfg.dirichlet_ratio.offset) == (68, 72, 80)
    assert ctypes.sizeof(cfg) == 88
    assert "az_chess_tree_search_noise" in az.EXPORTED
    with open(os.path.join(REPO, "include", "az_chess.h")) as f:
        header = f.read()
    assert "int az_chess_tree_search_noise(az_chess_engine* eng, int n_sims, const double* noise, int rows);" in header
