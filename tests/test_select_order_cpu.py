"""The best-edge choice on any evaluator output, on the CPU.

get_best_edge (mcts.py:64-68) is np.argmax over a list of Python floats: the
first NaN wins; else the first maximum, -0.0 == +0.0 a tie, +-inf ordinary
numbers.  Three statements of it are pinned here, each against numpy itself:

* the oracles' orc_argmax_f64 (oracle/az_oracle.c), on every vector of length
  1..5 over {NaN, -inf, -1, -0.0, +0.0, 1, +inf} and on seeded random ones;
* the device's select_key / select_edge / select_merge (csrc/az_device.h),
  built for the host and run over simulated lanes in the kernels' step order
  (tests/native/select_check.cpp) on the same vectors;
* whole games: the Connect-N oracle through its callback against
  oracle/refport.py (np.argmax on Python floats, as mcts.py) under evaluator
  outputs that are negative, cancelling, subnormal, huge, infinite or NaN
  (tests/select_cases.py).

Liveness: the loop the oracles and the plain descents had before -- the first
element, then strict `>` -- is kept below as a few lines of Python
(select_cases.kept_rule_argmax).  For every (shape, kind) the device tests run
with a non-finite kind, some compared game differs between np.argmax and that
loop, so a kernel that still skips a NaN cannot pass them.
"""
import contextlib
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import chess_oracle as C
import oracle
import select_cases as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
BUILD = os.path.join(NATIVE, "_build")

NAN = float("nan")


def np_argmax(v):
    return int(np.argmax([float(x) for x in v]))  # a list of Python floats, as get_best_edge builds


@pytest.fixture(scope="module")
def vectors():
    """every vector of length 1..5 over the alphabet (19,607), then seeded random ones up to length
    256 from the alphabet plus ordinary doubles, with a few shapes by hand"""
    vs = [list(v) for n in range(1, 6) for v in itertools.product(S.ALPHABET, repeat=n)]
    assert len(vs) == 19607
    rng = np.random.RandomState(7)
    pool = np.array(S.ALPHABET + [5e-324, -5e-324, 1e308, -1e308, 0.5, 1.0 + 2.0 ** -52])
    for i in range(3000):
        n = int(rng.randint(1, 257)) if i % 3 else int(rng.choice([63, 64, 65, 127, 128, 129, 255, 256]))
        mode = i % 4
        if mode == 0:    # the alphabet alone: many ties, NaN nearly everywhere
            v = rng.choice(pool[:7], n)
        elif mode == 1:  # ordinary doubles with a few oddities
            v = rng.standard_normal(n)
            k = rng.randint(0, n, 3)
            v[k] = rng.choice(pool, 3)
        elif mode == 2:  # few distinct values: the first maximum is among many equals
            v = rng.choice(np.array([-2.5, -0.0, 0.0, 3.25]), n)
        else:            # one NaN late among numbers
            v = rng.standard_normal(n)
            v[rng.randint(n // 2, n)] = NAN
        vs.append([float(x) for x in v])
    for n in (1, 2, 7, 8, 9, 64, 65, 128, 200, 256):
        vs += [[NAN] * n, [float("-inf")] * n, [-0.0] * n, [0.0] * (n - 1) + [-0.0], [-0.0] * (n - 1) + [0.0],
               [float("-inf")] * (n - 1) + [NAN], [float("inf")] * (n - 1) + [NAN]]
    return vs


@pytest.fixture(scope="module")
def expected(vectors):
    return [np_argmax(v) for v in vectors]


# ------------------------------------------------------------------ the oracles
def test_oracle_argmax_is_np_argmax(vectors, expected):
    got = [oracle.argmax_f64(v) for v in vectors]
    bad = [(v, g, w) for v, g, w in zip(vectors, got, expected) if g != w]
    assert not bad, bad[:5]


def test_the_kept_rule_is_not_np_argmax(vectors, expected):
    """the liveness of the vectors themselves: the earlier loop misses on many of them, and only
    where a NaN stands after index 0"""
    miss = [v for v, w in zip(vectors, expected) if S.kept_rule_argmax(v) != w]
    assert len(miss) > 5000
    assert all(any(x != x for x in v[1:]) for v in miss)


# ------------------------------------------------------- the device's statement
@pytest.fixture(scope="module")
def select_check():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "select_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                    os.path.join(NATIVE, "select_check.cpp"), "-o", exe], check=True, timeout=600)
    return exe


def test_device_select_is_np_argmax_on_every_lane(select_check, vectors, expected, tmp_path):
    path = tmp_path / "vectors.bin"
    with open(path, "wb") as f:
        for v in vectors:
            f.write(np.int32(len(v)).tobytes())
            f.write(np.asarray(v, "<f8").tobytes())
    lines = subprocess.run([select_check, str(path)], capture_output=True, text=True, check=True,
                           timeout=300).stdout.splitlines()
    assert len(lines) == len(vectors)
    ran = {8: 0, 16: 0, 32: 0, 64: 0}
    for v, want, line in zip(vectors, expected, lines):
        serial, g8, g16, g32, g64, chess, agree = (int(x) for x in line.split())
        cnt = len(v)
        assert agree == 1, v  # every lane of every group and of the wave ends with one index
        assert 0 <= want < cnt
        assert serial == want and chess == want, (v, serial, chess, want)
        for L, g in ((8, g8), (16, g16), (32, g32), (64, g64)):
            if cnt <= L:
                assert g == want, (v, L, g, want)
                ran[L] += 1
            else:
                assert g == -1
        if all(x != x for x in v) or all(x == float("-inf") for x in v):
            assert serial == 0  # all NaN, all -inf: the first edge
    assert min(ran.values()) > 19000


# ------------------------------------------------------------ Connect-N, games
def _oracle_game(shape, kind, seed):
    H, W, n, gravity, sims = S.SHAPES[shape]
    return oracle.play_game(H, W, n, gravity, sims, seed, evaluator="callback", callback=S.BoardEval(kind, shape))


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_oracle_game_equals_refport(shape, kind):
    """oracle.play_game through its callback == refport.play_game, bit for bit"""
    for seed in S.SEEDS:
        ref, got = S.port_game(shape, kind, seed), _oracle_game(shape, kind, seed)
        assert got["T"] == ref["T"], (seed, got["T"], ref["T"])
        np.testing.assert_array_equal(got["moves"], ref["moves"])
        np.testing.assert_array_equal(got["policy"].view(np.uint64), np.asarray(ref["policies"]).view(np.uint64))
        assert got["expansions"] == ref["expansions"]


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_illegal_junk_changes_nothing(shape):
    for seed in S.SEEDS:
        assert S.same_game(S.port_game(shape, "illegal_junk", seed), S.port_game(shape, None, seed))


@pytest.mark.parametrize("shape,kind", S.LIVE_CASES)
def test_nonfinite_case_is_live(shape, kind):
    """np.argmax and the kept rule part ways in some compared game of every non-finite case the
    device tests run"""
    assert any(not S.same_game(S.port_game(shape, kind, seed), S.port_game(shape, kind, seed, kept_rule=True))
               for seed in S.SEEDS)


def test_every_nonfinite_device_case_is_asserted_live():
    """(all-NaN nodes -- nan_prob -- take edge 0 under either rule in a serial statement; there the
    device tests check what a serial rule cannot state, that the lanes of a group agree)"""
    assert set(S.GPU_CASES) >= set(S.LIVE_CASES)
    for shape, kind in S.GPU_CASES:
        if kind in S.NONFINITE and kind != "nan_prob":
            assert (shape, kind) in S.LIVE_CASES


# ----------------------------------------------------------------------- chess
@contextlib.contextmanager
def kept_rule_chess_oracle():
    """chess_oracle.c built with its earlier best-edge loop (-DORC_CHESS_KEPT_RULE), a scratch
    build beside the native checks; the product oracle is not touched"""
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libchess_oracle_kept_rule.so")
    src = os.path.join(REPO, "oracle")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-builtin-pow",
                    "-DORC_CHESS_KEPT_RULE", "-shared", "-o", so, os.path.join(src, "chess_oracle.c"),
                    os.path.join(src, "az_oracle.c"), "-lm"], check=True, timeout=600)
    C.lib()
    saved = C._lib, C.LIB_PATH
    C._lib, C.LIB_PATH = None, so
    try:
        assert C.lib()._name == so
        yield
    finally:
        C._lib, C.LIB_PATH = saved


def test_chess_oracle_parts_from_the_kept_rule_on_nonfinite_kinds():
    fixed = {kind: S.chess_games(S.ChessEval(kind)) for kind in S.NONFINITE}
    with kept_rule_chess_oracle():
        kept = {kind: S.chess_games(S.ChessEval(kind)) for kind in S.NONFINITE}
        plain_kept = S.chess_games(S.ChessEval(None))
    assert isinstance(C.lib(), ctypes.CDLL) and C.lib()._name == C.LIB_PATH
    plain = S.chess_games(S.ChessEval(None))
    # on ordinary outputs the two rules are one
    assert all(S.same_chess_game(a, b) for a, b in zip(plain, plain_kept))
    for kind in S.NONFINITE:
        differs = any(not S.same_chess_game(a, b) for a, b in zip(fixed[kind], kept[kind]))
        if kind == "nan_prob":
            continue  # every UCB of the node is NaN: edge 0 under either rule (the wave descent's start value was the defect)
        assert differs, kind
        assert any(not S.same_chess_game(a, b) for a, b in zip(fixed[kind], plain)), kind


def test_chess_oddities_are_reached():
    """every kind's oracle games differ from the ordinary evaluator's; what the reference masks out
    changes nothing (subnormal priors are the ordinary ones scaled and rounded: the games may agree)"""
    plain = S.chess_games(S.ChessEval(None))
    for kind in S.KINDS:
        differs = any(not S.same_chess_game(a, b) for a, b in zip(S.chess_games(S.ChessEval(kind)), plain))
        if kind == "illegal_junk":
            assert not differs
        elif kind != "subnormal":
            assert differs, kind
