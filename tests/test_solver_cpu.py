"""The exact Connect-N solver without a GPU.

* tests/native/solver_check.cpp, built here with -fsanitize=address,undefined:
  the host build of csrc/az_solver.h's step function (serial, and with its
  state written out and reloaded every 1, 7 and 1000 steps) against an
  independent reference in that file, on every reachable position of 4x4 and
  4x3 n=3, on seeded samples of 5x4, 4x5, 5x5 n=3 and 7x6; a 2^4-entry table, a
  warm table, the host split, max_jobs, the node budget, input validation.
* tests/golden/solver_c4_7x6.npz is what solver_check writes today.
* exact_solvers/ against a stub solver backed by a score table: the argsort
  with ties, -inf for ending children, the one-hot policy, the sign, the
  arena's indexing of the argsort result, None for malformed move strings.
* With the default ConfigSolver every solver path still raises NotImplementedError.
* hipcc's resource remarks for az_solver.hip: no scratch, no spilled VGPR.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from custom_alphazero.config import ConfigConnectN, ConfigSolver
from custom_alphazero.connect_n.board import Board
from custom_alphazero.connect_n.move import Move
from custom_alphazero.evaluation import evaluate
from custom_alphazero.exact_solvers import c4_exact_solver as exact
from custom_alphazero.mcts.mcts import MCTS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
CSRC = os.path.join(REPO, "custom-alphazero_amd", "csrc")
EXE = os.path.join(NATIVE, "_build", "solver_check")
HIPCC = "/opt/rocm/bin/hipcc"

CHECKS = ["validation", "exhaustive_4x3_n3", "exhaustive_4x4", "random_5x4", "random_4x5", "random_5x5_n3",
          "c4_7x6", "tables", "split", "budget"]


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(NATIVE, "solver_check.cpp"), "-o", EXE], check=True, timeout=600)
    return EXE


@pytest.mark.parametrize("name", CHECKS)
def test_host_build_agrees_with_the_independent_reference(exe, name):
    out = subprocess.run([exe, "check", name], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines()[-1] == "ok"


def test_fixture_is_what_solver_check_writes(exe, golden):
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    try:
        import make_solver_fixture
    finally:
        sys.path.pop(0)
    r = make_solver_fixture.records(exe)
    z = golden("solver_c4_7x6")
    assert len(r) == 256
    stones = (r["board"] != 0).sum(axis=(1, 2))
    assert stones.min() >= 18 and stones.max() <= 36
    np.testing.assert_array_equal(z["boards"], r["board"])
    np.testing.assert_array_equal(z["scores"], r["score"])
    np.testing.assert_array_equal(z["nodes"], r["nodes"])


# ------------------------------------------------------------------ exact_solvers on a stub
class StubSolver:
    """Solver.solve from a score table: a board's score is a fixed function of
    its cells unless `table` names it; `unsolved` boards come back unsolved."""

    def __init__(self):
        self.table, self.unsolved, self.calls = {}, set(), []

    @staticmethod
    def default_score(b):
        return int((b.astype(np.int64) * np.arange(1, b.size + 1).reshape(b.shape)).sum() % 7) - 3

    def solve(self, boards, node_budget):
        boards = np.asarray(boards)
        assert boards.dtype == np.int8 and boards.ndim == 3
        self.calls.append(boards.copy())
        scores = np.array([self.table.get(b.tobytes(), self.default_score(b)) for b in boards], np.int32)
        status = np.array([b.tobytes() in self.unsolved for b in boards], np.uint8)
        return scores, status, np.ones(len(boards), np.int64)


@pytest.fixture
def stub(monkeypatch):
    """A 5-wide, 4-high board, the solver switched on and replaced by the stub."""
    monkeypatch.setattr(ConfigConnectN, "board_width", 5)
    monkeypatch.setattr(ConfigConnectN, "board_height", 4)
    monkeypatch.setattr(ConfigConnectN, "n", 4)
    monkeypatch.setattr(ConfigConnectN, "gravity", True)
    monkeypatch.setattr(ConfigSolver, "node_budget", 1000)
    s = StubSolver()
    monkeypatch.setattr(exact, "get_solver", lambda: s)
    return s


def played(columns):
    board = Board()
    for x in columns:
        board.play(Move(True, x))
    return board


def to_move(board):
    return (board.array * board.turn).astype(np.int8)


def test_ranked_moves_argsort_with_ties_and_sign(stub):
    board = played([2, 2, 1])  # black to move
    children = [board.play(m, on_copy=True) for m in board.moves]
    for child, score in zip(children, [3, -2, 3, -2, 0]):
        stub.table[to_move(child).tobytes()] = score
    stub.table[to_move(board).tobytes()] = -5
    ranked, value = exact.exact_ranked_moves_and_value(board)
    assert [int(i) for i in ranked] == [int(i) for i in np.argsort(np.array([3., -2., 3., -2., 0.]))]
    assert sorted(int(i) for i in ranked[:2]) == [1, 3] and int(ranked[2]) == 4
    assert value == -1.0 and isinstance(value, float)
    # one call: the board first, then its children, +1 the side to move
    assert len(stub.calls) == 1
    np.testing.assert_array_equal(stub.calls[0], np.stack([to_move(board)] + [to_move(c) for c in children]))
    stub.table[to_move(board).tobytes()] = 0
    assert exact.exact_ranked_moves_and_value(board)[1] == 0.0


def test_ending_children_rank_first_and_are_not_solved(stub):
    board = played([0, 0, 1, 1, 2, 2])  # white to move wins with column 3
    children = [board.play(m, on_copy=True) for m in board.moves]
    assert [c.is_game_over() for c in children] == [False, False, False, True, False]
    for child, score in zip(children, [-3, 1, 2, 0, -1]):
        stub.table[to_move(child).tobytes()] = score
    ranked, value = exact.exact_ranked_moves_and_value(board)
    assert [int(i) for i in ranked] == [3, 0, 4, 1, 2]
    assert len(stub.calls[0]) == 5  # the board and four children: the ending one is never sent
    all_moves = Board.get_all_possible_moves()
    policy, value2 = exact.exact_policy_and_value(board, all_moves)
    assert policy.tolist() == [0.0, 0.0, 0.0, 1.0, 0.0] and policy.dtype == np.float64
    assert value2 == value
    # a full column: the policy index is the move's place among all moves, not among the legal ones
    board = played([0, 0, 0, 0, 1, 1, 1, 1])  # columns 0 and 1 hold W B W B: both full
    assert [m.x for m in board.moves] == [2, 3, 4]
    for child, score in zip([board.play(m, on_copy=True) for m in board.moves], [5, -4, 1]):
        stub.table[to_move(child).tobytes()] = score
    policy, _ = exact.exact_policy_and_value(board, all_moves)
    assert policy.tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]


def test_batch_forms_equal_the_single_calls(stub):
    boards = [played([2, 2, 1]), played([0, 0, 1, 1, 2, 2]), played([])]
    single = [exact.exact_ranked_moves_and_value(b) for b in boards]
    stub.calls.clear()
    batch = exact.exact_ranked_moves_and_value_batch(boards)
    assert len(stub.calls) == 1
    assert [([int(i) for i in r], v) for r, v in batch] == [([int(i) for i in r], v) for r, v in single]
    policies, values = exact.exact_policy_and_value_batch(boards, Board.get_all_possible_moves())
    for b, p, v in zip(boards, policies, values):
        p1, v1 = exact.exact_policy_and_value(b, Board.get_all_possible_moves())
        assert p.tolist() == p1.tolist() and v == v1


def test_unsolved_position_raises_budget_error(stub):
    board = played([2, 2, 1])
    child = board.play(board.moves[1], on_copy=True)
    stub.unsolved.add(to_move(child).tobytes())
    with pytest.raises(exact.SolverBudgetError, match=r"4 stones.*1000"):
        exact.exact_ranked_moves_and_value(board)
    assert issubclass(exact.SolverBudgetError, RuntimeError)
    assert exact.exact_ranked_moves_and_value_batch([board, played([])])[0] is None


def test_move_strings(stub):
    scores = exact.evaluate_boards_with_solution("123\n31")
    assert len(stub.calls) == 1 and len(stub.calls[0]) == 2
    a = played([0, 1, 2])
    b = played([2, 0])
    np.testing.assert_array_equal(stub.calls[0], np.stack([to_move(a), to_move(b)]))
    assert scores == [StubSolver.default_score(to_move(a)), StubSolver.default_score(to_move(b))]
    assert all(isinstance(s, int) for s in scores)
    assert exact.evaluate_boards_with_solution("123\n") == scores[:1]  # a trailing end of line is dropped
    for bad in ["12a", "6", "0", "11111", "12\n\n3", "", "1212121"]:  # 1212121: white has won with the 7th stone
        stub.calls.clear()
        assert exact.evaluate_boards_with_solution(bad) is None, bad
        assert not stub.calls


class FakeTensor:
    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a


class FakePolicy:
    """model(x) -> (probabilities, value) preferring columns in a fixed order."""

    def __init__(self, order):
        self.p = np.zeros(len(order), np.float32)
        for rank, x in enumerate(order):
            self.p[x] = 2.0 ** -rank

    def __call__(self, x):
        return FakeTensor(np.tile(self.p / self.p.sum(), (len(x), 1))), FakeTensor(np.zeros((len(x), 1), np.float32))


def reference_scores(current, previous, game_index):
    """evaluate.py:39-62 replayed here: the current model's moves scored as its line 57 does."""
    scores = []
    models = (current, previous)
    turn = game_index % 2
    board = Board()
    all_moves = Board.get_all_possible_moves()
    while not board.is_game_over():
        p = models[turn](board.full_state[None])[0].numpy().ravel()[board.legal_moves_mask(all_moves)]
        move = board.moves[int(np.argmax(p))]
        if turn == 0:
            children = [board.play(m, on_copy=True) for m in board.moves]
            values = np.array([-np.inf if c.is_game_over() else StubSolver.default_score(to_move(c))
                               for c in children])
            ranked = list(np.argsort(values))
            scores.append(1 - (ranked[board.moves.index(move)] + 1) / len(board.moves))
        board.play(move, keep_same_player=True)
        turn = 1 - turn
    return scores


def test_arena_scores_index_the_argsort_by_the_move(stub, monkeypatch):
    current, previous = FakePolicy([2, 3, 1, 4, 0]), FakePolicy([0, 4, 1, 3, 2])
    all_moves = Board.get_all_possible_moves()
    total = []
    for game_index in (0, 1):
        _, scores = evaluate._single_game_evaluation(current, previous, game_index, all_moves, False, True, True)
        want = reference_scores(current, previous, game_index)
        assert scores == want and len(scores) >= 3
        assert evaluate.solver_report == {"scored": len(scores), "unsolved": 0}
        total += want
    # the reference's expression is not the move's rank: the two differ somewhere in these games
    assert any(s != 1 - (r + 1) / k for s, r, k in _rank_scores(current, previous)), "indexing cannot be told apart"
    monkeypatch.setattr(evaluate.ConfigServing, "evaluation_games_number", 2)
    score, solver_score = evaluate.evaluate_two_models(current, previous, evaluate_with_solver=True,
                                                       deterministic=True)
    assert solver_score == np.mean(total) and 0.0 <= score <= 1.0
    assert evaluate.solver_report == {"scored": len(total), "unsolved": 0}
    with pytest.raises(NotImplementedError):  # evaluate.py:100-102
        evaluate.evaluate_two_models(current, previous, evaluate_with_mcts=True, evaluate_with_solver=True)


def _rank_scores(current, previous):
    """(reference score, rank of the chosen move, number of moves) for game 0's scored moves."""
    out = []
    board, turn = Board(), 0
    all_moves = Board.get_all_possible_moves()
    models = (current, previous)
    while not board.is_game_over():
        p = models[turn](board.full_state[None])[0].numpy().ravel()[board.legal_moves_mask(all_moves)]
        move = board.moves[int(np.argmax(p))]
        if turn == 0:
            children = [board.play(m, on_copy=True) for m in board.moves]
            values = np.array([-np.inf if c.is_game_over() else StubSolver.default_score(to_move(c))
                               for c in children])
            ranked = list(np.argsort(values))
            i = board.moves.index(move)
            out.append((1 - (ranked[i] + 1) / len(board.moves), ranked.index(i), len(board.moves)))
        board.play(move, keep_same_player=True)
        turn = 1 - turn
    return out


def test_unsolved_moves_are_left_out_and_counted(stub):
    current, previous = FakePolicy([2, 3, 1, 4, 0]), FakePolicy([0, 4, 1, 3, 2])
    all_moves = Board.get_all_possible_moves()
    stub.unsolved.add(np.zeros((4, 5), np.int8).tobytes())  # the empty board: game 0's first move
    _, scores = evaluate._single_game_evaluation(current, previous, 0, all_moves, False, True, True)
    want = reference_scores(current, previous, 0)
    assert scores == want[1:]
    assert evaluate.solver_report == {"scored": len(want) - 1, "unsolved": 1}


# ------------------------------------------------------------------ still refused by default
def test_default_config_keeps_every_refusal():
    assert ConfigSolver.node_budget == 0
    moves = Board.get_all_possible_moves()
    with pytest.raises(NotImplementedError):
        MCTS(Board(), moves, use_solver=True)
    with pytest.raises(NotImplementedError):
        evaluate.evaluate_two_models(None, None, evaluate_with_solver=True)
    with pytest.raises(NotImplementedError):
        evaluate._single_game_evaluation(None, None, 0, moves, False, True, True)
    with pytest.raises(NotImplementedError):
        evaluate.evaluate_two_models_batched(None, None, 2, evaluate_with_solver=True)
    with pytest.raises(NotImplementedError):
        exact.evaluate_boards_with_solution("1")


def test_boards_the_solver_does_not_take_are_refused(monkeypatch):
    monkeypatch.setattr(ConfigSolver, "node_budget", 1000)
    monkeypatch.setattr(ConfigConnectN, "gravity", False)
    with pytest.raises(NotImplementedError, match="gravity"):
        exact.check_solver_config()
    monkeypatch.setattr(ConfigConnectN, "gravity", True)
    monkeypatch.setattr(ConfigConnectN, "board_width", 9)
    monkeypatch.setattr(ConfigConnectN, "board_height", 9)
    with pytest.raises(NotImplementedError, match=r"W \* \(H \+ 1\) <= 56"):
        exact.check_solver_config()
    with pytest.raises(NotImplementedError, match="56"):
        MCTS(Board(), Board.get_all_possible_moves(), use_solver=True)
    monkeypatch.setattr(evaluate.ConfigGeneral, "game", "chess")
    with pytest.raises(NotImplementedError):
        evaluate.evaluate_two_models(None, None, evaluate_with_solver=True)


# ------------------------------------------------------------------ kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_solver_kernel_uses_no_scratch(tmp_path):
    out = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
         "-c", os.path.join(CSRC, "az_solver.hip"), "-o", str(tmp_path / "s.o")],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "solve_kernel" in k}
    assert len(kernels) >= 1, usage
    for k, v in kernels.items():
        assert v == {"VGPRs Spill": 0, "ScratchSize [bytes/lane]": 0}, (k, v)
