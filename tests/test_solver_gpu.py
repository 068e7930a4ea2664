"""The exact Connect-N solver on the device (engine.Solver, csrc/az_solver.hip)
against the independent reference of tests/native/solver_check.cpp, which is
built here without sanitizers and recomputes the small boards' scores; the
7x6 positions and scores are tests/golden/solver_c4_7x6.npz.  Then the layers
on top: the arena's solver scoring (batched == sequential == a recomputation
from the reference's scores) and MCTS(use_solver=True).
"""
import os
import subprocess

import numpy as np
import pytest

from custom_alphazero import engine as az
from custom_alphazero.config import ConfigConnectN, ConfigSelfPlay, ConfigServing, ConfigSolver
from custom_alphazero.connect_n.board import Board
from custom_alphazero.evaluation import evaluate
from custom_alphazero.exact_solvers import c4_exact_solver as exact
from custom_alphazero.mcts.mcts import MCTS
from custom_alphazero.model.tensorflow.model import PolicyValueModel

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "solver_check_plain")
NO_BUDGET = 1 << 40


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """ref(mode, H, W, n, *args) -> records (board, score, nodes) from solver_check."""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(NATIVE, "solver_check.cpp"),
                    "-o", EXE], check=True, timeout=600)
    tmp = tmp_path_factory.mktemp("solver")
    cache = {}

    def run(mode, H, W, n, *args):
        key = (mode, H, W, n) + args
        if key not in cache:
            path = str(tmp / f"{len(cache)}.bin")
            subprocess.run([EXE, mode, str(H), str(W), str(n), *map(str, args), path], check=True,
                           capture_output=True, timeout=300)
            cache[key] = np.fromfile(path, np.dtype([("board", "i1", (H, W)), ("score", "i1"), ("nodes", "<i8")]))
        return cache[key]

    run.tmp = tmp
    return run


def ref_scores(ref, H, W, n, boards):
    """The reference's scores of arbitrary unfinished boards (+1 the side to move)."""
    path = str(ref.tmp / f"in_{abs(hash(np.asarray(boards).tobytes()))}.bin")
    np.ascontiguousarray(boards, np.int8).tofile(path)
    out = ref("scores", H, W, n, path)
    np.testing.assert_array_equal(out["board"], boards)
    return out["score"].astype(np.int32)


@pytest.fixture(scope="module")
def all_4x4(ref):
    return ref("table", 4, 4, 4)


def check(solver, records, budget=NO_BUDGET):
    scores, status, nodes = solver.solve(records["board"], budget)
    assert not status.any(), f"{int(status.sum())} unsolved"
    np.testing.assert_array_equal(scores, records["score"])
    assert (nodes >= 0).all()
    return nodes


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_wave_edges(all_4x4, count):
    rng = np.random.RandomState(count)
    pick = all_4x4[rng.choice(len(all_4x4), count, replace=False)]
    with az.Solver(4, 4, 4, tt_log2=16) as s:
        check(s, pick)


def test_more_jobs_than_lanes(all_4x4):
    """Every reachable unfinished 4x4 position in one call: twice the lanes a
    launch has, so the queue refills lanes; with the split off, then on."""
    assert len(all_4x4) > 2 * 65536
    with az.Solver(4, 4, 4, tt_log2=20) as s:
        s.configure(split_stones=1)
        check(s, all_4x4)
    with az.Solver(4, 4, 4, tt_log2=20) as s:
        check(s, all_4x4)


@pytest.mark.parametrize("H,W,n", [(4, 5, 4), (5, 4, 4), (5, 5, 3)])
def test_other_boards(ref, H, W, n):
    r = ref("random", H, W, n, 300, 5, 0, H * W - 1)
    with az.Solver(H, W, n, tt_log2=20) as s:
        check(s, r)


def test_empty_6x5_through_the_host_split():
    """The empty 6-wide, 5-high board is a draw (the reference of
    solver_check.cpp, run once outside the suite: it takes minutes there)."""
    with az.Solver(5, 6, 4, tt_log2=24) as s:
        s.configure(split_stones=10)
        scores, status, nodes = s.solve(np.zeros((1, 5, 6), np.int8), 1 << 21)
    assert status[0] == az.SOLVER_SOLVED and scores[0] == 0 and nodes[0] > 1000


@pytest.fixture(scope="module")
def c4(golden):
    z = golden("solver_c4_7x6")
    return z["boards"], z["scores"], int(z["nodes"].max()) * 16


def test_7x6_fixture(c4):
    boards, want, budget = c4
    with az.Solver(6, 7, 4, tt_log2=24) as s:
        scores, status, _ = s.solve(boards, budget)
    assert not status.any()
    np.testing.assert_array_equal(scores, want)


def test_steps_per_launch_and_table_size_do_not_change_scores(c4):
    """32 steps a launch: every search is written back and reloaded, the
    hardest some ten thousand times.  2^4 table entries: collisions and
    replacement on every store; there on the positions with 22 stones or more
    (a table that small repeats most of the work of the shallower ones)."""
    boards, want, _ = c4
    with az.Solver(6, 7, 4, tt_log2=24) as s:
        s.configure(steps_per_launch=32)
        scores, status, _ = s.solve(boards, NO_BUDGET)
        assert not status.any()
        np.testing.assert_array_equal(scores, want)
    easy = (boards != 0).sum(axis=(1, 2)) >= 22
    with az.Solver(6, 7, 4, tt_log2=4) as s:
        scores, status, _ = s.solve(boards[easy], NO_BUDGET)
        assert not status.any()
        np.testing.assert_array_equal(scores, want[easy])


def test_tiny_budget_never_gives_a_wrong_score(golden):
    z = golden("solver_c4_7x6")
    boards, want, host_nodes = z["boards"], z["scores"], z["nodes"]
    budget = 8
    with az.Solver(6, 7, 4, tt_log2=24) as s:
        scores, status, nodes = s.solve(boards, budget)
        solved = status == az.SOLVER_SOLVED
        assert solved.any() and not solved.all()
        np.testing.assert_array_equal(scores[solved], want[solved])
        assert (nodes[~solved] <= budget).all()
        scores, status, _ = s.solve(boards, int(host_nodes.max()) * 16)  # on the table the aborted jobs left
        assert not status.any()
        np.testing.assert_array_equal(scores, want)


def test_two_solvers_interleaved(ref, all_4x4, c4):
    boards, want, budget = c4
    small = all_4x4[::97]
    with az.Solver(4, 4, 4, tt_log2=16) as a, az.Solver(6, 7, 4, tt_log2=22) as b:
        for part in range(4):
            sa, sta, _ = a.solve(small["board"][part::4], NO_BUDGET)
            sb, stb, _ = b.solve(boards[part::4], budget)
            assert not sta.any() and not stb.any()
            np.testing.assert_array_equal(sa, small["score"][part::4])
            np.testing.assert_array_equal(sb, want[part::4])


def test_abi_refusals():
    with pytest.raises(az.AzError, match="56"):
        az.Solver(7, 8, 4)
    with pytest.raises(az.AzError, match="tt_log2"):
        az.Solver(6, 7, 4, tt_log2=2)
    with az.Solver(4, 4, 4, tt_log2=10) as s:
        floating = np.zeros((2, 4, 4), np.int8)
        floating[1, 2, 0] = 1
        with pytest.raises(az.AzError, match="board 1 has a floating stone"):
            s.solve(floating, 100)
        with pytest.raises(az.AzError, match="node_budget"):
            s.solve(floating[:1], 0)
        scores, status, nodes = s.solve(np.zeros((0, 4, 4), np.int8), 100)
        assert len(scores) == len(status) == len(nodes) == 0


# ------------------------------------------------------------------ the arena and MCTS
@pytest.fixture
def small_board():
    saved = (ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity,
             ConfigSolver.node_budget, ConfigSolver.tt_log2, ConfigSolver.split_stones,
             ConfigSelfPlay.mcts_iterations, ConfigServing.evaluation_games_number)

    def set_(H, W, n):
        ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n = H, W, n
        ConfigConnectN.gravity = True
        ConfigSolver.node_budget, ConfigSolver.tt_log2 = 1 << 30, 20
        exact.close_solvers()

    yield set_
    exact.close_solvers()
    (ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity,
     ConfigSolver.node_budget, ConfigSolver.tt_log2, ConfigSolver.split_stones,
     ConfigSelfPlay.mcts_iterations, ConfigServing.evaluation_games_number) = saved


def to_move(board):
    return (board.array * board.turn).astype(np.int8)


@pytest.mark.parametrize("deterministic", [True, False])
def test_arena_solver_scores(ref, small_board, deterministic):
    """5x4, two seeded networks, 4 games: the batched arena's per-move solver
    scores == the sequential loop's == evaluate.py:53-59 recomputed here from
    the independent reference's scores; evaluate_two_models returns their mean."""
    H, W, n, games, seed = 4, 5, 4, 4, 7
    small_board(H, W, n)
    shape = Board().full_state.shape
    a = PolicyValueModel(input_dim=shape, action_space=W, seed=1)
    b = PolicyValueModel(input_dim=shape, action_space=W, seed=2)
    moves = Board.get_all_possible_moves()

    batched = []
    _, results = evaluate.evaluate_two_models_batched(a, b, n_games=games, deterministic=deterministic, seed=seed,
                                                      evaluate_with_solver=True, solver_scores=batched)
    assert evaluate.solver_report == {"scored": len(batched), "unsolved": 0}

    sequential, seq_results = [], []
    for g in range(games):
        r, scores = evaluate._single_game_evaluation(a, b, g, moves, False, True, deterministic,
                                                     rng=np.random.RandomState(seed + g))
        seq_results.append(r)
        sequential += scores
    assert results == seq_results
    assert batched == sequential and len(batched) >= 2 * games

    # the same games replayed here; every position the scoring needs, scored by the reference
    pairs = []
    for g in range(games):
        rng = np.random.RandomState(seed + g)
        board, turn = Board(), g % 2
        while not board.is_game_over():
            move = evaluate._policy_move((a, b)[turn], board, moves, deterministic, rng)
            if turn == 0:
                pairs.append((Board(board.array.copy()), board.moves.index(move)))
            board.play(move, keep_same_player=True)
            turn = 1 - turn
    need, index = [], {}
    for board, _ in pairs:
        for child in [board.play(m, on_copy=True) for m in board.moves]:
            if not child.is_game_over() and to_move(child).tobytes() not in index:
                index[to_move(child).tobytes()] = len(need)
                need.append(to_move(child))
    scores = ref_scores(ref, H, W, n, np.stack(need))
    want = []
    for board, chosen in pairs:
        children = [board.play(m, on_copy=True) for m in board.moves]
        values = np.array([-np.inf if c.is_game_over() else scores[index[to_move(c).tobytes()]] for c in children])
        ranked = list(np.argsort(values))
        want.append(1 - (ranked[chosen] + 1) / len(children))
    assert batched == want

    if deterministic:
        ConfigServing.evaluation_games_number = games
        _, solver_score = evaluate.evaluate_two_models(a, b, evaluate_with_solver=True, deterministic=True)
        assert solver_score == np.mean(want)
        assert evaluate.solver_report == {"scored": len(want), "unsolved": 0}


def test_mcts_with_the_solver_as_evaluator(all_4x4, small_board):
    """MCTS(use_solver=True) on 4x4 == MCTS(model=f), f a Python callable that
    answers exact_policy_and_value from the independent reference's table."""
    small_board(4, 4, 4)
    ConfigSelfPlay.mcts_iterations = 12
    table = {r["board"].tobytes(): int(r["score"]) for r in all_4x4}
    moves = Board.get_all_possible_moves()

    def f(x):
        p = np.zeros((len(x), len(moves)), np.float32)
        v = np.zeros(len(x), np.float32)
        for i, planes in enumerate(x):
            board = Board(Board.from_one_hot(planes[..., :-1]).astype(np.int8))
            assert planes[0, 0, -1] == 1  # the search keeps the side to move white
            children = [board.play(m, on_copy=True) for m in board.moves]
            values = np.array([-np.inf if c.is_game_over() else table[to_move(c).tobytes()] for c in children])
            p[i, board.moves[int(np.argsort(values)[0])].x] = 1.0
            v[i] = np.sign(table[board.array.astype(np.int8).tobytes()])
        return p, v

    with_solver = MCTS(Board(), moves, use_solver=True)
    with_table = MCTS(Board(), moves, model=f)
    for ply in range(3):
        with_solver.search(12)
        with_table.search(12)
        ea, eb = with_solver.current_root.edges, with_table.current_root.edges
        assert [e.visit_count for e in ea] == [e.visit_count for e in eb] and sum(e.visit_count for e in ea) >= 11
        assert [e.prior for e in ea] == [e.prior for e in eb]
        assert [e.total_action_value for e in ea] == [e.total_action_value for e in eb]
        pa = with_solver.play(greedy=True, return_details=True, deterministic=True)
        pb = with_table.play(greedy=True, return_details=True, deterministic=True)
        np.testing.assert_array_equal(pa[2], pb[2])
        assert pa[3] == pb[3]


def test_budget_overrun_surfaces_from_the_search(small_board):
    small_board(6, 7, 4)
    ConfigSolver.node_budget = 1
    ConfigSolver.split_stones = 1  # no host split: the empty 7x6 board is one job, over its budget at once
    ConfigSelfPlay.mcts_iterations = 4
    mcts = MCTS(Board(), Board.get_all_possible_moves(), use_solver=True)
    with pytest.raises(exact.SolverBudgetError):
        mcts.search(4)
