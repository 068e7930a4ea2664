"""The exact solver's opening book on the device (engine.Solver.book_*,
csrc/az_book.hip).  The levels against a breadth-first search written here
(its own bitboards, row-major, and its own mirror); the scores against the
independent reference of tests/native/solver_check.cpp, built here without
sanitizers; budgets, chunks, resuming from a file in another process's stead,
the file's refusals; then the layers on top: the arena's solver scoring and
MCTS(use_solver=True) through ConfigSolver.book_path.
"""
import os
import subprocess
import time

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
ALL = 1 << 30

# (H, W, n, depth): the canonical level counts (a plain breadth-first search on a CPU)
COUNTS = {
    (4, 4, 4, 15): [1, 2, 8, 26, 82, 218, 564, 1226, 2524, 4378, 7176, 9749, 12365, 11902, 10447, 6495],
    (6, 7, 4, 6): [1, 4, 25, 121, 568, 2144, 8231],
    (4, 5, 4, 6): [1, 3, 13, 49, 177, 542, 1626],
    (5, 4, 4, 6): [1, 2, 8, 26, 82, 220, 600],
    (5, 5, 3, 5): [1, 3, 13, 49, 177, 495],
}
FULL_7X6 = [1, 7, 49, 238, 1120, 4263, 16422]
SMALL = [(4, 5, 4, 6), (5, 4, 4, 6), (5, 5, 3, 5)]


# ------------------------------------------------------------------ the reference program
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """ref(mode, H, W, n, *args) -> records (board, score, nodes) from solver_check."""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(NATIVE, "solver_check.cpp"),
                    "-o", EXE], check=True, timeout=600)
    tmp = tmp_path_factory.mktemp("book_ref")
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
    path = str(ref.tmp / f"in_{H}_{W}_{n}_{len(boards)}.bin")
    np.ascontiguousarray(boards, np.int8).tofile(path)
    out = ref("scores", H, W, n, path)
    np.testing.assert_array_equal(out["board"], boards)
    return out["score"].astype(np.int32)


@pytest.fixture(scope="module")
def all_4x4(ref):
    return ref("table", 4, 4, 4)


# ------------------------------------------------------------------ a breadth-first search of this file's own
def bfs_levels(H, W, n, depth):
    """levels[t]: the set of (mine, theirs) of every reachable unfinished
    position with t stones, `mine` the side to move's; cell (r, c), row 0 the
    top row, is bit r * W + c."""
    lines_at = [[] for _ in range(H * W)]
    for r in range(H):
        for c in range(W):
            for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                cells = [(r + k * dr, c + k * dc) for k in range(n)]
                if all(0 <= rr < H and 0 <= cc < W for rr, cc in cells):
                    m = sum(1 << (rr * W + cc) for rr, cc in cells)
                    for rr, cc in cells:
                        lines_at[rr * W + cc].append(m)
    levels = [{(0, 0)}]
    for t in range(depth):
        nxt = set()
        for mine, theirs in levels[-1]:
            occ = mine | theirs
            for c in range(W):
                r = H - 1
                while r >= 0 and occ >> (r * W + c) & 1:
                    r -= 1
                if r < 0:
                    continue
                cell = r * W + c
                m2 = mine | 1 << cell
                if t + 1 == H * W or any(m2 & m == m for m in lines_at[cell]):
                    continue
                nxt.add((theirs, m2))
        levels.append(nxt)
    return levels


def mirrored(x, H, W):
    out = 0
    for r in range(H):
        row = x >> (r * W) & ((1 << W) - 1)
        out |= int(format(row, f"0{W}b")[::-1], 2) << (r * W)
    return out


def canonical_boards(level, H, W):
    """The level reduced by the mirror, as the set of board bytes ([H, W] int8, +1 the side to move)."""
    reps = {min((a, b), (mirrored(a, H, W), mirrored(b, H, W))) for a, b in level}
    out = set()
    for a, b in reps:
        board = np.array([(a >> i & 1) - (b >> i & 1) for i in range(H * W)], np.int8).reshape(H, W)
        out.add(min(board.tobytes(), board[:, ::-1].tobytes()))
    return out


def keys_of(boards):
    """cur + mask of az_solver.h: cell (col, row from the bottom) is bit col * (H + 1) + row."""
    _, H, W = boards.shape
    weight = np.array([[np.uint64(1) << np.uint64(c * (H + 1) + (H - 1 - r)) for c in range(W)] for r in range(H)],
                      np.uint64)
    mask = ((boards != 0).astype(np.uint64) * weight).sum(axis=(1, 2), dtype=np.uint64)
    cur = ((boards == 1).astype(np.uint64) * weight).sum(axis=(1, 2), dtype=np.uint64)
    return cur + mask


@pytest.mark.parametrize("H,W,n,depth", sorted(COUNTS))
def test_levels_are_the_breadth_first_search(H, W, n, depth):
    want = bfs_levels(H, W, n, depth)
    if (H, W) == (6, 7):
        assert [len(l) for l in want] == FULL_7X6
    with az.Solver(H, W, n, tt_log2=10) as s:
        counts = s.book_begin(depth)
        assert counts.tolist() == COUNTS[(H, W, n, depth)]
        assert s.book_info()[:2] == (depth, az.BOOK_BUILDING) and s.book_info()[2].tolist() == counts.tolist()
        for t in range(depth + 1):
            boards, scores = s.book_level(t)
            assert len(boards) == counts[t] and (scores == az.BOOK_NO_SCORE).all()
            stones = (boards != 0).sum(axis=(1, 2))
            assert (stones == t).all() and ((boards == 1).sum(axis=(1, 2)) == t // 2).all()
            keys = keys_of(boards)
            assert (keys[1:] > keys[:-1]).all(), f"level {t} is not strictly ascending"
            assert (keys <= keys_of(boards[:, :, ::-1])).all(), f"level {t} holds a key above its mirror's"
            got = {min(b.tobytes(), b[:, ::-1].tobytes()) for b in boards}
            assert len(got) == len(boards)
            assert got == canonical_boards(want[t], H, W), f"level {t}"
        # strided read-out, and its bounds
        boards, _ = s.book_level(depth)
        part, _ = s.book_level(depth, 1, (len(boards) - 1 + 2) // 3, 3)
        np.testing.assert_array_equal(part, boards[1::3])
        with pytest.raises(az.AzError, match="passes the level"):
            s.book_level(depth, 0, len(boards) + 1, 1)
        with pytest.raises(az.AzError, match="levels 0"):
            s.book_level(depth + 1, 0, 1, 1)
    if (H, W) == (4, 4):
        assert sum(len(l) for l in want) == 134289


# ------------------------------------------------------------------ finished books, built once
def read_all(s, depth):
    levels = [s.book_level(t) for t in range(depth + 1)]
    return np.concatenate([b for b, _ in levels]), np.concatenate([sc for _, sc in levels])


@pytest.fixture(scope="module")
def books(tmp_path_factory):
    """books(H, W, n, depth) -> (path of the one-shot build's file, its boards, its scores)."""
    tmp = tmp_path_factory.mktemp("books")
    cache = {}

    def get(H, W, n, depth):
        key = (H, W, n, depth)
        if key not in cache:
            path = str(tmp / f"{H}x{W}x{n}_{depth}.book")
            with az.Solver(H, W, n, tt_log2=20) as s:
                s.book_begin(depth)
                assert s.book_solve(ALL, NO_BUDGET) == (0, 0)
                s.book_finish()
                assert s.book_info()[:2] == (depth, az.BOOK_FINISHED)
                s.book_save(path)
                cache[key] = (path,) + read_all(s, depth)
        return cache[key]

    return get


def test_4x4_full_book_answers_every_position(all_4x4, books):
    path, _, _ = books(4, 4, 4, 15)
    with az.Solver(4, 4, 4, tt_log2=16) as s:
        scores, status, _ = s.solve(all_4x4["board"], 1)
        assert (status == az.SOLVER_UNSOLVED).any(), "a budget of 1 node solves 4x4: the next assertions show nothing"
        s.book_load(path)
        scores, status, nodes = s.solve(all_4x4["board"], 1)
        assert not status.any(), f"{int(status.sum())} unsolved"
        np.testing.assert_array_equal(scores, all_4x4["score"])
        assert (nodes == 0).all()


@pytest.mark.parametrize("H,W,n,depth", SMALL)
def test_scores_of_the_other_boards(ref, books, H, W, n, depth):
    path, boards, scores = books(H, W, n, depth)
    assert len(boards) == sum(COUNTS[(H, W, n, depth)]) and (scores != az.BOOK_NO_SCORE).all()
    np.testing.assert_array_equal(scores, ref_scores(ref, H, W, n, boards))
    with az.Solver(H, W, n, tt_log2=10) as s:
        s.book_load(path)
        for b in (boards, boards[:, :, ::-1]):
            got, status, nodes = s.solve(b, 1)
            assert not status.any() and (nodes == 0).all()
            np.testing.assert_array_equal(got, scores)


def test_unreachable_input_is_a_miss(ref, books):
    """The second player's stone under the first player's only stone: parse_board
    takes it, play cannot reach it, so the book does not hold it."""
    board = np.zeros((1, 4, 4), np.int8)
    board[0, 3, 0], board[0, 2, 0] = -1, 1
    with az.Solver(4, 4, 4, tt_log2=16) as s:
        s.book_load(books(4, 4, 4, 15)[0])
        scores, status, nodes = s.solve(board, NO_BUDGET)
    assert status[0] == az.SOLVER_SOLVED and nodes[0] > 0
    assert scores[0] == ref_scores(ref, 4, 4, 4, board)[0]


def test_budget_leaves_positions_for_later(books):
    H, W, n, depth = 4, 5, 4, 6
    _, _, want = books(H, W, n, depth)
    with az.Solver(H, W, n, tt_log2=20) as s:
        total = int(s.book_begin(depth)[depth])
        remaining, unsolved = s.book_solve(ALL, 1)
        assert unsolved > 0 and remaining == unsolved and remaining <= total
        with pytest.raises(az.AzError, match="no score yet"):
            s.book_finish()
        assert s.book_info()[1] == az.BOOK_BUILDING
        _, scores = s.book_level(depth)
        assert int((scores == az.BOOK_NO_SCORE).sum()) == remaining
        for _ in range(3):
            if remaining == 0:
                break
            remaining, unsolved = s.book_solve(ALL, NO_BUDGET)
        assert (remaining, unsolved) == (0, 0)
        s.book_finish()
        np.testing.assert_array_equal(read_all(s, depth)[1], want)


def test_chunks_and_resume_give_the_same_bytes(books, tmp_path):
    H, W, n, depth = 4, 5, 4, 6
    want = open(books(H, W, n, depth)[0], "rb").read()
    part, whole = str(tmp_path / "part.book"), str(tmp_path / "whole.book")
    total = COUNTS[(H, W, n, depth)][depth]
    with az.Solver(H, W, n, tt_log2=20) as s:
        s.book_begin(depth)
        for k in range(1, 4):
            assert s.book_solve(100, NO_BUDGET) == (total - 100 * k, 0)
        s.book_save(part)
    with az.Solver(H, W, n, tt_log2=14) as s:
        s.configure(steps_per_launch=32)
        s.book_load(part)
        assert s.book_info()[:2] == (depth, az.BOOK_BUILDING)
        remaining, calls = total - 300, 0
        while remaining:
            before = remaining
            remaining, unsolved = s.book_solve(100, NO_BUDGET)
            assert unsolved == 0 and remaining == max(0, before - 100)
            calls += 1
        assert calls == (total - 300 + 99) // 100
        s.book_finish()
        s.book_save(whole)
    assert open(whole, "rb").read() == want
    assert open(part, "rb").read() != want
    # build_book, chunked and through a file, ends at the same bytes too
    with az.Solver(H, W, n, tt_log2=18) as s:
        seen = []
        assert s.build_book(depth, NO_BUDGET, chunk=700, path=part, report=lambda *a: seen.append(a)) is True
        assert [a[1] for a in seen] == [total - 700, total - 1400, 0]
    assert open(part, "rb").read() == want


def test_file_refusals_and_an_unfinished_book(books, tmp_path):
    path4 = books(4, 4, 4, 15)[0]
    data = open(path4, "rb").read()
    cut, flipped, unfinished = (str(tmp_path / name) for name in ("cut.book", "flipped.book", "unfinished.book"))
    open(cut, "wb").write(data[:len(data) // 2])
    open(flipped, "wb").write(data[:1000] + bytes([data[1000] ^ 4]) + data[1001:])
    with az.Solver(4, 5, 4, tt_log2=10) as s:
        with pytest.raises(az.AzError, match="another geometry"):
            s.book_load(path4)
        assert s.book_info()[:2] == (-1, az.BOOK_NONE)
    empty = np.zeros((1, 4, 4), np.int8)
    with az.Solver(4, 4, 4, tt_log2=16) as s:
        with pytest.raises(az.AzError, match="short file"):
            s.book_load(cut)
        with pytest.raises(az.AzError, match="checksum mismatch"):
            s.book_load(flipped)
        with pytest.raises(az.AzError, match="cannot read"):
            s.book_load(str(tmp_path / "none.book"))
        with pytest.raises(az.AzError, match="no book"):
            s.book_save(unfinished)
        s.book_begin(9)
        s.book_solve(2000, NO_BUDGET)
        s.book_save(unfinished)
    with az.Solver(4, 4, 4, tt_log2=16) as s:
        s.book_load(unfinished)
        assert s.book_info()[:2] == (9, az.BOOK_BUILDING)
        _, status, nodes = s.solve(empty, 1)  # lookups are off: the split's jobs run, one node each
        assert status[0] == az.SOLVER_UNSOLVED or nodes[0] > 0
        remaining, _ = s.book_solve(ALL, NO_BUDGET)
        assert remaining == 0
        s.book_finish()
        scores, status, nodes = s.solve(empty, 1)
        assert (scores[0], status[0], nodes[0]) == (0, az.SOLVER_SOLVED, 0)
        with pytest.raises(az.AzError, match="no book is being built"):
            s.book_solve(ALL, NO_BUDGET)


# ------------------------------------------------------------------ the arena and MCTS
@pytest.fixture
def small_board():
    saved = (ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity,
             ConfigSolver.node_budget, ConfigSolver.tt_log2, ConfigSolver.split_stones, ConfigSolver.book_path,
             ConfigSelfPlay.mcts_iterations, ConfigServing.evaluation_games_number)

    def set_(H, W, n, node_budget, book_path=""):
        ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n = H, W, n
        ConfigConnectN.gravity = True
        ConfigSolver.node_budget, ConfigSolver.tt_log2, ConfigSolver.book_path = node_budget, 20, book_path
        exact.close_solvers()

    yield set_
    exact.close_solvers()
    (ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity,
     ConfigSolver.node_budget, ConfigSolver.tt_log2, ConfigSolver.split_stones, ConfigSolver.book_path,
     ConfigSelfPlay.mcts_iterations, ConfigServing.evaluation_games_number) = saved


def arena(H, W, games=4):
    shape = Board().full_state.shape
    a = PolicyValueModel(input_dim=shape, action_space=W, seed=1)
    b = PolicyValueModel(input_dim=shape, action_space=W, seed=2)
    scores = []
    evaluate.evaluate_two_models_batched(a, b, n_games=games, deterministic=True, seed=7, evaluate_with_solver=True,
                                         solver_scores=scores)
    return scores, dict(evaluate.solver_report)


def test_arena_scores_are_the_same_with_the_book(books, small_board):
    path = books(4, 5, 4, 6)[0]
    small_board(4, 5, 4, 1 << 30)
    without, report = arena(4, 5)
    assert report["unsolved"] == 0 and len(without) >= 8
    small_board(4, 5, 4, 1 << 30, path)
    with_book, report = arena(4, 5)
    assert exact.get_solver().book_info()[:2] == (6, az.BOOK_FINISHED)
    assert with_book == without and report == {"scored": len(without), "unsolved": 0}


def test_4x4_book_carries_the_arena_and_mcts_on_a_budget_of_one(books, small_board):
    path = books(4, 4, 4, 15)[0]
    moves = None
    for book_path in ("", path):
        small_board(4, 4, 4, 1, book_path)
        ConfigSelfPlay.mcts_iterations = 12
        moves = Board.get_all_possible_moves()
        scores, report = arena(4, 4)
        mcts = MCTS(Board(), moves, use_solver=True)
        if not book_path:
            assert report["unsolved"] > 0
            with pytest.raises(exact.SolverBudgetError):
                mcts.search(12)
        else:
            assert report["unsolved"] == 0 and report["scored"] == len(scores) >= 8
            mcts.search(12)
            assert sum(e.visit_count for e in mcts.current_root.edges) >= 11


def test_missing_book_file_says_so(small_board, tmp_path):
    small_board(4, 4, 4, 1, str(tmp_path / "absent.book"))
    with pytest.raises(FileNotFoundError, match="absent.book"):
        exact.get_solver()


# ------------------------------------------------------------------ 6 wide, 5 high
def test_6x5_book_reaches_the_empty_board():
    """Depth 10 is the frontier test_empty_6x5_through_the_host_split searches;
    the book holds it mirror-reduced, and afterwards the empty board, a draw, costs no node."""
    H, W, n, depth = 5, 6, 4, 10
    t0 = time.perf_counter()
    with az.Solver(H, W, n, tt_log2=24) as s:
        assert s.build_book(depth, 1 << 21, chunk=1 << 20) is True
        print(f"6x5 depth {depth}: {int(s.book_info()[2][depth])} positions, {time.perf_counter() - t0:.2f} s")
        scores, status, nodes = s.solve(np.zeros((1, H, W), np.int8), 1)
        assert (scores[0], status[0], nodes[0]) == (0, az.SOLVER_SOLVED, 0)
        level = int(s.book_info()[2][depth])
        boards, want = s.book_level(depth, 0, 256, level // 256)
    with az.Solver(H, W, n, tt_log2=24) as plain:
        scores, status, nodes = plain.solve(boards, 1 << 21)
        assert not status.any() and (nodes > 0).any()
        np.testing.assert_array_equal(scores, want)
