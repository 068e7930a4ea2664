"""The reference's exact-solver seam (exact_solvers/c4_exact_solver.py:24-85)
on the device solver (engine.Solver, csrc/az_solver.hip).

The reference pipes move strings to a prebuilt c4solver with a 7x6 opening
book; here the positions are solved by libaz, any gravity board it accepts
(W <= 16, W * (H + 1) <= 56), with the c4solver's score convention.  A
position is searched within ConfigSolver.node_budget nodes; an opening book of
this project's own (ConfigSolver.book_path, built by `python -m
custom_alphazero.exact_solvers --build-book`) answers the shallow positions no
budget reaches, as the reference's book does on 7x6.  The solver is off until
ConfigSolver.node_budget > 0 (NotImplementedError, as before), and a position
that is not in the book and whose search passes the budget raises
SolverBudgetError.

The three reference functions keep their names and signatures; the *_batch
forms answer many boards from one solver call (the batched arena, the MCTS
evaluator).
"""
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from custom_alphazero import engine as az
from custom_alphazero.config import ConfigConnectN, ConfigGeneral, ConfigSolver
from custom_alphazero.connect_n.board import Board
from custom_alphazero.connect_n.move import Move

MAX_WIDTH, MAX_BITS = 16, 56


class SolverBudgetError(RuntimeError):
    """A position came back unsolved: its search passed ConfigSolver.node_budget
    nodes (or its host split passed max_jobs)."""


_solvers = {}  # (height, width, n, device) -> engine.Solver, created on first use


def solver_enabled() -> bool:
    return int(ConfigSolver.node_budget) > 0


def check_solver_config():
    """NotImplementedError unless the device solver is on and takes ConfigConnectN's board."""
    if not solver_enabled():
        raise NotImplementedError("the exact solver is off: set ConfigSolver.node_budget > 0 "
                                  "(the c4solver binary is not run here)")
    if ConfigGeneral.game != "connect_n":
        raise NotImplementedError("the exact solver plays Connect-N only")
    c = ConfigConnectN
    H, W, n = int(c.board_height), int(c.board_width), int(c.n)
    if not c.gravity:
        raise NotImplementedError("the exact solver takes gravity boards only")
    if not (H >= 2 and 2 <= W <= MAX_WIDTH and W * (H + 1) <= MAX_BITS and 2 <= n <= max(H, W)):
        raise NotImplementedError(
            f"the exact solver takes boards with H, W >= 2, W <= {MAX_WIDTH}, W * (H + 1) <= {MAX_BITS} and "
            f"2 <= n <= max(H, W); got {W}x{H}, n={n}")


def get_solver() -> az.Solver:
    """The module-level solver of ConfigConnectN's (H, W, n) on ConfigSolver.device,
    with the opening book of ConfigSolver.book_path loaded when that is set: a
    missing file is FileNotFoundError, a file of another geometry or a damaged
    one engine.AzError naming which, a book whose build is not finished RuntimeError."""
    check_solver_config()
    c = ConfigConnectN
    book_path = str(ConfigSolver.book_path or "")
    key = (int(c.board_height), int(c.board_width), int(c.n), int(ConfigSolver.device), book_path)
    if key not in _solvers:
        if book_path and not os.path.isfile(book_path):
            raise FileNotFoundError(f"ConfigSolver.book_path = {book_path!r}: no such file (build it with "
                                    f"python -m custom_alphazero.exact_solvers --build-book)")
        s = az.Solver(key[0], key[1], key[2], tt_log2=int(ConfigSolver.tt_log2), device=key[3])
        try:
            s.configure(split_stones=int(ConfigSolver.split_stones), max_jobs=int(ConfigSolver.max_jobs))
            if book_path:
                s.book_load(book_path)
                if s.book_info()[1] != az.BOOK_FINISHED:
                    raise RuntimeError(f"ConfigSolver.book_path = {book_path!r}: the book's build is not finished "
                                       f"(go on with --build-book)")
        except Exception:
            s.close()
            raise
        _solvers[key] = s
    return _solvers[key]


def close_solvers():
    """Free the module-level solvers (their tables with them)."""
    for s in _solvers.values():
        s.close()
    _solvers.clear()


def solve_arrays(arrays: Sequence[np.ndarray]) -> List[Optional[int]]:
    """Exact scores of boards given as arrays with +1 the side to move: one
    solver call; None where the position came back unsolved."""
    if not len(arrays):
        return []
    scores, status, _ = get_solver().solve(np.stack(arrays).astype(np.int8), int(ConfigSolver.node_budget))
    return [None if st else int(sc) for sc, st in zip(scores, status)]


def _require_solved(results, arrays):
    for r, a in zip(results, arrays):
        if r is None:
            raise SolverBudgetError(
                f"a position with {int(np.count_nonzero(a))} stones was not solved within "
                f"ConfigSolver.node_budget = {int(ConfigSolver.node_budget)} nodes")


def _replay(line: str) -> Optional[np.ndarray]:
    """A line of 1-based columns played from the empty board, as the array with
    +1 the side to move; None when it is no legal unfinished game."""
    if not line or not line.isdigit():
        return None
    board = Board()
    for ch in line:
        x = int(ch) - 1
        if board.is_game_over() or not 0 <= x < board.board_width or board.array[0, x] != board.empty:
            return None
        board.play(Move(True, x), keep_same_player=True)
    if board.is_game_over():
        return None
    return board.array.copy()


def evaluate_boards_with_solution(boards_as_list_moves: str) -> Optional[List[int]]:
    """c4_exact_solver.py:24-48: one line of played moves per board (columns
    from 1, Board.repr_list_played_moves) -> the boards' scores for the side to
    move; None for input the c4solver would reject (the reference prints and
    returns None)."""
    check_solver_config()
    text = boards_as_list_moves[:-1] if boards_as_list_moves.endswith("\n") else boards_as_list_moves
    arrays = [_replay(line) for line in text.split("\n")]
    if any(a is None for a in arrays):
        print("Incorrect input!")
        return None
    results = solve_arrays(arrays)
    _require_solved(results, arrays)
    return results


def _to_move_array(board: Board) -> np.ndarray:
    """board.array with +1 the side to move (black to move: negated)."""
    return (board.array * board.turn).astype(np.int8)


def _children(board: Board):
    assert not board.is_game_over()
    child_boards = [board.play(move, on_copy=True) for move in board.moves]
    ending_moves = np.array([child_board.is_game_over() for child_board in child_boards])
    all_non_ending_boards = [board] + [c for c, over in zip(child_boards, ending_moves) if not over]
    return ending_moves, [_to_move_array(b) for b in all_non_ending_boards]


def _ranked(ending_moves: np.ndarray, results: List[int]) -> Tuple[List[int], float]:
    """c4_exact_solver.py:67-74 from the scores of [board] + its non-ending children."""
    exact_child_values = np.zeros(len(ending_moves))
    exact_child_values[ending_moves] = -np.inf
    exact_child_values[~ending_moves] = results[1:]
    ranked_moves_indexes = list(np.argsort(exact_child_values))
    exact_value = float(np.sign(results[0]))  # we want a value in {-1, 0, 1} for the board
    return ranked_moves_indexes, exact_value


def exact_ranked_moves_and_value(board: Board) -> Tuple[List[int], float]:
    """c4_exact_solver.py:51-74.  The board goes through board.array and
    board.turn, so it need not carry its played moves."""
    ending_moves, arrays = _children(board)
    results = solve_arrays(arrays)
    assert results is not None
    _require_solved(results, arrays)
    return _ranked(ending_moves, results)


def exact_ranked_moves_and_value_batch(boards: Sequence[Board]) -> List[Optional[Tuple[List[int], float]]]:
    """exact_ranked_moves_and_value of every board from one solver call; None
    for a board that (or a child of which) came back unsolved."""
    parts = [_children(b) for b in boards]
    flat = [a for _, arrays in parts for a in arrays]
    results = solve_arrays(flat)
    out, at = [], 0
    for ending_moves, arrays in parts:
        mine = results[at:at + len(arrays)]
        at += len(arrays)
        out.append(None if any(r is None for r in mine) else _ranked(ending_moves, mine))
    return out


def _policy(board: Board, all_possible_moves: List[Move], ranked_moves_indexes) -> np.ndarray:
    exact_policy = np.zeros(len(all_possible_moves)).astype(float)
    best_move_index = int(ranked_moves_indexes[0])
    keys = [m.key() for m in all_possible_moves]
    best_all_moves_index = keys.index(board.moves[best_move_index].key())
    exact_policy[best_all_moves_index] = 1.0
    return exact_policy


def exact_policy_and_value(board: Board, all_possible_moves: List[Move]) -> Tuple[np.ndarray, float]:
    """c4_exact_solver.py:77-85: the one-hot policy of the first ranked move, and the sign."""
    ranked_moves_indexes, exact_value = exact_ranked_moves_and_value(board)
    return _policy(board, all_possible_moves, ranked_moves_indexes), exact_value


def exact_policy_and_value_batch(boards: Sequence[Board], all_possible_moves: List[Move]):
    """exact_policy_and_value of every board from one solver call: (policies
    [n, A], values [n]); SolverBudgetError if any position is unsolved."""
    ranked = exact_ranked_moves_and_value_batch(boards)
    policies = np.zeros((len(boards), len(all_possible_moves)))
    values = np.zeros(len(boards))
    for i, (board, r) in enumerate(zip(boards, ranked)):
        if r is None:
            raise SolverBudgetError(
                f"a position at or below {int(np.count_nonzero(board.array))} stones was not solved within "
                f"ConfigSolver.node_budget = {int(ConfigSolver.node_budget)} nodes")
        policies[i], values[i] = _policy(board, all_possible_moves, r[0]), r[1]
    return policies, values
