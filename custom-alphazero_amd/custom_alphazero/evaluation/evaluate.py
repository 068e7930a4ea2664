"""Arena: two models play each other (reference evaluation/evaluate.py:29-134).

* `_single_game_evaluation` / `evaluate_two_models` keep the reference's
  signatures and game loop (one game at a time; per-move fresh MCTS with the
  model to move, or the raw policy when evaluate_with_mcts is False).
* `evaluate_two_models_batched` plays all evaluation games at once on the
  device: one engine per model, each ply every unfinished game is searched by
  the engine of the model to move (az_tree_reset / az_tree_release keep the
  other engine's copy idle).  With deterministic=True the per-game results are
  those of the sequential loop; with stochastic play each game draws from its
  own RandomState(seed + game) instead of the shared np.random stream (the
  only difference; the draw count per move is the reference's).  Dirichlet
  root noise (ConfigMCTS.enable_dirichlet_noise) is drawn the same way: the
  search's root-noise vectors, then play's draw, from the game's stream.
The exact-solver scoring path (evaluate.py:53-59: how the solver ranks the
current model's raw-policy moves) runs on the device solver
(exact_solvers/c4_exact_solver.py) once ConfigSolver.node_budget > 0; with
the default 0 it raises NotImplementedError, as it does for chess, for boards
the solver does not take and together with evaluate_with_mcts
(evaluate.py:100-102).  The one deviation from the reference: it has an
opening book, this has a budget -- a move whose position comes back unsolved
is left out of the mean and counted; `solver_report` holds {"scored",
"unsolved"} of the last call, and with nothing scored the solver score is None.

The game is ConfigGeneral.game, read at call time (evaluate.py:16-26 picks
Board, Move and get_all_possible_moves by it): "connect_n" as above, "chess"
with chess.board.Board and chess.utils.get_all_possible_moves.  Rules of a
chess arena game:
* decisive means bool(board.get_result()) -- chess get_result takes no
  keep_same_player; on the canonical board a checkmate is a win for the side
  that just moved, and the last mover is credited; everything else is a draw;
* a game that reaches ConfigSelfPlay.chess_max_plies plies without an outcome
  is a draw (the engine's own addition: the reference has no cap);
* greedy is the reference's expression on the game's own board,
  fullmove_number > ConfigMCTS.index_move_greedy;
* the models alternate as in evaluate.py:39, 61-62, 75-83;
* a model is a PolicyValueModel (a network engine) or, under MCTS, any other
  callable model(x) -> (probabilities, value) (a host-evaluator engine);
* Dirichlet root noise stays refused here (check_mcts_config("chess"): the
  chess engine has it in self-play and as ChessEngine.tree_search(noise=),
  which this arena is not wired to yet), and `trace` collects the final
  boards' az_chess_pos records.
The batched chess arena searches each ply with az_chess_tree_release /
_reset / _search / _play; its raw-policy mode encodes every live board in one
batched kernels.encode.  deterministic=True gives the sequential loop's
per-game results and final positions; stochastic play draws from each game's
own stream, one draw per move as Connect-N.
"""
from copy import deepcopy
from typing import List, Optional, Tuple

import numpy as np

from custom_alphazero import engine as az
from custom_alphazero.config import (ConfigConnectN, ConfigGeneral, ConfigMCTS, ConfigModel, ConfigSelfPlay,
                                     ConfigServing, check_mcts_config)
from custom_alphazero.connect_n.board import Board
from custom_alphazero.connect_n.move import Move
from custom_alphazero.exact_solvers import c4_exact_solver as exact
from custom_alphazero.mcts.mcts import MCTS, root_noise_rows
from custom_alphazero.mcts.utils import normalize_probabilities

get_all_possible_moves = Board.get_all_possible_moves

# moves the solver scored / could not score within its budget, in the last arena call
solver_report = {"scored": 0, "unsolved": 0}


def _check_solver(evaluate_with_mcts: bool = False):
    """The refusals of solver scoring, all NotImplementedError."""
    if _game()[2]:
        raise NotImplementedError("solver scoring is not implemented for chess")
    exact.check_solver_config()
    if evaluate_with_mcts:
        raise NotImplementedError("solver scoring under MCTS is not implemented (evaluate.py:100-102)")


def _solver_move_score(ranked_moves_indexes, board: Board, move: Move) -> float:
    """evaluate.py:55-59, the reference's own expression: the argsort result
    indexed by the move's index."""
    return 1 - (ranked_moves_indexes[board.moves.index(move)] + 1) / len(board.moves)


def _game():
    """(Board, get_all_possible_moves, is chess) of ConfigGeneral.game, resolved
    per call (evaluate.py:16-26 resolves it at import)."""
    if ConfigGeneral.game == "connect_n":
        return Board, get_all_possible_moves, False
    if ConfigGeneral.game == "chess":
        from custom_alphazero.chess.board import Board as ChessBoard
        from custom_alphazero.chess.utils import get_all_possible_moves as chess_moves
        return ChessBoard, chess_moves, True
    raise NotImplementedError(f"no arena for ConfigGeneral.game = {ConfigGeneral.game!r}")


def _chess_legal_policy(probabilities, board, all_possible_moves):
    return normalize_probabilities(probabilities[board.legal_moves_mask(all_possible_moves)])


def _chess_pick(board, legal, deterministic: bool, rng):
    """The raw-policy move of a chess board: argmax, or rng.choice's one draw over the move indices."""
    moves = board.moves
    if deterministic:
        return moves[int(np.argmax(legal))]
    return moves[int(rng.choice(len(moves), 1, p=legal).item())]


def _single_chess_game(current_model, previous_model, game_index: int, all_possible_moves,
                       evaluate_with_mcts: bool, deterministic: bool, rng, trace):
    """_single_game_evaluation's loop (evaluate.py:29-98) on a chess board."""
    ChessBoard = _game()[0]
    cap = max(int(ConfigSelfPlay.chess_max_plies), 1)
    model = current_model if game_index % 2 == 0 else previous_model
    plies = 0
    if not evaluate_with_mcts:
        board = ChessBoard()
        while not board.is_game_over() and plies < cap:
            probabilities, _ = model(np.expand_dims(board.full_state, axis=0))
            legal = _chess_legal_policy(az._as_numpy(probabilities).ravel(), board, all_possible_moves)
            board.play(_chess_pick(board, legal, deterministic, rng), keep_same_player=True)
            plies += 1
            if not board.is_game_over():
                model = previous_model if model is current_model else current_model
    else:
        mcts = MCTS(board=ChessBoard(), all_possible_moves=all_possible_moves, concurrency=False,
                    model=model, plays_inferences={})
        while not mcts.board.is_game_over() and plies < cap:
            greedy = mcts.board.fullmove_number > ConfigMCTS.index_move_greedy
            mcts.search(ConfigSelfPlay.mcts_iterations)
            if rng is not np.random and not deterministic:
                # play draws its move from np.random: route this game's stream through it
                state = np.random.get_state()
                np.random.set_state(rng.get_state())
                try:
                    mcts.play(greedy, deterministic=deterministic)
                finally:
                    rng.set_state(np.random.get_state())
                    np.random.set_state(state)
            else:
                mcts.play(greedy, deterministic=deterministic)
            plies += 1
            if not mcts.board.is_game_over() and plies < cap:
                model = previous_model if mcts.model is current_model else current_model
                mcts = MCTS(board=mcts.board, all_possible_moves=all_possible_moves,
                            concurrency=False, model=model, plays_inferences={})
        board = mcts.board
    if trace is not None:
        trace.append(board._pos.copy())
    if board.get_result():  # None (the cap) and 0 (a draw) are not decisive
        return (1 if current_model is model else -1), []
    return 0, []


def _policy_move(model, board: Board, all_possible_moves: List[Move], deterministic: bool, rng):
    """evaluate.py:40-53: raw-policy move (legal probabilities normalised)."""
    probabilities, _ = model(np.expand_dims(board.full_state, axis=0))
    probabilities = probabilities.numpy().ravel()
    legal = normalize_probabilities(probabilities[board.legal_moves_mask(all_possible_moves)])
    if deterministic:
        return board.moves[int(np.argmax(legal))]
    return rng.choice(board.moves, 1, p=legal).item()


def _single_game_evaluation(current_model, previous_model, game_index: int,
                            all_possible_moves: List[Move], evaluate_with_mcts: bool,
                            evaluate_with_solver: bool, deterministic: bool,
                            rng=None, trace: Optional[list] = None,
                            report: Optional[dict] = None) -> Tuple[int, Optional[List[float]]]:
    """evaluate.py:29-98.  Additions: `rng` replaces the global np.random;
    `trace` collects the final board's array; `report` counts the scored and
    unsolved moves (default: solver_report, reset)."""
    solver_scores = []
    if evaluate_with_solver:
        _check_solver()
        if report is None:
            report = solver_report
            report.update(scored=0, unsolved=0)
    rng = np.random if rng is None else rng
    if _game()[2]:
        return _single_chess_game(current_model, previous_model, game_index, all_possible_moves,
                                  evaluate_with_mcts, deterministic, rng, trace)
    model = current_model if game_index % 2 == 0 else previous_model
    if not evaluate_with_mcts:
        board = Board()
        while not board.is_game_over():
            move = _policy_move(model, board, all_possible_moves, deterministic, rng)
            if evaluate_with_solver and model is current_model:
                try:
                    ranked_moves_indexes, _ = exact.exact_ranked_moves_and_value(board)
                    solver_scores.append(_solver_move_score(ranked_moves_indexes, board, move))
                    report["scored"] += 1
                except exact.SolverBudgetError:
                    report["unsolved"] += 1
            board.play(move, keep_same_player=True)
            if not board.is_game_over():
                model = previous_model if model is current_model else current_model
    else:
        mcts = MCTS(board=Board(), all_possible_moves=all_possible_moves, concurrency=False,
                    model=model, plays_inferences={})
        while not mcts.board.is_game_over():
            greedy = mcts.board.fullmove_number > ConfigMCTS.index_move_greedy
            if rng is not np.random and (not deterministic or ConfigMCTS.enable_dirichlet_noise):
                # the shim draws (root noise in search, the move in play) from
                # np.random; route this game's stream through it
                state = np.random.get_state()
                np.random.set_state(rng.get_state())
                try:
                    mcts.search(ConfigSelfPlay.mcts_iterations)
                    mcts.play(greedy, deterministic=deterministic)
                finally:
                    rng.set_state(np.random.get_state())
                    np.random.set_state(state)
            else:
                mcts.search(ConfigSelfPlay.mcts_iterations)
                mcts.play(greedy, deterministic=deterministic)
            if not mcts.board.is_game_over():
                model = previous_model if mcts.model is current_model else current_model
                mcts = MCTS(board=mcts.board, all_possible_moves=all_possible_moves,
                            concurrency=False, model=model, plays_inferences={})
        board = mcts.board
    if trace is not None:
        trace.append(board.array.copy())
    result = board.get_result(keep_same_player=True)
    if result:
        return (1 if current_model is model else -1), solver_scores
    return 0, solver_scores


def _score(results) -> float:
    """evaluate.py:120-134: wins / decisive games, 0.5 when all draws."""
    results = np.asarray(results)
    if np.all(results == 0):
        return 0.5
    return float((results == 1).sum() / (results != 0).sum())


def evaluate_two_models(model, other_model, evaluate_with_mcts: bool = False,
                        evaluate_with_solver: bool = False, deterministic: bool = False):
    """evaluate.py:101-134: (score of `model`, solver score or None)."""
    if evaluate_with_solver:
        _check_solver(evaluate_with_mcts)
        solver_report.update(scored=0, unsolved=0)
    all_possible_moves = _game()[1]()
    results, solver_scores = [], []
    for g in range(ConfigServing.evaluation_games_number):
        result, scores = _single_game_evaluation(model, other_model, g, all_possible_moves, evaluate_with_mcts,
                                                 evaluate_with_solver, deterministic, report=solver_report)
        results.append(result)
        solver_scores.extend(scores)
    solver_score = np.mean(solver_scores) if evaluate_with_solver and len(solver_scores) else None
    return _score(results), solver_score


def _arena_engine(model, n_slots: int) -> az.Engine:
    check_mcts_config()
    c = ConfigConnectN
    eng = az.Engine(c.board_height, c.board_width, c.n, c.gravity,
                    max(ConfigSelfPlay.mcts_iterations, 1), slots=n_slots,
                    evaluator=az.EVAL_NETWORK, index_move_greedy=ConfigMCTS.index_move_greedy,
                    exploration_constant=ConfigMCTS.exploration_constant,
                    filters=ConfigModel.filters, depth=ConfigModel.depth,
                    value_hidden=ConfigModel.value_hidden, bn_epsilon=ConfigModel.bn_epsilon,
                    lanes=1, dirichlet_noise=ConfigMCTS.enable_dirichlet_noise,
                    dirichlet_alpha=ConfigMCTS.dirichlet_noise_value,
                    dirichlet_ratio=ConfigMCTS.dirichlet_noise_ratio)
    eng.set_weights(model.engine_weights())
    return eng


def _chess_arena_engine(model, n_slots: int) -> az.ChessEngine:
    """One chess engine of n_slots trees for `model`: a network engine for a
    PolicyValueModel, a host-evaluator engine for any other callable."""
    check_mcts_config("chess")
    sims = max(ConfigSelfPlay.mcts_iterations, 1)
    if model is not None and hasattr(model, "engine_weights"):
        evaluator = az.EVAL_NETWORK
    elif callable(model):
        evaluator = az.EVAL_HOST
    else:
        raise TypeError("the chess arena needs PolicyValueModels or callables model(x) -> (probabilities, value)")
    eng = az.ChessEngine(mcts_iterations=sims, slots=n_slots, evaluator=evaluator,
                         max_plies=max(ConfigSelfPlay.chess_max_plies, 1),
                         index_move_greedy=ConfigMCTS.index_move_greedy,
                         exploration_constant=ConfigMCTS.exploration_constant,
                         filters=ConfigModel.filters, depth=ConfigModel.depth,
                         value_hidden=ConfigModel.value_hidden, bn_epsilon=ConfigModel.bn_epsilon,
                         arena_edges=160 * sims + 4096, lanes=1)
    if evaluator == az.EVAL_NETWORK:
        eng.set_weights(model.engine_weights())
    else:
        eng.set_host_evaluator(model)
    return eng


def _chess_arena_batched(model, other_model, n: int, evaluate_with_mcts: bool, deterministic: bool,
                         seed: int, trace: Optional[list]):
    from custom_alphazero.chess.board import full_states
    from custom_alphazero.chess.move import Move as ChessMove
    ChessBoard, chess_moves, _ = _game()
    all_moves = chess_moves()
    cap = max(int(ConfigSelfPlay.chess_max_plies), 1)
    boards = [ChessBoard() for _ in range(n)]
    side = np.array([g % 2 for g in range(n)])  # 0: `model` to move, 1: `other_model`
    rngs = [np.random.RandomState((seed + g) % 2 ** 32) for g in range(n)]
    models = (model, other_model)
    engines = [_chess_arena_engine(m, n) for m in models] if evaluate_with_mcts else None
    active = [set(), set()]
    last_side = np.zeros(n, np.int64)
    try:
        for _ply in range(cap):
            live = [g for g in range(n) if not boards[g].is_game_over()]
            if not live:
                break
            for s in (0, 1):
                idx = [g for g in live if side[g] == s]
                if not idx:
                    continue
                if not evaluate_with_mcts:
                    x = full_states([boards[g] for g in idx])  # one batched encode
                    probs = az._as_numpy(models[s](x)[0])
                    for k, g in enumerate(idx):
                        legal = _chess_legal_policy(probs[k], boards[g], all_moves)
                        boards[g].play(_chess_pick(boards[g], legal, deterministic, rngs[g]),
                                       keep_same_player=True)
                else:
                    eng = engines[s]
                    stale = sorted(active[s] - set(idx))
                    if stale:
                        eng.tree_release(stale)
                    eng.tree_reset(idx, np.stack([boards[g]._pos for g in idx]))
                    active[s] = set(idx)
                    eng.tree_search(ConfigSelfPlay.mcts_iterations)
                    u = None
                    if not deterministic:
                        u = np.zeros(n)
                        for g in idx:
                            u[g] = rngs[g].random_sample()  # np.random.choice's one draw (mcts.py:201)
                    # the games move in lockstep from one start position: one greedy flag per ply
                    greedy = {boards[g].fullmove_number > ConfigMCTS.index_move_greedy for g in idx}
                    if len(greedy) != 1:
                        raise RuntimeError("the live games disagree on fullmove_number")
                    out = eng.tree_play(u, greedy=greedy.pop(), deterministic=deterministic)
                    for g in idx:
                        boards[g].play(ChessMove.from_code(int(out["moves"][g])), keep_same_player=True)
                last_side[idx] = s
            side = 1 - side
    finally:
        for eng in engines or ():
            eng.close()
    results = []
    for g in range(n):
        if trace is not None:
            trace.append(boards[g]._pos.copy())
        results.append(0 if not boards[g].get_result() else (1 if last_side[g] == 0 else -1))
    return _score(results), results


def evaluate_two_models_batched(model, other_model, n_games: Optional[int] = None,
                                evaluate_with_mcts: bool = False, deterministic: bool = True,
                                seed: int = 0, trace: Optional[list] = None,
                                evaluate_with_solver: bool = False, solver_scores: Optional[list] = None):
    """All games at once.  Returns (score of `model`, per-game results);
    `trace` collects the final boards' arrays (chess: az_chess_pos records) in game order.
    evaluate_with_solver: `solver_scores` collects the sequential loop's solver
    score of every scored move of `model`, in game order then ply order; the
    positions are gathered while the games run and solved in one solver call."""
    n = int(n_games or ConfigServing.evaluation_games_number)
    if evaluate_with_solver:
        _check_solver(evaluate_with_mcts)
        solver_report.update(scored=0, unsolved=0)
    scored_moves = [[] for _ in range(n)]  # per game: (board before the move, the move) of `model`
    if _game()[2]:
        return _chess_arena_batched(model, other_model, n, evaluate_with_mcts, deterministic, seed, trace)
    all_moves = get_all_possible_moves()
    A = len(all_moves)
    boards = [Board() for _ in range(n)]
    side = np.array([g % 2 for g in range(n)])  # 0: `model` to move, 1: `other_model`
    rngs = [np.random.RandomState((seed + g) % 2 ** 32) for g in range(n)]
    models = (model, other_model)
    engines = [_arena_engine(m, n) for m in models] if evaluate_with_mcts else None
    active = [set(), set()]
    last_side = np.zeros(n, np.int64)
    while True:
        live = [g for g in range(n) if not boards[g].is_game_over()]
        if not live:
            break
        ply = boards[live[0]].fullmove_number  # lockstep: every live game is at the same ply
        for s in (0, 1):
            idx = [g for g in live if side[g] == s]
            if not idx:
                continue
            if not evaluate_with_mcts:
                x = np.stack([boards[g].full_state for g in idx])
                probs = models[s](x)[0].numpy()
                for k, g in enumerate(idx):
                    legal = normalize_probabilities(probs[k][boards[g].legal_moves_mask(all_moves)])
                    if deterministic:
                        move = boards[g].moves[int(np.argmax(legal))]
                    else:
                        move = rngs[g].choice(boards[g].moves, 1, p=legal).item()
                    if evaluate_with_solver and s == 0:
                        scored_moves[g].append((deepcopy(boards[g]), move))
                    boards[g].play(move, keep_same_player=True)
            else:
                eng = engines[s]
                stale = sorted(active[s] - set(idx))
                if stale:
                    eng.tree_release(stale)
                eng.tree_reset(idx, np.stack([boards[g].array for g in idx]))
                active[s] = set(idx)
                sims = ConfigSelfPlay.mcts_iterations
                if ConfigMCTS.enable_dirichlet_noise:
                    # each move's MCTS starts on an unexpanded root (evaluate.py:64-83):
                    # sims - 1 root selections draw from the game's stream, before play's draw
                    rows = max(sims - 1, 0)
                    noise = np.zeros((n, max(rows, 1), A))
                    for g in idx:
                        noise[g] = root_noise_rows(rngs[g], len(boards[g].moves), rows, A)
                    eng.tree_search(sims, noise=noise)
                else:
                    eng.tree_search(sims)
                u = None
                if not deterministic:
                    u = np.zeros(n)
                    for g in idx:
                        u[g] = rngs[g].random_sample()  # np.random.choice's one draw (mcts.py:201)
                greedy = ply > ConfigMCTS.index_move_greedy
                moves, _status, _policy = eng.tree_play(u, greedy=greedy, deterministic=deterministic)
                for g in idx:
                    boards[g].play(all_moves[int(moves[g])], keep_same_player=True)
            last_side[idx] = s
        side = 1 - side
    results = []
    for g in range(n):
        if trace is not None:
            trace.append(boards[g].array.copy())
        r = boards[g].get_result(keep_same_player=True)
        results.append(0 if not r else (1 if last_side[g] == 0 else -1))
    _ = A
    if evaluate_with_solver:
        pairs = [p for game in scored_moves for p in game]
        ranked = exact.exact_ranked_moves_and_value_batch([b for b, _ in pairs])
        for (board, move), r in zip(pairs, ranked):
            if r is None:
                solver_report["unsolved"] += 1
                continue
            solver_report["scored"] += 1
            if solver_scores is not None:
                solver_scores.append(_solver_move_score(r[0], board, move))
    return _score(results), results
