"""The chess arena (reference evaluation/evaluate.py:16-134 with
ConfigGeneral.game == "chess"): two chess models play each other, one game at
a time as the reference does and all games at once on the device
(az_chess_tree_*); the batched form reproduces the sequential loop game by
game.  A short ply cap keeps the sequential form's one engine per MCTS cheap."""
import zlib

import numpy as np
import pytest

from custom_alphazero.config import (ConfigChess, ConfigGeneral, ConfigModel, ConfigSelfPlay,
                                     ConfigServing)
from custom_alphazero.evaluation import evaluate

pytestmark = pytest.mark.gpu


@pytest.fixture
def chess_config(monkeypatch):
    monkeypatch.setattr(ConfigGeneral, "game", "chess")
    monkeypatch.setattr(ConfigSelfPlay, "mcts_iterations", 8)
    monkeypatch.setattr(ConfigSelfPlay, "chess_max_plies", 6)
    monkeypatch.setattr(ConfigModel, "depth", 1)


@pytest.fixture
def two_models(chess_config):
    from custom_alphazero.model.tensorflow.model import PolicyValueModel
    a = PolicyValueModel(input_dim=(8, 8, 118), action_space=1880, seed=1)
    b = PolicyValueModel(input_dim=(8, 8, 118), action_space=1880, seed=2)
    return a, b


def plane_model(x):
    """A callable that is not a PolicyValueModel: probabilities and value from the bytes of each state."""
    probs, values = [], []
    for xi in np.asarray(x, np.float32):
        rng = np.random.RandomState(zlib.crc32(np.ascontiguousarray(xi).tobytes()))
        probs.append(rng.random_sample(1880).astype(np.float32))
        values.append(np.float32(rng.random_sample() * 2.0 - 1.0))
    return np.stack(probs), np.array(values, np.float32)


@pytest.mark.parametrize("with_mcts", [False, True])
@pytest.mark.parametrize("deterministic", [True, False])
def test_batched_chess_arena_matches_sequential(two_models, with_mcts, deterministic):
    from custom_alphazero.chess.utils import get_all_possible_moves
    a, b = two_models
    n = 2
    tb, ts = [], []
    _, batched = evaluate.evaluate_two_models_batched(a, b, n_games=n, evaluate_with_mcts=with_mcts,
                                                      deterministic=deterministic, seed=7, trace=tb)
    moves = get_all_possible_moves()
    seq = [evaluate._single_game_evaluation(a, b, g, moves, with_mcts, False, deterministic,
                                            rng=np.random.RandomState(7 + g), trace=ts)[0]
           for g in range(n)]
    assert batched == seq
    assert len(tb) == len(ts) == n
    for x, y in zip(tb, ts):  # the same final positions, field for field
        assert x.tobytes() == y.tobytes()
    assert set(batched) <= {-1, 0, 1}
    start = evaluate._game()[0]()._pos
    assert all(x.tobytes() != start.tobytes() for x in tb)  # the games were played


def test_callable_against_a_network_in_the_batched_mcts_arena(two_models):
    a, _ = two_models
    runs = []
    for _ in range(2):
        trace = []
        score, results = evaluate.evaluate_two_models_batched(plane_model, a, n_games=2, evaluate_with_mcts=True,
                                                              deterministic=False, seed=3, trace=trace)
        assert 0.0 <= score <= 1.0 and set(results) <= {-1, 0, 1}
        runs.append((results, [t.tobytes() for t in trace]))
    assert runs[0] == runs[1]


MATE_IN_ONE = "6k1/5ppp/8/8/8/8/5PPP/R5K1"  # Ra8#


def _mating_model(x):
    from custom_alphazero.chess.move import Move
    from custom_alphazero.chess.utils import get_all_possible_moves
    probs = np.zeros((len(x), 1880), np.float32)
    probs[:, get_all_possible_moves().index(Move(uci="a1a8"))] = 1.0
    return probs, np.zeros(len(x), np.float32)


@pytest.mark.parametrize("with_mcts", [False, True])
def test_a_mate_is_credited_to_the_last_mover(chess_config, monkeypatch, with_mcts):
    """From a mate-in-one start position the model to move mates: game 0 is `model`'s (score 1.0),
    game 1 the other model's (-1: score 0.0), in both forms of the arena."""
    from custom_alphazero.chess.utils import get_all_possible_moves
    monkeypatch.setattr(ConfigChess, "initial_board_fen", MATE_IN_ONE)
    monkeypatch.setattr(ConfigChess, "initial_castling_rights", "-")

    def other(x):
        return _mating_model(x)

    trace = []
    score, results = evaluate.evaluate_two_models_batched(_mating_model, other, n_games=2,
                                                          evaluate_with_mcts=with_mcts, deterministic=True,
                                                          trace=trace)
    assert results == [1, -1] and score == 0.5
    moves = get_all_possible_moves()
    seq = [evaluate._single_game_evaluation(_mating_model, other, g, moves, with_mcts, False, True)[0]
           for g in range(2)]
    assert seq == [1, -1]
    assert evaluate._score(seq[:1]) == 1.0 and evaluate._score(seq[1:]) == 0.0
    monkeypatch.setattr(ConfigServing, "evaluation_games_number", 1)
    assert evaluate.evaluate_two_models(_mating_model, other, evaluate_with_mcts=with_mcts,
                                        deterministic=True) == (1.0, None)


def test_chess_solver_scoring_is_still_refused(chess_config):
    with pytest.raises(NotImplementedError):
        evaluate.evaluate_two_models(plane_model, plane_model, evaluate_with_solver=True)
    with pytest.raises(NotImplementedError):
        evaluate._single_game_evaluation(plane_model, plane_model, 0, [], False, True, True)
