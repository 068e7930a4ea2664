"""Host-side choices of the chess evaluator seam and the arena's game
dispatch: what is decided before any device work."""
import pytest

from custom_alphazero import engine as az
from custom_alphazero.config import ConfigGeneral
from custom_alphazero.evaluation import evaluate
from custom_alphazero.mcts import mcts


@pytest.mark.parametrize("model", [None, object()])
def test_chess_engine_for_refuses_what_it_cannot_call(model, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(az, "ChessEngine", no_engine)
    with pytest.raises(TypeError, match="callable"):
        mcts._chess_engine_for(model)


def test_chess_engine_for_takes_a_callable_to_the_host_seam(monkeypatch):
    made = {}

    class FakeEngine:
        def __init__(self, **kw):
            made.update(kw)

        def set_host_evaluator(self, fn):
            made["fn"] = fn

    monkeypatch.setattr(az, "ChessEngine", FakeEngine)

    def model(x):
        raise AssertionError("not called here")

    eng = mcts._chess_engine_for(model)
    assert isinstance(eng, FakeEngine) and made["evaluator"] == az.EVAL_HOST and made["fn"] is model
    assert made["slots"] == 1


def test_self_play_picks_the_same_three_evaluators():
    from custom_alphazero import self_play

    class Net:
        def engine_weights(self):
            return []

        def __call__(self, x):
            return None

    assert self_play._chess_evaluator(mcts.SyntheticEvaluator()) == az.EVAL_SYNTHETIC
    assert self_play._chess_evaluator(Net()) == az.EVAL_NETWORK
    assert self_play._chess_evaluator(lambda x: None) == az.EVAL_HOST
    for bad in (None, object()):
        with pytest.raises(TypeError):
            self_play._chess_evaluator(bad)


def test_arena_resolves_the_game_at_call_time(monkeypatch):
    from custom_alphazero.chess.board import Board as ChessBoard
    from custom_alphazero.connect_n.board import Board
    board, moves, is_chess = evaluate._game()
    assert board is Board and not is_chess and moves is evaluate.get_all_possible_moves
    monkeypatch.setattr(ConfigGeneral, "game", "chess")
    board, moves, is_chess = evaluate._game()
    assert board is ChessBoard and is_chess and moves.__module__ == "custom_alphazero.chess.utils"
    monkeypatch.setattr(ConfigGeneral, "game", "go")
    with pytest.raises(NotImplementedError):
        evaluate._game()


def test_chess_binding_declares_the_evaluator_setter():
    assert "az_chess_engine_set_evaluator" in az.EXPORTED
    assert hasattr(az.ChessEngine, "set_host_evaluator")
