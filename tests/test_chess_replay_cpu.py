"""CPU checks of the chess replay window's host side (engine.ChessReplay):
no CPU fallback, and the pure preparation of self-play results into the
records ChessReplay.push takes (engine.chess_replay_records)."""
import numpy as np
import pytest

from custom_alphazero import engine as az
from custom_alphazero.chess import kernels as K


def test_replay_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(az.AzError, match="no HIP device"):
        az.ChessReplay(4)


def _results():
    """Three hand-made games of max_plies 5: decisive in 3 plies, empty, drawn in 4 plies"""
    G, P, M = 3, 5, K.MAX_MOVES
    rng = np.random.RandomState(0)
    r = dict(lengths=np.array([3, 0, 4], np.int32), results=np.array([1, 0, 0], np.int32),
             positions=np.zeros((G, P), K.POS_DTYPE), policy_n=rng.randint(1, 30, size=(G, P)).astype(np.int32),
             policy_actions=rng.randint(0, K.ACTIONS, size=(G, P, M)).astype(np.int16),
             policy_probs=rng.rand(G, P, M))
    r["positions"]["fullmove_number"] = 100 * (np.arange(G)[:, None] + 1) + np.arange(P)  # names every ply
    r["positions"]["occupied_co"] = rng.randint(1, 2 ** 62, size=(G, P, 2)).astype(np.uint64)
    return r


def test_records_follow_play_chess():
    from custom_alphazero.self_play import alternating_rewards
    r = _results()
    start = np.zeros((), K.POS_DTYPE)
    start["fullmove_number"], start["turn"] = 1, 1
    rec = az.chess_replay_records(r, start)
    assert tuple(rec) == az.ChessReplay.KEYS
    plies = [(0, 0), (0, 1), (0, 2), (2, 0), (2, 1), (2, 2), (2, 3)]  # game order; the empty game gives nothing
    n = len(plies)
    assert rec["hist"].shape == (n, 8) and rec["hist"].dtype == K.POS_DTYPE
    assert rec["valid"].shape == (n, 8) and rec["valid"].dtype == np.uint8
    assert rec["policy_n"].shape == (n,) and rec["policy_n"].dtype == np.int32
    assert rec["policy_actions"].shape == (n, 256) and rec["policy_actions"].dtype == np.int16
    assert rec["policy_probs"].shape == (n, 256) and rec["policy_probs"].dtype == np.float64
    assert rec["z"].shape == (n,) and rec["z"].dtype == np.float32
    zero = np.zeros((), K.POS_DTYPE)
    for i, (g, t) in enumerate(plies):
        # [0 x 7, pos] for a game's first ply, [0 x 6, start, pos] afterwards
        want_valid = [0] * 7 + [1] if t == 0 else [0] * 6 + [1, 1]
        assert rec["valid"][i].tolist() == want_valid
        assert rec["hist"][i, 7] == r["positions"][g, t]
        assert all(rec["hist"][i, h] == zero for h in range(6))
        assert rec["hist"][i, 6] == (zero if t == 0 else start)
        assert rec["policy_n"][i] == r["policy_n"][g, t]
        assert np.array_equal(rec["policy_actions"][i], r["policy_actions"][g, t])
        assert np.array_equal(rec["policy_probs"][i], r["policy_probs"][g, t])
    # decisive: the last mover won, signs alternate going back; drawn: zeros
    assert np.array_equal(rec["z"][:3], alternating_rewards(1, 3).astype(np.float32))
    assert rec["z"][:3].tolist() == [1.0, -1.0, 1.0]
    assert np.array_equal(rec["z"][3:], alternating_rewards(0, 4).astype(np.float32))
    assert rec["z"][3:].tolist() == [0.0] * 4


def test_records_honour_the_discounting_factor(monkeypatch):
    from custom_alphazero.config import ConfigSelfPlay
    from custom_alphazero.self_play import alternating_rewards
    monkeypatch.setattr(ConfigSelfPlay, "discounting_factor", 0.9)
    rec = az.chess_replay_records(_results(), np.zeros((), K.POS_DTYPE))
    want = alternating_rewards(1, 3)
    assert want.dtype == np.float64 and np.array_equal(rec["z"][:3], want.astype(np.float32))
    assert rec["z"][0] == np.float32(0.81)


def test_no_games_give_empty_records():
    r = _results()
    r["lengths"][:] = 0
    rec = az.chess_replay_records(r, np.zeros((), K.POS_DTYPE))
    assert [len(rec[k]) for k in az.ChessReplay.KEYS] == [0] * 6
    assert rec["hist"].shape == (0, 8) and rec["policy_probs"].shape == (0, 256)


def test_the_default_start_is_the_start_position():
    from custom_alphazero.chess.board import Board
    r = _results()
    rec = az.chess_replay_records(r)
    assert rec["hist"][1, 6] == Board()._pos and rec["hist"][1, 6]["fullmove_number"] == 1
