"""The chess engine's host-evaluator seam (AZ_EVAL_HOST in az_chess_config,
az_chess_engine_set_evaluator, ChessEngine.set_host_evaluator): any callable
model(x) -> (probabilities, value) on the (n, 8, 8, 118) Board.full_state
planes searches chess, as the reference's MCTS calls self.model on whatever
it was given (mcts/mcts.py:130-137).

The model here is a pure function of the bytes of each x[i], so the same
function handed to the chess oracle through its (pos, initial) callback --
which encodes the reference's history form itself -- pins every path bit for
bit: all 118 planes, the root's [0 x 7, start] history against the later
boards' [0 x 6, start, board], the lanes' serialisation over one staging
buffer, and the transposition cache's transparency."""
import zlib

import numpy as np
import pytest

import chess_oracle as C
from test_chess_selfplay_gpu import _compare

pytestmark = pytest.mark.gpu


def _plane_row(xi):
    """(probs f32 [1880], value in [-1, 1)) from the bytes of one (8, 8, 118) f32 state; all-zero
    probabilities for one hash residue (normalize_probabilities' zero-sum -> uniform float64 branch)."""
    h = zlib.crc32(np.ascontiguousarray(xi, np.float32).tobytes())
    rng = np.random.RandomState(h)
    p = rng.random_sample(1880).astype(np.float32)
    v = np.float32(rng.random_sample() * 2.0 - 1.0)
    if h % 16 == 0:
        p[:] = 0.0
    return p, v


class PlaneModel:
    """model(x) -> (probs (n, 1880), values (n,)); records every call's batch size."""

    def __init__(self):
        self.calls = []

    def __call__(self, x):
        assert x.dtype == np.float32 and x.shape[1:] == (8, 8, 118) and x.flags["C_CONTIGUOUS"]
        self.calls.append(len(x))
        rows = [_plane_row(xi) for xi in x]
        return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32)


def _oracle_cb(pos, initial):
    x = C.full_state(*C.reference_history(pos, bool(initial)), pos)[None].astype(np.float32)
    p, v = _plane_row(x[0])
    return p, float(v)


def _host_engine(model=None, **kw):
    from custom_alphazero import engine as az
    eng = az.ChessEngine(evaluator=az.EVAL_HOST, **kw)
    if model is not None:
        eng.set_host_evaluator(model)
    return eng


@pytest.fixture(scope="module")
def oracle_games():
    """The oracle's three games under the plane model (computed once; every lanes / cache case
    compares against them)."""
    return [C.play_game(16, 900 + g, 12, callback=_oracle_cb) for g in range(3)]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("cache_log2", [0, 10])
def test_host_selfplay_matches_oracle(oracle_games, lanes, cache_log2):
    model = PlaneModel()
    games, slots = 3, 6
    eng = _host_engine(model, mcts_iterations=16, slots=slots, max_plies=12, lanes=lanes, cache_log2=cache_log2)
    st = eng.selfplay_run(0, games, 900)
    r = eng.selfplay_results()
    assert st["errors"] == 0 and st["games_done"] == games
    for g in range(games):
        _compare(r, g, oracle_games[g], ("host", lanes, cache_log2))
    # the batches: a lane's leaves at once, never more than its slots, and not one call per expansion
    lane_slots = slots // lanes
    assert model.calls and min(model.calls) >= 1 and max(model.calls) <= lane_slots
    assert len(model.calls) < int(r["expansions"].sum())
    # the first simulation's leaves are the live games' roots, all the start position: with the cache
    # they share one row; without it every live game of the first lane has its own (the first lane's
    # slots are all live whenever the games fill it: min(games, lane_slots) of them)
    assert model.calls[0] == (1 if cache_log2 else min(games, lane_slots))
    eng.close()


def test_host_tree_api_matches_oracle():
    pos, _ = C.random_positions(40, seed=5)
    roots = [C.from_fen(), pos[7], pos[23]]
    model = PlaneModel()
    eng = _host_engine(model, mcts_iterations=8, slots=3, max_plies=64, arena_edges=20_000)
    eng.tree_reset(np.arange(3), np.array(roots, C.POS_DTYPE))
    trees = [C.Tree(r, callback=_oracle_cb) for r in roots]

    def check(tag):
        for s, tr in enumerate(trees):
            t, want = eng.tree_export(s), tr.root()
            sl = slice(t["root_first"], t["root_first"] + t["root_n"])
            assert t["root_n"] == len(want["moves"]), (tag, s)
            np.testing.assert_array_equal(t["moves"][sl], want["moves"].astype(np.int32))
            np.testing.assert_array_equal(t["prior"][sl].view(np.uint64), want["prior"].view(np.uint64))
            np.testing.assert_array_equal(t["n"][sl], want["n"])
            np.testing.assert_array_equal(t["w"][sl].view(np.uint64), want["w"].view(np.uint64))

    eng.tree_search(8)
    for tr in trees:
        tr.search(8)
    check("first search")
    u = np.array([0.3, 0.6, 0.9])
    out = eng.tree_play(u)
    for s, tr in enumerate(trees):
        mv, oc, pa, pp = tr.play(u[s])
        assert out["moves"][s] == mv and out["status"][s] == oc
        k = int(out["policy_n"][s])
        np.testing.assert_array_equal(out["policy_actions"][s, :k], pa)
        np.testing.assert_array_equal(out["policy_probs"][s, :k].view(np.uint64), pp.view(np.uint64))
    eng.tree_search(8)
    for tr in trees:
        tr.search(8)
    check("second search")
    assert max(model.calls) <= 3
    eng.close()


def test_mcts_accepts_a_callable_chess_model(monkeypatch):
    from custom_alphazero.chess.board import Board as ChessBoard
    from custom_alphazero.chess.utils import get_all_possible_moves
    from custom_alphazero.config import ConfigSelfPlay
    from custom_alphazero.mcts.mcts import MCTS
    monkeypatch.setattr(ConfigSelfPlay, "mcts_iterations", 12)
    model = PlaneModel()
    mcts = MCTS(ChessBoard(), get_all_possible_moves(), model=model)
    tree = C.Tree(C.from_fen(), callback=_oracle_cb)
    np.random.seed(41)
    ref_rng = np.random.RandomState(41)
    for _ply in range(3):
        mcts.search(12)
        tree.search(12)
        _parent, _child, policy, move = mcts.play(return_details=True)
        mv, _oc, pa, pp = tree.play(ref_rng.random_sample())
        assert move.code == mv
        dense = np.zeros(1880)
        dense[pa] = pp
        np.testing.assert_array_equal(policy.view(np.uint64), dense.view(np.uint64))
    assert max(model.calls) == 1  # one tree: batch-1 calls


def test_self_play_takes_a_callable_chess_model(oracle_games, monkeypatch):
    """self_play.play_chess / play_game with ConfigGeneral.game == "chess" and a plain callable."""
    from custom_alphazero import self_play
    from custom_alphazero.chess.utils import get_all_possible_moves
    from custom_alphazero.config import ConfigGeneral, ConfigSelfPlay
    monkeypatch.setattr(ConfigGeneral, "game", "chess")
    monkeypatch.setattr(ConfigSelfPlay, "mcts_iterations", 16)
    monkeypatch.setattr(ConfigSelfPlay, "chess_max_plies", 12)
    monkeypatch.setattr(ConfigSelfPlay, "chess_concurrent_games", 6)
    model = PlaneModel()
    states, policies, rewards, records = self_play.play_chess(model, 3, 900)
    for g, ref in enumerate(oracle_games):
        assert records[g].length == ref["T"] and np.array_equal(records[g].moves, ref["moves"])
    total = sum(ref["T"] for ref in oracle_games)
    assert states.shape == (total, 8, 8, 118) and policies.shape == (total, 1880) and len(rewards) == total
    # another callable is another engine (the cache key holds the callable's identity)
    first = next(iter(self_play._CHESS_ENGINES.values()))
    assert first.host_model is model
    other = PlaneModel()
    s1, p1, _r1, rec = self_play.play_game(0, get_all_possible_moves(), 16, "run", model=other)
    assert 1 <= rec.length <= 12 and s1.shape == (rec.length, 8, 8, 118) and p1.shape == (rec.length, 1880)
    assert other.calls and next(iter(self_play._CHESS_ENGINES.values())).host_model is other


def test_network_as_the_callable_plays_the_network_engines_games():
    """A host engine whose callable is another engine's forward plays the network engine's games."""
    from custom_alphazero import engine as az
    from custom_alphazero.model.weights import init_weights, weight_spec
    w = init_weights(weight_spec(8, 8, 1880, depth=1, in_channels=118), seed=3, randomize_bn=True)
    kw = dict(mcts_iterations=16, slots=4, max_plies=12, depth=1)
    net = az.ChessEngine(evaluator=az.EVAL_NETWORK, **kw)
    net.set_weights(w.items())
    net.selfplay_run(0, 4, 31)
    want = net.selfplay_results()
    host = _host_engine(net.forward, **kw)
    st = host.selfplay_run(0, 4, 31)
    got = host.selfplay_results()
    assert st["errors"] == 0 and st["games_done"] == 4
    np.testing.assert_array_equal(got["lengths"], want["lengths"])
    np.testing.assert_array_equal(got["expansions"], want["expansions"])
    np.testing.assert_array_equal(got["moves"], want["moves"])
    np.testing.assert_array_equal(got["policy_n"], want["policy_n"])
    np.testing.assert_array_equal(got["policy_actions"], want["policy_actions"])
    np.testing.assert_array_equal(got["policy_probs"].view(np.uint64), want["policy_probs"].view(np.uint64))
    host.close()
    net.close()


def test_host_evaluator_errors():
    from custom_alphazero import engine as az
    start = np.array([C.from_fen()], C.POS_DTYPE)
    # no callable set
    eng = _host_engine(mcts_iterations=4, slots=1, max_plies=8)
    eng.tree_reset([0], start)
    with pytest.raises(az.AzError, match="set_evaluator"):
        eng.tree_search(2)
    # forward / set_weights belong to the network evaluator
    with pytest.raises(az.AzError):
        eng.forward(np.zeros((1, 8, 8, 118), np.float32))

    # a raising callable: its own exception, then AZ_E_STATE until a reset
    class Boom(Exception):
        pass

    state = {"fail": True}

    def flaky(x):
        if state["fail"]:
            raise Boom("model failure")
        return PlaneModel()(x)

    eng.set_host_evaluator(flaky)
    with pytest.raises(Boom):
        eng.tree_search(2)
    state["fail"] = False
    with pytest.raises(az.AzError, match="-3"):
        eng.tree_search(2)
    with pytest.raises(az.AzError, match="-3"):
        eng.tree_play(np.array([0.5]))
    eng.tree_reset([0], start)
    eng.tree_search(2)
    assert eng.tree_export(0)["root_n"] == 20

    # a wrong output shape
    eng.set_host_evaluator(lambda x: (np.zeros((len(x), 7), np.float32), np.zeros(len(x), np.float32)))
    eng.tree_reset([0], start)
    with pytest.raises(ValueError):
        eng.tree_search(1)
    eng.close()

    # the seam belongs to engines created with EVAL_HOST
    syn = az.ChessEngine(mcts_iterations=4, slots=1, evaluator=az.EVAL_SYNTHETIC, max_plies=8)
    with pytest.raises(az.AzError, match="AZ_EVAL_HOST"):
        syn.set_host_evaluator(PlaneModel())
    syn.close()
