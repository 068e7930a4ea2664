"""The Connect-N search on any evaluator output, through the host-evaluator
seam (AZ_EVAL_HOST): a callable may return negative, cancelling, subnormal,
huge, infinite or NaN numbers, and the reference searches on them -- its
arithmetic as numpy does it, its best edge np.argmax over Python floats, the
first NaN first (mcts.py:64-68).

The evaluators are tests/select_cases.py's, on the smallest shape of each
descent (the L = 8 Connect-4 and generic groups, L = 16, 32, 64 and the serial
loop).  Self-play games are compared with oracle/refport.py's (np.argmax
itself), bit for bit; the noise cases and the tree API with the C oracle,
whose games tests/test_select_order_cpu.py pins to refport's.  The same file
shows every non-finite case live: np.argmax and the first-element-then-`>`
loop part ways in a compared game.
"""
import numpy as np
import pytest

import oracle
import select_cases as S
from custom_alphazero import engine as az
from test_engine_gpu import selfplay_games

pytestmark = pytest.mark.gpu

GAMES = len(S.SEEDS)


def _engine(shape, kind, **kw):
    H, W, n, gravity, sims = S.SHAPES[shape]
    eng = az.Engine(H, W, n, gravity, sims, slots=kw.pop("slots", GAMES), evaluator=az.EVAL_HOST, **kw)
    eng.set_host_evaluator(S.PlaneModel(kind, shape))
    return eng


def _selfplay(shape, kind, **kw):
    eng = _engine(shape, kind, **kw)
    try:
        games = selfplay_games(eng, 0, GAMES, base_seed=S.SEEDS[0])
        assert eng.stats()["errors"] == 0
    finally:
        eng.close()
    return games


def _check_port(shape, kind, games, tag=()):
    for seed, got in zip(S.SEEDS, games):
        ref = S.port_game(shape, kind, seed)
        assert got["T"] == ref["T"], (tag, seed, got["T"], ref["T"])
        np.testing.assert_array_equal(got["moves"], ref["moves"])
        np.testing.assert_array_equal(got["policy"].view(np.uint64), np.asarray(ref["policies"]).view(np.uint64))
        assert got["expansions"] == ref["expansions"], (tag, seed)


def _assert_bits_nan_equal(got, want):
    """bitwise, except that a NaN matches any NaN (the default NaN's sign and payload differ
    between x86 and gfx950)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


@pytest.mark.parametrize("shape,kind", S.GPU_CASES)
def test_selfplay_matches_refport(shape, kind):
    _check_port(shape, kind, _selfplay(shape, kind))
    if kind == "illegal_junk":  # what the reference masks out changes nothing
        assert all(S.same_game(S.port_game(shape, kind, s), S.port_game(shape, None, s)) for s in S.SEEDS)


VARIANT_CASES = [(shape, kind) for shape in ("c4_6x7", "nograv_4x4", "nograv_6x6", "nograv_5x13")
                 for kind in ("nan_value", "inf_prob", "nan_prob")]


@pytest.mark.parametrize("variant", [dict(cache_log2=10), dict(lanes=2), dict(compact=True)],
                         ids=["cache", "lanes2", "compact"])
@pytest.mark.parametrize("shape,kind", VARIANT_CASES)
def test_selfplay_variants_match_refport(shape, kind, variant):
    """the cache (NaN and inf payloads round-trip it: the games are those without it), two lanes,
    and the left subtrees reclaimed after every move"""
    _check_port(shape, kind, _selfplay(shape, kind, **variant), tag=tuple(variant))


NOISE_CASES = [(shape, kind) for shape in ("c4_6x7", "nograv_4x4", "nograv_5x5", "nograv_6x6", "nograv_5x13")
               for kind in ("cancel", "nan_value", "inf_prob", "nan_prob")]


@pytest.mark.parametrize("shape,kind", NOISE_CASES)
def test_selfplay_with_root_noise_matches_oracle(shape, kind):
    """get_best_edge_with_noise on the same outputs (cancel: the float64 uniform priors' mix),
    against the C oracle's noise path"""
    H, W, n, gravity, sims = S.SHAPES[shape]
    games = _selfplay(shape, kind, dirichlet_noise=True, dirichlet_alpha=0.03, dirichlet_ratio=0.25)
    for seed, got in zip(S.SEEDS, games):
        ref = oracle.play_game(H, W, n, gravity, sims, seed, evaluator="callback",
                               callback=S.BoardEval(kind, shape), noise=(0.03, 0.25))
        assert got["T"] == ref["T"], (seed, got["T"], ref["T"])
        np.testing.assert_array_equal(got["moves"], ref["moves"])
        np.testing.assert_array_equal(got["policy"].view(np.uint64), ref["policy"].view(np.uint64))
        assert got["expansions"] == ref["expansions"]


@pytest.mark.parametrize("shape,kind", [("c4_6x7", "nan_value"), ("grav_4x5", "inf_value"),
                                        ("nograv_4x4", "inf_prob"), ("nograv_5x5", "nan_prob"),
                                        ("nograv_6x6", "nan_value"), ("nograv_5x13", "inf_prob")])
def test_tree_api_edges_match_oracle(shape, kind):
    """MCTS.search / play through the tree API, a whole game: after every search the root's edges
    hold the oracle's N exactly, and its W and priors bit for bit with NaN matching NaN"""
    H, W, n, gravity, sims = S.SHAPES[shape]
    seed = S.SEEDS[0]
    ref = oracle.play_game(H, W, n, gravity, sims, seed, evaluator="callback", callback=S.BoardEval(kind, shape))
    eng = _engine(shape, kind, slots=1)
    try:
        eng.tree_reset([0], np.zeros((1, H, W), np.int8))
        rng = np.random.RandomState(seed)
        rng.rand(1, H, W, 4)  # play_game's model construction
        saw_nan = False
        for ply in range(ref["T"]):
            eng.tree_search(sims)
            t = eng.tree_export(0)
            k, f = t["root_n"], t["root_first"]
            assert k == ref["n_edges"][ply]
            np.testing.assert_array_equal(t["action"][f:f + k], ref["edge_action"][ply, :k])
            np.testing.assert_array_equal(t["n"][f:f + k], ref["edge_n"][ply, :k])
            _assert_bits_nan_equal(t["w"][f:f + k], ref["edge_w"][ply, :k])
            _assert_bits_nan_equal(t["prior"][f:f + k], ref["edge_prior"][ply, :k])
            saw_nan |= bool(np.isnan(t["w"][f:f + k]).any() or np.isnan(t["prior"][f:f + k]).any())
            moves, status, policy = eng.tree_play([rng.random_sample()], greedy=ply >= 8)
            assert moves[0] == ref["moves"][ply]
            np.testing.assert_array_equal(policy[0].view(np.uint64), ref["policy"][ply].view(np.uint64))
            assert (status[0] != 0) == (ply == ref["T"] - 1)
        assert saw_nan  # the oddity reached a root's statistics
    finally:
        eng.close()
