"""Dirichlet root noise in the chess engine against tests/chess_noise_ref.py
(the plain-Python MCTS that tests/test_chess_noise_cpu.py pins to the chess
oracle with noise off): host-drawn rows through the tree API, device-drawn
noise in self-play (bit for bit numpy's legacy RandomState.dirichlet on each
game's MT19937 stream), the float32 / float64 prior forms of the mix, and the
Python surface."""
import functools

import numpy as np
import pytest

import chess_noise_ref as R
import chess_oracle as C
from test_chess_tree_gpu import ROOTS

pytestmark = pytest.mark.gpu

M = 256  # AZ_CHESS_MAX_MOVES


def _root_edges(eng, slot):
    t = eng.tree_export(slot)
    sl = slice(t["root_first"], t["root_first"] + t["root_n"])
    return {k: t[k][sl] for k in ("moves", "prior", "n", "w", "child_n")}


def _check_root(eng, slot, ref, tag):
    got, want = _root_edges(eng, slot), ref.root()
    assert got["moves"].tolist() == want["moves"].astype(np.int32).tolist(), tag
    assert got["prior"].view(np.uint64).tolist() == want["prior"].view(np.uint64).tolist(), tag
    assert got["n"].tolist() == want["n"].tolist(), tag
    assert got["w"].view(np.uint64).tolist() == want["w"].view(np.uint64).tolist(), tag
    assert got["child_n"].tolist() == want["child_n"].tolist(), tag


def _rows(rng, trees, sims, alpha):
    """[slots, sims, 256]: per slot `sims` np.random.dirichlet vectors over its root's moves."""
    out = np.zeros((len(trees), sims, M))
    for s, tr in enumerate(trees):
        k = len(C.legal_moves(tr.root_node.pos))
        for r in range(sims):
            if k:
                out[s, r, :k] = rng.dirichlet(np.ones(k) * alpha)
    return out


# ------------------------------------------------- 5. host-drawn, tree API
PLAN = [(40, False, False), (25, False, False), (1, False, False), (30, True, False), (20, False, True)]


@pytest.mark.parametrize("lanes", [1, 2])
def test_chess_tree_host_noise_matches_reference(lanes):
    from custom_alphazero import engine as az
    alpha, ratio = 0.3, 0.25
    roots = [C.from_fen(f) for f in ROOTS[:5]]
    eng = az.ChessEngine(mcts_iterations=64, slots=5, evaluator=az.EVAL_SYNTHETIC, max_plies=64, lanes=lanes,
                         arena_edges=50_000, dirichlet_noise=True, dirichlet_alpha=alpha, dirichlet_ratio=ratio)
    eng.tree_reset(np.arange(5), np.array(roots, C.POS_DTYPE))
    trees = [R.Tree(r, noise=(alpha, ratio)) for r in roots]
    rng = np.random.RandomState(40 + lanes)
    live = list(range(5))
    for step, (sims, greedy, det) in enumerate(PLAN):
        rows = _rows(rng, trees, sims, alpha)
        eng.tree_search(sims, noise=rows)
        for s in live:
            trees[s].search(sims, rows=rows[s])
            _check_root(eng, s, trees[s], ("search", step, s))
        u = rng.random_sample(5)
        out = eng.tree_play(u, greedy=greedy, deterministic=det)
        for s in list(live):
            mv, oc, pa, pp = trees[s].play(u[s], greedy, det)
            assert (out["moves"][s], out["status"][s]) == (mv, oc), (step, s)
            k = int(out["policy_n"][s])
            assert out["policy_actions"][s, :k].tolist() == pa.tolist()
            assert out["policy_probs"][s, :k].view(np.uint64).tolist() == pp.view(np.uint64).tolist()
            if oc == 0:
                _check_root(eng, s, trees[s], ("reuse", step, s))  # the reused subtree, prior form included
            else:
                eng.tree_release([s])
                live.remove(s)
    assert len(live) >= 3
    assert eng.stats()["expansions"] == sum(t.expansions for t in trees)
    eng.close()


def test_chess_tree_noise_refusals():
    from custom_alphazero import engine as az
    root = np.array([C.from_fen(ROOTS[1])], C.POS_DTYPE)
    noisy = az.ChessEngine(mcts_iterations=8, slots=1, evaluator=az.EVAL_SYNTHETIC, max_plies=8,
                           dirichlet_noise=True, dirichlet_alpha=0.3, dirichlet_ratio=0.25)
    plain = az.ChessEngine(mcts_iterations=8, slots=1, evaluator=az.EVAL_SYNTHETIC, max_plies=8)
    try:
        noisy.tree_reset([0], root)
        plain.tree_reset([0], root)
        with pytest.raises(az.AzError, match="az_chess_tree_search_noise"):
            noisy.tree_search(3)
        with pytest.raises(az.AzError, match="dirichlet_noise = 1"):
            plain.tree_search(3, noise=np.zeros((1, 3, M)))
        with pytest.raises(ValueError, match="noise must be"):
            noisy.tree_search(3, noise=np.zeros((1, 3, 7)))
        # the first simulation expands the root and takes no row; the next two take both; the fourth has none
        rows = _rows(np.random.RandomState(1), [R.Tree(root[0])], 2, 0.3)
        with pytest.raises(az.AzError, match="root-noise-rows-exhausted"):
            noisy.tree_search(4, noise=rows)
        with pytest.raises(az.AzError, match="Dirichlet noise needs 0 < dirichlet_alpha <= 1"):
            az.ChessEngine(mcts_iterations=8, slots=1, evaluator=az.EVAL_SYNTHETIC, dirichlet_noise=True,
                           dirichlet_alpha=1.5)
    finally:
        noisy.close()
        plain.close()


# ------------------------------------------------ 6. device-drawn, self-play
SP_GAMES, SP_SIMS, SP_PLIES, SP_SEED = 5, 24, 6, 9100


@functools.lru_cache(maxsize=None)
def _reference_games(alpha, ratio):
    return [R.play_game(SP_SIMS, SP_SEED + g, SP_PLIES, noise=(alpha, ratio)) for g in range(SP_GAMES)]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("alpha,ratio", [(0.03, 0.25), (0.3, 0.3), (1.0, 0.25)])
def test_chess_selfplay_device_noise_matches_reference(alpha, ratio, lanes):
    """5 games on 3 slots (a slot is refilled and reseeded).  A game draws
    24 * 6 vectors of 20-30 components, ~14 k MT19937 words: every game crosses
    the 624-word boundary some twenty times, with play's random_sample between
    the moves shifting the alignment."""
    from custom_alphazero import engine as az
    eng = az.ChessEngine(mcts_iterations=SP_SIMS, slots=3, evaluator=az.EVAL_SYNTHETIC, max_plies=SP_PLIES,
                         lanes=lanes, dirichlet_noise=True, dirichlet_alpha=alpha, dirichlet_ratio=ratio)
    st = eng.selfplay_run(0, SP_GAMES, SP_SEED)
    assert st["errors"] == 0 and st["games_done"] == SP_GAMES
    r = eng.selfplay_results()
    eng.close()
    for g, ref in enumerate(_reference_games(alpha, ratio)):
        T = int(r["lengths"][g])
        assert T == ref["T"], g
        assert r["moves"][g, :T].tolist() == ref["moves"].tolist(), g
        assert r["positions"][g, :T].tobytes() == ref["positions"].tobytes(), g
        assert (int(r["results"][g]), int(r["terminations"][g]), int(r["expansions"][g])) == \
            (ref["result"], ref["termination"], ref["expansions"]), g
        for t in range(T):
            k = int(r["policy_n"][g, t])
            assert k == int(ref["policy_n"][t])
            assert r["policy_actions"][g, t, :k].tolist() == ref["policy_actions"][t].tolist(), (g, t)
            assert r["policy_probs"][g, t, :k].view(np.uint64).tolist() == \
                ref["policy_probs"][t].view(np.uint64).tolist(), (g, t)


# ------------------------------------------------------- 7. the prior's dtype
def _power_of_two_root():
    pos, _ = C.random_positions(600, 3)
    for p in pos:
        if len(C.legal_moves(p)) in (16, 32) and C.outcome(p) == 0:
            return p
    raise AssertionError("no root with a power-of-two move count among the scanned positions")


def test_chess_noise_mix_uses_the_priors_dtype():
    """A root with 2^m legal moves: 1/n is the same number as a float32 (equal
    positive outputs, normalize_probabilities' quotient) and as a float64 (all
    zero outputs, its uniform branch), but (1 - 0.3) * priors is not: float32
    rounds 0.7 and keeps the product 7.45e-10 lower, for every edge alike.  That
    uniform shift weighs less on a visited edge (c * prior * sqrt(sum) / (1 + N)).
    The evaluator's value -0.125 makes the visited edge 0 worth q = 0.125, and
    the row of the third simulation (sum = 1: edge 0 visited once, the others
    never) puts edge 1 halfway between the two forms' tie points with edge 0:
    the float64 mix selects edge 1, the float32 mix edge 0 again."""
    from custom_alphazero import engine as az
    ratio, alpha, c, sims = 0.3, 0.3, 1.5, 12
    root = _power_of_two_root()
    k = len(C.legal_moves(root))
    rng = np.random.RandomState(5)
    rows = np.zeros((1, sims, M))
    for r in range(sims):
        rows[0, r, :k] = rng.dirichlet(np.ones(k) * alpha)
    kept64 = (1 - ratio) * (1.0 / k)
    kept32 = float(np.float32(1 - ratio) * np.float32(1.0 / k))
    assert kept64 != kept32
    d0 = 0.01

    def tie(kept):  # d1 with 0.125 + c (kept + ratio d0) / 2 == c (kept + ratio d1)
        return ((0.125 + c * (kept + ratio * d0) / 2) / c - kept) / ratio

    rows[0, 1, :k] = 0.001
    rows[0, 1, 0] = d0
    rows[0, 1, 1] = (tie(kept64) + tie(kept32)) / 2

    results = []
    for p in (0.0, 1.0 / 64):
        def fn(x, p=p):
            return np.full((len(x), 1880), p, np.float32), np.full(len(x), -0.125, np.float32)

        eng = az.ChessEngine(mcts_iterations=sims, slots=1, evaluator=az.EVAL_HOST, max_plies=8,
                             dirichlet_noise=True, dirichlet_alpha=alpha, dirichlet_ratio=ratio)
        eng.set_host_evaluator(fn)
        eng.tree_reset([0], np.array([root], C.POS_DTYPE))
        eng.tree_search(sims, noise=rows)
        ref = R.Tree(root, callback=lambda pos, initial, p=p: (np.full(1880, p, np.float32), -0.125),
                     noise=(alpha, ratio))
        ref.search(sims, rows=rows[0])
        assert ref.rows_used == sims - 1
        _check_root(eng, 0, ref, p)
        eng.close()
        results.append(ref.root())
    zero, equal = results
    assert zero["prior"].view(np.uint64).tolist() == equal["prior"].view(np.uint64).tolist()  # the same numbers ...
    assert zero["n"].tolist() != equal["n"].tolist()  # ... whose dtype decided a selection


# ---------------------------------------------------------- 8. Python surface
def test_chess_self_play_with_noise_matches_reference():
    from custom_alphazero import self_play
    from custom_alphazero.chess.board import Board
    from custom_alphazero.chess.utils import get_all_possible_moves
    from custom_alphazero.config import ConfigGeneral, ConfigMCTS, ConfigSelfPlay
    from custom_alphazero.mcts.mcts import MCTS, SyntheticEvaluator
    saved = (ConfigGeneral.game, ConfigMCTS.enable_dirichlet_noise, ConfigMCTS.dirichlet_noise_value,
             ConfigMCTS.dirichlet_noise_ratio, ConfigSelfPlay.chess_max_plies)
    try:
        ConfigGeneral.game = "chess"
        ConfigMCTS.enable_dirichlet_noise = True
        ConfigMCTS.dirichlet_noise_value = 0.3
        ConfigMCTS.dirichlet_noise_ratio = 0.25
        ConfigSelfPlay.chess_max_plies = 4
        states, policies, rewards, records = self_play.play("unused", model=SyntheticEvaluator(), n_games=2,
                                                            base_seed=321, sims=16)
        row = 0
        for g, rec in enumerate(records):
            ref = R.play_game(16, 321 + g, 4, greedy_ply=ConfigMCTS.index_move_greedy,
                              c_puct=ConfigMCTS.exploration_constant, noise=(0.3, 0.25))
            assert (rec.length, rec.result, rec.expansions) == (ref["T"], ref["result"], ref["expansions"])
            assert rec.moves.tolist() == ref["moves"].tolist()
            for t in range(ref["T"]):
                dense = np.zeros(1880)
                dense[ref["policy_actions"][t].astype(np.int64)] = ref["policy_probs"][t]
                assert policies[row].view(np.uint64).tolist() == dense.view(np.uint64).tolist(), (g, t)
                row += 1
        assert row == len(policies) == len(states) == len(rewards)
        # the object API on a chess board is not wired to the noisy search: still refused
        m = MCTS(board=Board(), all_possible_moves=get_all_possible_moves(), model=SyntheticEvaluator())
        with pytest.raises(NotImplementedError):
            m.search(4)
    finally:
        (ConfigGeneral.game, ConfigMCTS.enable_dirichlet_noise, ConfigMCTS.dirichlet_noise_value,
         ConfigMCTS.dirichlet_noise_ratio, ConfigSelfPlay.chess_max_plies) = saved
        for e in self_play._CHESS_ENGINES.values():
            e.close()
        self_play._CHESS_ENGINES.clear()
