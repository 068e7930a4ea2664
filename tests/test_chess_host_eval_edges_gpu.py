"""The chess search on any evaluator output, through the host-evaluator seam
(az_chess_engine_set_evaluator): negative, cancelling, subnormal, huge,
infinite and NaN outputs, searched as the reference searches them -- numpy's
arithmetic, and np.argmax's order for the best edge, the first NaN first
(mcts.py:64-68).  One NaN among a node's legal probabilities makes every prior
and every UCB of that node NaN; the reference then takes edge 0, and so must
the wave descent, whose index stays below the node's count on any input.

The evaluators are tests/select_cases.py's ChessEval, the same function on
both sides: the chess oracle calls it with (pos, initial), the engine's
callable looks its rows up by the bytes of the planes.  The oracle's best edge
is orc_argmax_f64, pinned to numpy by tests/test_select_order_cpu.py, which
also shows these games part from the earlier loop's on the non-finite kinds.
"""
import pytest

import select_cases as S
from test_chess_selfplay_gpu import _compare

pytestmark = pytest.mark.gpu

_ORACLE = {}
# Once an edge's W is NaN its UCB is, and every later simulation through its node takes it: the
# subtree a move keeps then holds nearly all of the game's expansions (8 a ply, 10 plies, up to a
# few dozen edges each), more than the default arena of a search that spreads its visits.
ARENA_EDGES = 8192


def _oracle_games(kind):
    """(evaluator, the oracle's games under it), once per kind"""
    if kind not in _ORACLE:
        ev = S.ChessEval(kind)
        _ORACLE[kind] = ev, S.chess_games(ev)
    return _ORACLE[kind]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("cache_log2", [0, 10])
@pytest.mark.parametrize("kind", S.NONFINITE[::-1] + S.FINITE)
def test_host_selfplay_matches_oracle(kind, cache_log2, lanes):
    from custom_alphazero import engine as az
    ev, want = _oracle_games(kind)
    eng = az.ChessEngine(evaluator=az.EVAL_HOST, mcts_iterations=S.CHESS_SIMS, slots=S.CHESS_GAMES,
                         max_plies=S.CHESS_PLIES, lanes=lanes, cache_log2=cache_log2, arena_edges=ARENA_EDGES)
    try:
        eng.set_host_evaluator(ev.model)
        st = eng.selfplay_run(0, S.CHESS_GAMES, S.CHESS_SEED)
        r = eng.selfplay_results()
        assert st["errors"] == 0 and st["games_done"] == S.CHESS_GAMES
        for g in range(S.CHESS_GAMES):
            _compare(r, g, want[g], (kind, lanes, cache_log2))
    finally:
        eng.close()

