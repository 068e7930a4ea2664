"""The group descent (select_group_kernel) at every group width, against the
C oracle game by game and bitwise.

The rest of the suite reaches groups of 8, 16 and 32 lanes and the serial
kernel; here every width runs, 64 included (partly filled and a full wave),
with fewer children than lanes and with as many, on 3 and on 11 slots: both
refill, and a launch's last wave holds fewer groups than fit (3 groups of 8,
16 or 32) or the launch spans several waves (11 groups of 8 fill one wave and
part of the next; 11 groups of 64 are 11 waves in 6 blocks).  The group's
reductions (visit sum, first-maximum UCB in np.argmax's order with root noise)
and the winner's broadcast decide every move, so any lane pairing that went
wrong shows as a different game."""
import functools

import numpy as np
import pytest

import oracle
from custom_alphazero import engine as az

pytestmark = pytest.mark.gpu

GAMES = 8
SEED = 31
NOISE = (0.03, 0.25)

# (H, W, n, gravity, sims): action space -> group width
SHAPES = [
    pytest.param((4, 5, 3, True, 40), id="4x5-A5-L8-short-group"),
    pytest.param((6, 7, 4, True, 40), id="6x7-A7-L8-c64"),
    pytest.param((4, 4, 3, False, 30), id="4x4-A16-L16-full"),
    pytest.param((9, 9, 5, True, 40), id="9x9-A9-L16"),
    pytest.param((5, 5, 4, False, 30), id="5x5-A25-L32"),
    pytest.param((6, 6, 4, False, 30), id="6x6-A36-L64-part"),
    pytest.param((8, 8, 4, False, 30), id="8x8-A64-L64-full"),
]


@functools.lru_cache(maxsize=None)
def reference(shape, noise):
    """The oracle's games for a shape, computed once and shared by the cases."""
    H, W, n, grav, S = shape
    return tuple(oracle.play_game(H, W, n, grav, S, SEED + g, noise=NOISE if noise else None)
                 for g in range(GAMES))


def selfplay_games(eng, n_games, base_seed):
    eng.selfplay_run(0, n_games, base_seed)
    r = eng.selfplay_results()
    games = []
    for g in range(n_games):
        T = int(r["lengths"][g])
        games.append(dict(T=T, moves=r["moves"][g, :T], policy=r["policies"][g, :T],
                          boards=r["boards"][g, :T], expansions=int(r["expansions"][g])))
    return games


@pytest.mark.parametrize("compact", [False, True], ids=["static", "compact"])
@pytest.mark.parametrize("cache_log2", [0, 16], ids=["nocache", "cache16"])
@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("shape", SHAPES)
def test_group_descent_vs_oracle(shape, noise, cache_log2, compact):
    H, W, n, grav, S = shape
    ref = reference(shape, noise)
    kw = dict(dirichlet_noise=True, dirichlet_alpha=NOISE[0], dirichlet_ratio=NOISE[1]) if noise else {}
    for slots in (3, 11):
        eng = az.Engine(H, W, n, grav, S, slots=slots, evaluator=az.EVAL_SYNTHETIC,
                        cache_log2=cache_log2, compact=compact, **kw)
        try:
            got = selfplay_games(eng, GAMES, SEED)
        finally:
            eng.close()
        for g in range(GAMES):
            assert got[g]["T"] == ref[g]["T"], (slots, g)
            np.testing.assert_array_equal(got[g]["moves"], ref[g]["moves"])
            np.testing.assert_array_equal(got[g]["policy"].view(np.uint64), ref[g]["policy"].view(np.uint64))
            np.testing.assert_array_equal(got[g]["boards"], ref[g]["boards"])
            assert got[g]["expansions"] == ref[g]["expansions"], (slots, g)
