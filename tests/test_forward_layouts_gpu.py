"""The inference forward against the float64 restatement at every tower layout
load_network chooses (tests/forward_ref.py: the case table, lively heads, and
per case a tolerance an eighth of what the mildest mutant does -- DESIGN
section 3 has the measured errors), with every conv algorithm the engine
accepts for the board; what the engine chose pinned through its issued FLOP;
batch invariance across tiles; the dual launch's two tile heights; and the
self-play input path (boards from the eval queue) by oracle replay."""
import numpy as np
import pytest

import forward_ref as fr
import oracle
from custom_alphazero import engine as az
from test_engine_gpu import selfplay_games

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in fr.CASES]
ALGOS = {"tower": az.CONV_F16X2, "direct": az.CONV_DIRECT, "layers": az.CONV_F16X2_LAYERS}


def accepted(c, algo):
    return algo != "layers" or c.W <= 16


def make_engine(c, w, algo="tower", slots=128, S=8, **kw):
    eng = az.Engine(c.H, c.W, c.n, c.gravity, S, slots=slots, evaluator=az.EVAL_NETWORK, depth=c.depth,
                    value_hidden=c.hidden, conv_algo=ALGOS[algo], **kw)
    eng.set_weights(w.items())
    return eng


def check_outputs(d, p, v, rows, label):
    """p, v of the batch rows `rows` within the case's tolerances; prints the
    measured error over e32 and over tol (the table of DESIGN section 3)."""
    ep, ev = float(np.abs(p - d["p"][rows]).max()), float(np.abs(v - d["v"][rows]).max())
    print(f"FWDERR {d['case'].name} {label} policy {ep:.2e} = {ep / d['e32_p']:.2f} e32 = {ep / d['tol_p']:.3f} tol; "
          f"value {ev:.2e} = {ev / d['e32_v']:.2f} e32 = {ev / d['tol_v']:.3f} tol")
    assert ep <= d["tol_p"], (label, ep, d["tol_p"])
    assert ev <= d["tol_v"], (label, ev, d["tol_v"])
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("name", NAMES)
def test_forward_case_matches_float64(name, algo):
    d = fr.case_data(name)
    c, x = d["case"], d["x"]
    if not accepted(c, algo):
        with pytest.raises(az.AzError, match="16 columns"):
            make_engine(c, d["w"], algo)
        return
    eng = make_engine(c, d["w"], algo)
    p, v = eng.forward(x)
    st = eng.stats()
    eng.close()
    check_outputs(d, p, v, slice(None), algo)
    assert st["errors"] == 0
    if algo != "tower":
        return
    # what the engine really chose -- tile rows, boards per tile, the plan's skips -- through the
    # FLOP it issues per board, against the layout program's figures; and the plan changes no bit
    L = fr.layouts()[name]
    nat = make_engine(c, d["w"], algo, tower_natural_order=True)
    pn, vn = nat.forward(x)
    stn = nat.stats()
    nat.close()
    assert L["tower"] and stn["errors"] == 0
    assert stn["issued_flop_per_board"] == L["flop_natural"], (stn["issued_flop_per_board"], L)
    assert st["issued_flop_per_board"] == L["flop"], (st["issued_flop_per_board"], L)
    if L["dual"]:
        assert stn["issued_flop_per_board_small"] == L["alt_flop_natural"]
        assert st["issued_flop_per_board_small"] == L["alt_flop"]
        assert st["tower_small_max_boards"] > 0
    else:
        assert st["issued_flop_per_board_small"] == 0 and st["tower_small_max_boards"] == -1
    np.testing.assert_array_equal(p, pn)
    np.testing.assert_array_equal(v, vn)


@pytest.mark.parametrize("name", NAMES)
def test_forward_case_is_batch_invariant_across_tiles(name):
    """One board, a batch one board longer than a tile that starts inside
    another tile's boards, and the whole batch: the same bits per board."""
    d = fr.case_data(name)
    c, x = d["case"], d["x"]
    bpw = fr.layouts()[name]["boards"]
    assert 3 + bpw + 1 <= len(x)
    for algo in ALGOS:
        if not accepted(c, algo):
            continue
        eng = make_engine(c, d["w"], algo)
        p, v = eng.forward(x)
        for lo, hi in ((0, 1), (3, 3 + bpw + 1)):
            q, u = eng.forward(x[lo:hi])
            np.testing.assert_array_equal(q, p[lo:hi], err_msg=f"{algo} [{lo}:{hi}]")
            np.testing.assert_array_equal(u, v[lo:hi], err_msg=f"{algo} [{lo}:{hi}]")
        assert eng.stats()["errors"] == 0
        eng.close()


@pytest.mark.parametrize("name", fr.DUAL_CASES)
def test_forward_dual_launch_heights_agree(name):
    """A launch of at most tower_small_max_boards boards runs the 96-row tiles
    (with their own staging and plan), a larger one the 128-row tiles: the
    same bits for a board either way, both within the case's tolerances."""
    d = fr.case_data(name)
    c, x = d["case"], d["x"]
    eng = make_engine(c, d["w"], slots=256, lanes=8)
    thr = eng.stats()["tower_small_max_boards"]
    assert len(x) < thr and thr + 5 <= 256, thr  # one launch each
    rows = np.arange(thr + 5) % len(x)
    p_small, v_small = eng.forward(x)
    p_big, v_big = eng.forward(x[rows])
    assert eng.stats()["errors"] == 0
    eng.close()
    np.testing.assert_array_equal(p_small, p_big[:len(x)])
    np.testing.assert_array_equal(v_small, v_big[:len(x)])
    check_outputs(d, p_small, v_small, slice(None), "tower-96")
    check_outputs(d, p_big, v_big, rows, "tower-128")


@pytest.mark.parametrize("cfg", [(3, 3, 3, True, 1, 8, 4), (11, 11, 5, True, 2, 6, 2), (6, 7, 4, True, 16, 10, 2)])
def test_selfplay_replays_on_oracle_with_lively_weights(cfg):
    """Self-play's tower reads its boards from the eval queue, not from x: the
    oracle, fed the engine's own batch-1 forward of every board it asks about,
    reproduces every move and visit-count policy bit for bit -- with heads
    whose outputs depend on the board (8 boards per 96-row tile; one board per
    tile; 128-row tiles in place)."""
    H, W, n, grav, depth, S, n_games = cfg
    c = fr.Case("selfplay", H, W, n, grav, depth, 256)
    w = fr.lively_weights(H, W, grav, depth, 256, fr.make_batch(H, W), seed=0)
    eng = make_engine(c, w, slots=n_games, S=S)
    games = selfplay_games(eng, 0, n_games, base_seed=123)
    cache = {}

    def cb(board):
        key = board.tobytes()
        if key not in cache:
            p, v = eng.forward(oracle.full_state(board[None]))
            cache[key] = (p[0], float(v[0]))
        return cache[key]

    for g, got in enumerate(games):
        ref = oracle.play_game(H, W, n, grav, S, 123 + g, evaluator="callback", callback=cb)
        assert got["T"] == ref["T"]
        np.testing.assert_array_equal(got["moves"], ref["moves"])
        np.testing.assert_array_equal(got["policy"].view(np.uint64), ref["policy"].view(np.uint64))
        assert got["expansions"] == ref["expansions"]
    assert len({v for _, v in cache.values()}) > len(cache) // 2  # the value head is live
    assert eng.stats()["errors"] == 0
    eng.close()
