"""The one-term fp16 forward (conv_algo = CONV_F16) on the chess tower (the
input-row form: the 118-plane stem as a K loop, 128- and 64-row tiles):
tests/test_forward_f16_gpu.py's bounds -- 4 x the mode's own accuracy cost,
tests/forward_f16_ref.py -- on chess_forward_ref.CASES, the same bits at
launch sizes on both sides of the 64- / 128-row switch, self-play (the stem
that skips the two known-zero input chunks) replayed on the oracle bit for
bit, and bitwise equality with the default arithmetic on a network that is
exact in fp16."""
import numpy as np
import pytest

import chess_forward_ref as cr
import chess_oracle as C
import forward_f16_ref as f16
from custom_alphazero import engine as az
from test_chess_forward_layouts_gpu import SHIPPED, _batch1
from test_chess_selfplay_gpu import _compare

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cr.CASES]


def make_engine(depth, hidden, w, conv_algo=az.CONV_F16, slots=64, sims=1, plies=4, **kw):
    eng = az.ChessEngine(mcts_iterations=sims, slots=slots, evaluator=az.EVAL_NETWORK, max_plies=plies, depth=depth,
                         value_hidden=hidden, conv_algo=conv_algo, **kw)
    eng.set_weights(w.items())
    return eng


def check_cost(name, p, v, rows, label):
    d, k = cr.case_data(name), f16.costs(name)
    ep, ev = float(np.abs(p - d["p"][rows]).max()), float(np.abs(v - d["v"][rows]).max())
    print(f"F16ERR {name} {label} cost_p {k['cost_p']:.2e} cost_v {k['cost_v']:.2e} policy {ep:.2e} = "
          f"{ep / k['cost_p']:.2f} cost value {ev:.2e} = {ev / k['cost_v']:.2f} cost")
    assert ep <= 4 * k["cost_p"], (label, ep, k["cost_p"])
    assert ev <= 4 * k["cost_v"], (label, ev, k["cost_v"])
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_chess_one_term_forward_within_four_costs(name):
    d = cr.case_data(name)
    c = d["case"]
    eng = make_engine(c.depth, c.hidden, d["w"])
    p, v = eng.forward(d["x"])
    st = eng.stats()
    eng.close()
    check_cost(name, p, v, slice(None), "tower")
    assert st["errors"] == 0
    ref = make_engine(c.depth, c.hidden, d["w"], az.CONV_F16X2)
    p3, v3 = ref.forward(d["x"])
    st3 = ref.stats()
    ref.close()
    assert not (np.array_equal(p, p3) and np.array_equal(v, v3))  # it is another arithmetic
    assert st["issued_flop_per_board"] > 0 and st["issued_flop_per_board"] * 3 == st3["issued_flop_per_board"]


def test_chess_one_term_bits_do_not_depend_on_launch_size():
    """2 and 511 boards run 64-row tiles of one board, 512 and 513 the
    128-row tiles of two (an odd count: the last tile half empty)."""
    d = cr.case_data(SHIPPED)
    c, x = d["case"], d["x"]
    eng = make_engine(c.depth, c.hidden, d["w"], slots=520, lanes=1)
    p29, v29 = eng.forward(x)
    for n in (2, 511, 512, 513):
        rows = (np.arange(n) * 7 + 3) % len(x)
        p, v = eng.forward(x[rows])
        np.testing.assert_array_equal(p, p29[rows], err_msg=f"n = {n}")
        np.testing.assert_array_equal(v, v29[rows], err_msg=f"n = {n}")
    assert eng.stats()["errors"] == 0
    eng.close()
    check_cost(SHIPPED, p, v, rows, "tower-513")


def test_chess_one_term_selfplay_replays_on_oracle():
    """test_chess_selfplay_replays_on_oracle_with_lively_weights' smallest
    configuration (3 slots: 64-row tiles, the leaves' planes built in the
    stem, first_chunk 2) in the one-term mode: bit for bit."""
    d = cr.case_data(SHIPPED)
    c = d["case"]
    eng = make_engine(c.depth, c.hidden, d["w"], sims=16, plies=12, slots=3)
    st = eng.selfplay_run(0, 3, 77)
    r = eng.selfplay_results()
    assert st["errors"] == 0 and st["games_done"] == 3
    cb = _batch1(eng)
    for g in range(3):
        _compare(r, g, C.play_game(16, 77 + g, 12, callback=cb), "one-term tower")
    values = {v for _, v in cb.seen.values()}
    assert len(cb.seen) > 100 and len(values) > len(cb.seen) // 2, (len(values), len(cb.seen))  # the value head is live
    eng.close()


def test_chess_one_term_equals_default_bitwise_on_the_exact_network():
    depth, hidden, seed = f16.EXACT_CHESS
    w = f16.exact_network(8, 8, False, depth, hidden, seed, in_channels=cr.PLANES, A=cr.ACTIONS)
    x = f16.exact_chess_batch()
    out = {}
    for algo in (az.CONV_F16, az.CONV_F16X2):
        eng = make_engine(depth, hidden, w, algo, bn_epsilon=f16.EXACT_EPS)
        out[algo] = eng.forward(x)
        assert eng.stats()["errors"] == 0
        eng.close()
    p, v = out[az.CONV_F16]
    np.testing.assert_array_equal(p, out[az.CONV_F16X2][0])
    np.testing.assert_array_equal(v, out[az.CONV_F16X2][1])
    p64, v64 = f16.restate16(w, x, depth, np.float64, f16.EXACT_EPS)
    assert np.abs(p - p64).max() <= 1e-5 and np.abs(v - v64).max() <= 1e-5
    assert len(np.unique(v)) > len(v) // 2  # the outputs depend on the board
