"""The forms the default conv_algo falls back to where the one-launch tower
does not take the network (csrc/az_net_form.h; tests/forward_ref.py
FALLBACK_CASES: depth > 16, value_hidden > 256, both on a board wider than 16
columns, and depth 0): each within its case's tolerance of the float64
restatement, bit for bit the explicit algorithm the rule names (both sides run
the same kernels), and the form it really ran pinned through its launch count
and its issued-FLOP figure.  Chess: depth 17 is the per-layer fp16x2 chain."""
import numpy as np
import pytest

import chess_forward_ref as cr
import forward_ref as fr
from custom_alphazero import engine as az
from test_forward_layouts_gpu import check_outputs

pytestmark = pytest.mark.gpu

# case -> the explicit algorithm whose form the default takes (tests/test_net_form_cpu.py asserts both)
NAMED = {"3x3g_d17_h256": az.CONV_F16X2_LAYERS, "3x3g_d1_h300": az.CONV_F16X2_LAYERS,
         "2x20g_d17_h256": az.CONV_DIRECT, "3x3g_d0_h256": az.CONV_DIRECT}


def test_the_table_is_the_fallback_cases():
    assert sorted(NAMED) == sorted(c.name for c in fr.FALLBACK_CASES)


def run(d, conv_algo):
    """One forward of the case's batch with the timer on -> probs, values, the
    conv launches it added, the stats after it."""
    c = d["case"]
    eng = az.Engine(c.H, c.W, c.n, c.gravity, 8, slots=128, evaluator=az.EVAL_NETWORK, depth=c.depth,
                    value_hidden=c.hidden, conv_algo=conv_algo)
    eng.set_weights(d["w"].items())
    eng.timer(True)
    before = eng.stats()["conv_launches"]
    p, v = eng.forward(d["x"])
    st = eng.stats()
    eng.close()
    assert st["errors"] == 0
    return p, v, st["conv_launches"] - before, st


@pytest.mark.parametrize("name", list(NAMED))
def test_default_algo_falls_back_to_the_named_form(name):
    d = fr.case_data(name)
    c = d["case"]
    p, v, launches, st = run(d, az.CONV_F16X2)
    # (c) the per-layer chain: two conv launches per block, no tower and so no issued-FLOP figure
    assert launches == 2 * c.depth, launches
    assert st["issued_flop_per_board"] == 0 and st["issued_flop_per_board_small"] == 0
    assert st["tower_small_max_boards"] == -1
    # (b) the same bits as the explicit algorithm
    q, u, named_launches, _ = run(d, NAMED[name])
    assert named_launches == 2 * c.depth
    np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(v, u)
    if c.depth == 0:  # the per-layer fp16x2 chain has no last conv2 to run the head convs in: the fp32 chain too
        q, u, _, _ = run(d, az.CONV_F16X2_LAYERS)
        np.testing.assert_array_equal(p, q)
        np.testing.assert_array_equal(v, u)
    # (a) the float64 restatement
    check_outputs(d, p, v, slice(None), "default")


def test_control_tower_case_is_one_launch():
    """The same measurements tell the tower apart: one launch, a FLOP figure."""
    d = fr.case_data("3x3g_d1_h256")
    p, v, launches, st = run(d, az.CONV_F16X2)
    assert launches == 1 and st["issued_flop_per_board"] > 0
    check_outputs(d, p, v, slice(None), "tower")


def test_chess_depth_17_is_the_per_layer_fp16x2_chain():
    x = cr.chess_batch()[:8]
    w = cr.lively_chess_weights(17, 256, x, seed=0)
    out = {}
    for algo in (az.CONV_F16X2, az.CONV_F16X2_LAYERS):
        eng = az.ChessEngine(mcts_iterations=1, slots=8, evaluator=az.EVAL_NETWORK, max_plies=4, depth=17,
                             value_hidden=256, conv_algo=algo)
        eng.set_weights(w.items())
        eng.timer(True)
        before = eng.stats()["conv_launches"]
        p, v = eng.forward(x)
        st = eng.stats()
        eng.close()
        assert st["errors"] == 0
        assert st["conv_launches"] - before == 34 and st["issued_flop_per_board"] == 0
        out[algo] = (p, v)
    np.testing.assert_array_equal(out[az.CONV_F16X2][0], out[az.CONV_F16X2_LAYERS][0])
    np.testing.assert_array_equal(out[az.CONV_F16X2][1], out[az.CONV_F16X2_LAYERS][1])
    assert np.ptp(out[az.CONV_F16X2][1]) > 0  # the value head is live
