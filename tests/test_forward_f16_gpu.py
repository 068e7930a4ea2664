"""The one-term fp16 forward (conv_algo = CONV_F16) on the Connect-N tower,
at every layout of forward_ref.CASES.  Bounds are in units of the mode's own
accuracy cost (tests/forward_f16_ref.py: restate16(float64) against the
float64 outputs): the kernel is one more realisation of that rounding, which
tests/test_forward_f16_ref_cpu.py holds within 2 x cost for float32 sums, so
it gets 4 x cost -- half of what the mildest structural mutant moves.  On a
network whose trunk is exact in fp16 the mode must equal the default
arithmetic bit for bit (the two sum the same products in the same order when
every second term is zero), which catches a wrong tap, fragment, slot or skip
at the bit level.  Self-play replays on the oracle bit for bit, as in the
default mode."""
import numpy as np
import pytest

import forward_f16_ref as f16
import forward_ref as fr
import oracle
from custom_alphazero import engine as az
from test_engine_gpu import selfplay_games

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in fr.CASES]


def make_engine(c, w, conv_algo=az.CONV_F16, slots=128, S=8, **kw):
    eng = az.Engine(c.H, c.W, c.n, c.gravity, S, slots=slots, evaluator=az.EVAL_NETWORK, depth=c.depth,
                    value_hidden=c.hidden, conv_algo=conv_algo, **kw)
    eng.set_weights(w.items())
    return eng


def check_cost(name, p, v, rows, label):
    d, k = fr.case_data(name), f16.costs(name)
    ep, ev = float(np.abs(p - d["p"][rows]).max()), float(np.abs(v - d["v"][rows]).max())
    print(f"F16ERR {name} {label} cost_p {k['cost_p']:.2e} cost_v {k['cost_v']:.2e} policy {ep:.2e} = "
          f"{ep / k['cost_p']:.2f} cost value {ev:.2e} = {ev / k['cost_v']:.2f} cost")
    assert ep <= 4 * k["cost_p"], (label, ep, k["cost_p"])
    assert ev <= 4 * k["cost_v"], (label, ev, k["cost_v"])
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_one_term_forward_within_four_costs(name):
    d = fr.case_data(name)
    c, x = d["case"], d["x"]
    eng = make_engine(c, d["w"])
    p, v = eng.forward(x)
    st = eng.stats()
    eng.close()
    check_cost(name, p, v, slice(None), "tower")
    assert st["errors"] == 0
    ref = make_engine(c, d["w"], az.CONV_F16X2)
    p3, v3 = ref.forward(x)
    st3 = ref.stats()
    ref.close()
    assert not (np.array_equal(p, p3) and np.array_equal(v, v3))  # it is another arithmetic
    assert st["issued_flop_per_board"] > 0 and st["issued_flop_per_board"] * 3 == st3["issued_flop_per_board"]
    assert st["issued_flop_per_board_small"] * 3 == st3["issued_flop_per_board_small"]
    assert (st["issued_flop_per_board_small"] > 0) == bool(fr.layouts()[name]["dual"])
    assert st["tower_small_max_boards"] == st3["tower_small_max_boards"]


@pytest.mark.parametrize("name", NAMES)
def test_one_term_forward_same_bits_in_natural_order_and_across_tiles(name):
    d = fr.case_data(name)
    c, x = d["case"], d["x"]
    eng = make_engine(c, d["w"])
    p, v = eng.forward(x)
    bpw = fr.layouts()[name]["boards"]
    assert 3 + bpw + 1 <= len(x)
    for lo, hi in ((0, 1), (3, 3 + bpw + 1)):
        q, u = eng.forward(x[lo:hi])
        np.testing.assert_array_equal(q, p[lo:hi], err_msg=f"[{lo}:{hi}]")
        np.testing.assert_array_equal(u, v[lo:hi], err_msg=f"[{lo}:{hi}]")
    assert eng.stats()["errors"] == 0
    eng.close()
    nat = make_engine(c, d["w"], tower_natural_order=True)
    pn, vn = nat.forward(x)
    assert nat.stats()["errors"] == 0
    nat.close()
    np.testing.assert_array_equal(p, pn)
    np.testing.assert_array_equal(v, vn)


@pytest.mark.parametrize("name", fr.DUAL_CASES)
def test_one_term_dual_launch_heights_agree(name):
    """test_forward_dual_launch_heights_agree's construction: a launch of at
    most tower_small_max_boards boards runs the 96-row tiles, a larger one
    the 128-row tiles -- the same bits for a board either way."""
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
    check_cost(name, p_small, v_small, slice(None), "tower-96")
    check_cost(name, p_big, v_big, rows, "tower-128")


@pytest.mark.parametrize("shape", f16.EXACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_d{s[3]}")
def test_one_term_equals_default_bitwise_on_the_exact_network(shape):
    H, W, gravity, depth, hidden, seed = shape
    c = fr.Case("exact", H, W, min(4, H, W), gravity, depth, hidden)
    w = f16.exact_network(H, W, gravity, depth, hidden, seed)
    x = f16.onehot_batch(H, W)
    out = {}
    for algo in (az.CONV_F16, az.CONV_F16X2):
        eng = make_engine(c, w, algo, bn_epsilon=f16.EXACT_EPS)
        out[algo] = eng.forward(x)
        assert eng.stats()["errors"] == 0
        eng.close()
    p, v = out[az.CONV_F16]
    np.testing.assert_array_equal(p, out[az.CONV_F16X2][0])
    np.testing.assert_array_equal(v, out[az.CONV_F16X2][1])
    p64, v64 = f16.restate16(w, x, depth, np.float64, f16.EXACT_EPS)
    assert np.abs(p - p64).max() <= 1e-5 and np.abs(v - v64).max() <= 1e-5
    assert len(np.unique(v)) > len(v) // 2  # the outputs depend on the board


def replay(cfg, **kw):
    H, W, n, grav, depth, S, n_games = cfg
    c = fr.Case("selfplay", H, W, n, grav, depth, 256)
    w = fr.lively_weights(H, W, grav, depth, 256, fr.make_batch(H, W), seed=0)
    eng = make_engine(c, w, slots=n_games, S=S, **kw)
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
    return games


@pytest.mark.parametrize("cfg", [(3, 3, 3, True, 1, 8, 4), (6, 7, 4, True, 2, 10, 2)])
def test_one_term_selfplay_replays_on_oracle(cfg):
    """The eval queue's one-hot boards are exact fp16 operands: self-play's
    forward is bitwise forward(full_state(board)), so the oracle fed the
    engine's own batch-1 forward reproduces every game; with the
    transposition cache on, the same games."""
    games = replay(cfg)
    if cfg[0] == 6:
        cached = replay(cfg, cache_log2=10)
        for a, b in zip(games, cached):
            assert a["T"] == b["T"]
            np.testing.assert_array_equal(a["moves"], b["moves"])
            np.testing.assert_array_equal(a["policy"].view(np.uint64), b["policy"].view(np.uint64))


def test_one_term_needs_the_tower():
    with pytest.raises(az.AzError, match="AZ_CONV_F16"):
        az.Engine(6, 7, 4, True, 8, slots=4, evaluator=az.EVAL_NETWORK, depth=0, conv_algo=az.CONV_F16)
    with pytest.raises(az.AzError, match="AZ_CONV_F16"):
        az.Engine(6, 7, 4, True, 8, slots=4, evaluator=az.EVAL_NETWORK, value_hidden=300, conv_algo=az.CONV_F16)
