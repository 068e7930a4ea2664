"""What the GPU bounds of the one-term forward (AZ_CONV_F16) rest on, for
every case of forward_ref.CASES and chess_forward_ref.CASES
(tests/forward_f16_ref.py has the definitions):

  1. restate16(float32) lies within 2 x cost of the float64 outputs, in
     policy and value: another realisation of the mode's rounding (fp32
     sums in another order) costs no more than twice the mode itself, so the
     kernel -- one more such realisation -- is held to 4 x cost on the GPU;
  2. the mildest structural mutant that moves the policy (M3, M5; chess also
     M6), applied on top of restate16(float64), moves it by at least 8 x
     cost_p: twice the GPU bound, so no such error hides inside it.
     (chess_forward_ref's M7 rounds the input to fp16, which this mode does
     anyway: on restate16 it is the identity and cannot be asked to move
     anything);
  3. M4 moves the value by at least 8 x cost_v;
  4. the exact network's float64 trunk holds integers of magnitude <= 2048
     in every stored activation, at least 20 % of each layer positive, and
     the float32 trunk equals it exactly -- the premise of the bitwise
     comparison of the two modes on the GPU."""
import numpy as np
import pytest

import chess_forward_ref as cr
import forward_f16_ref as f16
import forward_ref as fr

NAMES = [c.name for c in fr.CASES] + [c.name for c in cr.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_within_twice_the_cost(name):
    d, _ = f16._data(name)
    k = f16.costs(name)
    p32, v32 = f16.restate16(d["w"], d["x"], d["case"].depth, np.float32)
    ep, ev = f16._dist(p32, d["p"]), f16._dist(v32, d["v"])
    print(f"{name}: cost_p {k['cost_p']:.3e} cost_v {k['cost_v']:.3e}; float32 {ep / k['cost_p']:.2f} x, "
          f"{ev / k['cost_v']:.2f} x")
    assert ep <= 2 * k["cost_p"] and ev <= 2 * k["cost_v"]


@pytest.mark.parametrize("name", NAMES)
def test_mutants_move_the_outputs_eight_costs(name):
    k, m = f16.costs(name), f16.moved(name)
    policy = ("M3", "M5") + (("M6",) if name.startswith("chess") else ())
    mild_p = min(m[x][0] for x in policy)
    print(f"{name}: mildest policy mutant {mild_p / k['cost_p']:.1f} x cost_p, M4 {m['M4'][1] / k['cost_v']:.1f} x cost_v")
    assert mild_p >= 8 * k["cost_p"], m
    assert m["M4"][1] >= 8 * k["cost_v"], m


def _exact_checks(w, x, depth):
    s64, s32 = [], []
    h64 = f16.trunk16(w, x, depth, np.float64, f16.EXACT_EPS, stored=s64)
    h32 = f16.trunk16(w, x, depth, np.float32, f16.EXACT_EPS, stored=s32)
    assert len(s64) == 2 * depth  # the stem, conv1 outputs and the block outputs but the last
    for a64, a32 in zip(s64 + [h64], s32 + [h32]):
        assert np.array_equal(a64, np.round(a64)) and np.abs(a64).max() <= 2048
        assert (a64 > 0).mean() >= 0.2, (a64 > 0).mean()
        assert np.array_equal(a64, a32.astype(np.float64))


@pytest.mark.parametrize("shape", f16.EXACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_d{s[3]}")
def test_exact_network_is_exact(shape):
    H, W, gravity, depth, hidden, seed = shape
    w = {k: np.asarray(v, np.float64) for k, v in f16.exact_network(H, W, gravity, depth, hidden, seed).items()}
    _exact_checks(w, f16.onehot_batch(H, W), depth)


def test_exact_chess_network_is_exact():
    depth, hidden, seed = f16.EXACT_CHESS
    w = f16.exact_network(8, 8, False, depth, hidden, seed, in_channels=cr.PLANES, A=cr.ACTIONS)
    _exact_checks({k: np.asarray(v, np.float64) for k, v in w.items()}, f16.exact_chess_batch(), depth)
