"""What the chess trainer fixes without a GPU: the spec it trains, its refusal
to run without a device (there is no CPU fallback), the model's precondition,
the bench's `game` argument and the shape of the test batches."""
import inspect

import numpy as np
import pytest

import train_chess_ref as C
from custom_alphazero import engine as az


def test_chess_spec_names_and_shapes():
    spec = C.make_spec(2, hidden=40)
    shapes = dict(spec)
    assert shapes["stem.kernel"] == (3, 3, 118, 128)
    assert shapes["policy.dense.kernel"] == (128, 1880) and shapes["policy.dense.bias"] == (1880,)
    assert shapes["value.dense1.kernel"] == (64, 40) and shapes["value.dense2.kernel"] == (40, 1)
    assert shapes["block1.conv2.kernel"] == (3, 3, 128, 128) and shapes["block1.res.kernel"] == (1, 1, 128, 128)
    assert shapes["policy.conv.kernel"] == (1, 1, 128, 2) and shapes["value.conv.kernel"] == (1, 1, 128, 1)
    assert "block2.conv1.kernel" not in shapes and len(spec) == 6 * (1 + 3 * 2 + 2) + 6
    # the trainer class carries the same spec as the chess engine loads
    assert az.ChessTrainer.planes == 118 and issubclass(az.ChessTrainer, az.Trainer)
    assert "az_chess_trainer_create" in az.EXPORTED


def test_chess_trainer_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(az.AzError, match="no HIP device"):
        az.ChessTrainer(max_batch=4, depth=1)


def test_chess_trainer_validates_before_it_opens_a_device():
    """The refusals run on the host, in front of the device: they answer the same with or without a GPU."""
    with pytest.raises(az.AzError, match="error -1.*filters"):
        az.ChessTrainer(max_batch=4, filters=64, depth=1)
    with pytest.raises(az.AzError, match="error -1.*depth"):
        az.ChessTrainer(max_batch=4, depth=17)
    with pytest.raises(az.AzError, match="error -1.*value_hidden"):
        az.ChessTrainer(max_batch=4, depth=1, value_hidden=0)
    with pytest.raises(az.AzError, match="error -1.*max_batch"):
        az.ChessTrainer(max_batch=262144, depth=1)


def test_a_model_without_weights_has_no_trainer():
    from custom_alphazero.model.policy_value import PolicyValueModel
    for dim, actions in (((8, 8, 118), 1880), ((6, 7, 4), 7)):
        hollow = PolicyValueModel.__new__(PolicyValueModel)
        hollow.input_dim, hollow.action_space, hollow._trainer = dim, actions, None
        with pytest.raises(az.AzError, match="error -1.*no weights"):
            hollow.trainer()


def test_bench_takes_a_game():
    from custom_alphazero import train
    p = inspect.signature(train.bench).parameters
    assert p["game"].default == "connect_n"
    assert inspect.signature(train.step_flop).parameters["stem_planes"].default == 0
    assert train.step_flop(256, 6, 7, 4) == 3.0 * 4 * 19 * 2.0 * 256 * 42 * 128 * 128


def test_batches_are_shaped_like_full_state():
    x, pi, z = C.make_batch(9, seed=1)
    assert x.shape == (9, 8, 8, 118) and pi.shape == (9, 1880) and z.shape == (9,)
    for s in range(8):
        onehot = x[..., 14 * s:14 * s + 13]
        assert set(np.unique(onehot.sum(axis=-1))) <= {0.0, 1.0}            # one piece code per cell, or no history
        rep = x[..., 14 * s + 13]
        assert np.all(rep == rep[:, :1, :1]) and set(np.unique(rep)) <= {0.0, 1.0}
    assert np.all(x[0::3, :, :, :84] == 0) and np.all(x[1, :, :, :84].sum(axis=-1) >= 6)
    tail = x[..., 112:]
    assert np.all(tail == tail[:, :1, :1])                                   # constant over a board
    assert set(np.unique(tail[..., :4])) <= {0.0, 1.0} and x[..., 116].min() >= 1 and x[..., 116].max() >= 100
    assert set(C.ZERO_PLANES) <= set(C.zero_planes(x)) and len(C.zero_planes(C.make_batch(1)[0])) >= 84
    counts = (pi > 0).sum(axis=1)
    assert counts[0] == 1 and pi[0].max() == 1.0 and counts[1] == 218 and counts.max() <= 218
    np.testing.assert_allclose(pi.sum(axis=1), 1.0, atol=1e-6)
    assert set(np.unique(z)) <= {-1.0, 0.0, 1.0}


# ------------------------------------------------------------ the edge cases' inputs (test_train_chess_shapes_gpu.py)
def test_reference_run_keeps_its_defaults():
    """No mods and eps = 1e-3 are the run every earlier caller got: same batch seed, same cache entry."""
    ref = C.reference_run(3, 1, **C.HYPER)
    assert C.reference_run(3, 1, weights_mod=None, batch_mod=None, eps=1e-3, batch_seed=0, **C.HYPER) is ref
    assert C.reference_run(3, 1, eps=1e-5, **C.HYPER) is not ref
    assert C.BATCH_SEEDS[(5, 2)] == 5 and C.BATCH_SEEDS[(4, 1, 1)] == 1 and C.BATCH_SEEDS[(4, 4)] == 3
    x, pi, z = C.make_batch(3, 0)
    assert np.array_equal(ref["batch"][0], x) and np.array_equal(ref["batch"][1], pi)
    named = C.reference_run(4, 1, hidden=1, **C.HYPER)
    assert np.array_equal(named["batch"][0], C.make_batch(4, 1)[0])
    assert sorted(C.PARITY_CASES) == sorted(set(C.PARITY_CASES)) and len(C.PARITY_CASES) == len(C.EDGE_SHAPES) + 6


@pytest.mark.parametrize("case", list(C.PARITY_CASES))
def test_parity_inputs_meet_the_input_condition(case):
    """What every case of test_train_chess_shapes_gpu.py asserts before it touches the device, here
    without one: every compared tensor's e32 <= KINK_FREE, ReLU margin >= 0.95 x CLEAR_MARGIN."""
    (n, depth, hidden), more, gradients = C.PARITY_CASES[case]
    ref = C.reference_run(n, depth, hidden=hidden, **more, **C.HYPER)
    worst, at, margin = C.input_condition(ref, case, gradients)
    e32 = [abs(a - b) / abs(b) for a, b in zip(ref["f32"][0]["losses"], ref["f64"][0]["losses"])]
    print(f"{case}: worst e32 {worst:.2e} ({at}), ReLU margin {margin:.2e}, losses' e32 "
          + " / ".join(f"{e:.1e}" for e in e32))
    assert set(C.ZERO_PLANES) <= set(C.zero_planes(ref["batch"][0]))
    if case == "n4_d4_h256":  # the depth case keeps a margin of two under KINK_FREE (EDGE_SHAPES)
        assert worst <= C.KINK_FREE / 2


@pytest.mark.parametrize("shape", [(4, 4, 256), (4, 1, 1024)], ids=["n4_d4", "n4_d1_h1024"])
def test_batch_seeds_named_by_cancellation_are_the_criterions(shape):
    """BATCH_SEEDS' entries for these shapes are what batch_seed_by_cancellation picks of seeds 0..9
    (float64 alone), and the pick's head scalars cancel less than tenfold."""
    seed, ratios = C.batch_seed_by_cancellation(*shape)
    print(f"{shape}: largest head cancellation ratio per batch seed "
          + ", ".join(f"{s}: {r:.1f}" for s, r in ratios.items()))
    assert C.BATCH_SEEDS.get(shape, C.BATCH_SEEDS.get(shape[:2])) == seed
    assert ratios[seed] < 10 < ratios[0]


@pytest.mark.parametrize("case", ["policy_x4", "policy_x8"])
def test_the_epsilon_in_the_log_carries_the_gradient(case):
    """policy.dense.kernel x4 / x8: a target move's probability falls below 1e-6, and the float64
    gradient of the loss without the 1e-7 is 100 tolerances or more from the true one."""
    ref = C.parity_reference(case)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    short, pmin = C.shortcut_gradient(ref, 1, ["policy.dense.bias", "stem.kernel"])
    assert pmin < 1e-6
    for k in short:
        assert C.rel_l2(short[k], g64[k]) >= 100 * C.tolerance(C.rel_l2(g32[k], g64[k])), k


def test_saturated_dead_and_epsilon_inputs_are_what_they_claim():
    ref = C.parity_reference("saturated")
    _, v = C.float64_forward(ref, 1)
    assert np.abs(v).max() >= 0.97 and C.SATURATION in (10, 8, 6)
    ref = C.parity_reference("dead_channels")
    for unit, c in C.DEAD.items():
        assert not ref["weights"][unit + ".kernel"][..., c].any()
        var1, var0 = ref["f64"][0]["w"][unit + ".var"][c], float(ref["weights"][unit + ".var"][c])
        assert abs(var1 - C.HYPER["bn_momentum"] * var0) <= 1e-12 * var1 and 0 < var1 < var0
    ref = C.parity_reference("eps_1e-5")
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    other = C.gradient_at_another_epsilon(ref, 1, 1e-3)
    assert max(C.rel_l2(other[k], g64[k]) / C.tolerance(C.rel_l2(g32[k], g64[k]))
               for k in g64 if C.conv_bias_unit(k) is None) >= 100
    same = C.gradient_at_another_epsilon(ref, 1, C.EPS_CASE)
    assert all(np.array_equal(same[k], g64[k]) for k in g64)
