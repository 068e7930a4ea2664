"""The chess network's training step on the device (az_chess_trainer_create,
engine.ChessTrainer, csrc/az_train.hip chess_stem_* / chess_heads_kernel)
against the float64 torch restatement (tests/train_chess_ref.py: train_ref's
restatement on the chess spec and on batches shaped like Board.full_state).

The rules are tests/test_train_gpu.py's.  Per tensor, e32 = the relative L2
error of the restatement's own float32 CPU run against float64; the device must
be within train_ref.tolerance(e32) = max(8 * e32, 1e-6), never looser than
1e-4.  Every e32 must stay below 1.25e-5 (KINK_FREE): the weights come through
clear_kinks, which keeps every ReLU input of the first step 2e-5 from zero on
the float64 run, and the two-step test's batch seed keeps the second step's
1e-6 from zero (train_chess_ref.BATCH_SEEDS, asserted).  The bias of a conv in
front of a training-mode BN has a true gradient of 0: the device's stays below
1e-4 of that unit's gamma gradient norm.

Input channels that are zero over the whole batch (planes 13 and 115 in every
batch, planes 0..83 as well at n = 1) get no data gradient: the stem kernel's
gradient there is exactly 0.0 when the step runs with l2 = 0, and with the
tests' l2 = 1e-4 exactly the L2 term float32(2 * l2) * w and nothing else (the
trainer's gradient is the total loss's).  Both are asserted.

Worst device error measured on an MI355X, relative L2 over every tensor
(gradient of the total loss, one step), the tensor closest to its bound, and
the losses' errors (total / policy / value):
  n 1, depth 1             1.5e-6  stem.beta 1.46e-6 of 6.15e-6           6.1e-8 / 5.9e-8 / 2.5e-7
  n 3, depth 1             9.8e-7  block0.conv1.beta 8.5e-7 of 7.4e-6     2.0e-8 / 4.5e-9 / 6.0e-8
  n 9, depth 1             1.2e-6  block0.conv1.beta 9.7e-7 of 7.9e-6     7.3e-9 / 5.5e-9 / 1.2e-8
  n 5, depth 2             1.4e-6  value.conv.gamma 1.006e-6 of 1.048e-6  1.8e-8 / 1.4e-8 / 1.1e-7
  n 3, depth 1, hidden 40  2.3e-6  stem.beta 1.36e-6 of 1.85e-5           2.8e-8 / 4.5e-9 / 2.0e-7
  n 5, depth 2, two steps: momentum 1.5e-6 (value.conv.gamma 1.5e-7 of 1e-6), moving statistics
                           2.6e-7 (value.conv.mean 1.7e-7 of 1e-6)
One tensor is close to its bound: value.conv.gamma at (5, 2), one scalar, a
sum of 320 terms of both signs (their root sum of squares is 3.3 times the
sum, their absolute sum 29 times).  With every term carrying the step's general
fp32 error of about 3e-7, the sum is off by about 1e-6, where the device lands; the CPU's
float32 run happens to hit the scalar within 1.3e-7 (2.7e-7 on another CPU), so
its bound is barely above the rule's floor of 1e-6.  Summing the head convs'
dots in float64 did not move it (1.17e-6): the error comes with the tower's
fp32 activations, not from the head's arithmetic.  The moving mean of the same
head missed its bound at first (1.8e-6 of 1e-6): m * mean + (1 - m) * mu
cancels there fivefold and moving_update_kernel's fp32 `1 - 0.99f` is 9.5e-7
short of 0.01; the chess trainer now passes the factor rounded once from
float64 (1.7e-7).
"""
import numpy as np
import pytest

import train_chess_ref as C
from custom_alphazero import engine as az
from custom_alphazero.config import ConfigModel

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, momentum=0.9, l2=1e-4, bn_momentum=0.99)
# (n, depth, hidden): one 64-row part; a partial board part; a crossing of kBoardsPerPart = 8; two blocks;
# a value head of another width
SHAPES = [(1, 1, 256), (3, 1, 256), (9, 1, 256), (5, 2, 256), (3, 1, 40)]


def _reference(shape, steps=1):
    """The shared CPU runs, after the condition on the inputs: no ReLU kinks in the steps compared."""
    n, depth, hidden = shape
    ref = C.reference_run(n, depth, steps=steps, hidden=hidden, **HYPER)
    for s in range(steps):
        g64, g32 = ref["f64"][s]["grad"], ref["f32"][s]["grad"]
        for k in g64:
            if C.conv_bias_unit(k) is None:
                assert C.rel_l2(g32[k], g64[k]) <= C.KINK_FREE, (shape, s, k)
        if s == 0:  # clear_kinks built the weights for this (less their rounding to float32)
            assert ref["f64"][s]["relu_margin"] >= 0.95 * C.CLEAR_MARGIN, (shape, s)
        else:
            assert ref["f64"][s]["relu_margin"] >= C.MIN_RELU_MARGIN, (shape, s)
    return ref


def _trainer(shape, ref, max_batch=None):
    n, depth, hidden = shape
    tr = az.ChessTrainer(max_batch=max_batch or n, depth=depth, value_hidden=hidden)
    tr.set_weights(ref["weights"].items())
    return tr


def _check_tensors(dev, ref64, ref32, what, shape):
    report, worst = [], 0.0
    for k, r64 in ref64.items():
        if C.conv_bias_unit(k) is not None and what != "w":
            continue
        e32 = C.rel_l2(ref32[k], r64)
        err = C.rel_l2(dev[k], r64)
        worst = max(worst, err)
        report.append((err, C.tolerance(e32), k))
    err, tol, k = max(report, key=lambda r: r[0] / r[1])
    print(f"{what} {shape}: worst device error {worst:.3e}; closest to its bound: {k} {err:.3e} of {tol:.3e}")
    bad = [(k, err, tol) for err, tol, k in report if not err <= tol]
    assert not bad, (what, shape, bad[:8])


def _state(tr):
    return [tr.read_all(az.TRAIN_WEIGHT), tr.read_all(az.TRAIN_GRAD), tr.read_all(az.TRAIN_MOMENTUM)]


def _assert_bitwise(a, b):
    assert a[0] == b[0]  # the losses
    for da, db in zip(a[1:], b[1:]):
        assert sorted(da) == sorted(db)
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"n{s[0]}_d{s[1]}_h{s[2]}")
def test_one_step_gradients_and_losses(shape):
    ref = _reference(shape)
    x = ref["batch"][0]
    zero = C.zero_planes(x)
    assert set(C.ZERO_PLANES) <= set(zero) and (shape[0] > 1 or set(range(84)) <= set(zero))
    assert x[..., 116].max() >= 100 and np.all(x[0, :, :, :84] == 0)  # a large move counter; a game's first plies
    tr = _trainer(shape, ref)
    losses = tr.step(*ref["batch"], **HYPER)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    dev = tr.read_all(az.TRAIN_GRAD)
    # the same step without the L2 term, for the zero input channels below
    tr.set_weights(ref["weights"].items())
    tr.reset_momentum()
    tr.step(*ref["batch"], **dict(HYPER, l2=0.0))
    stem_no_l2 = tr.read("stem.kernel", az.TRAIN_GRAD)
    tr.close()
    assert sorted(dev) == sorted(g64)
    for i, name in enumerate(("total", "policy", "value")):
        l64, l32 = ref["f64"][0]["losses"][i], ref["f32"][0]["losses"][i]
        err = abs(losses[i] - l64) / abs(l64)
        print(f"loss {name} {shape}: device error {err:.3e} (e32 {abs(l32 - l64) / abs(l64):.3e})")
        assert err <= C.tolerance(abs(l32 - l64) / abs(l64)), (name, losses[i], l64)
    # conv biases in front of a BN: true gradient 0
    for k in g64:
        unit = C.conv_bias_unit(k)
        if unit is not None:
            assert np.linalg.norm(dev[k]) <= 1e-4 * np.linalg.norm(g64[unit + ".gamma"]), k
    # input channels that are zero over the batch: no data gradient at all
    assert np.all(stem_no_l2[:, :, zero, :] == 0.0)
    l2_term = (np.float32(2.0) * np.float32(HYPER["l2"])) * ref["weights"]["stem.kernel"][:, :, zero, :]
    assert np.array_equal(dev["stem.kernel"][:, :, zero, :], l2_term)
    live = [c for c in range(C.PLANES) if c not in zero]
    assert np.all(np.abs(stem_no_l2[:, :, live, :]).max(axis=(0, 1, 3)) > 0)
    _check_tensors(dev, g64, g32, "grad", shape)


def test_two_steps_momentum_moving_statistics_and_weights():
    shape = (5, 2, 256)
    ref = _reference(shape, steps=2)
    assert min(r["relu_margin"] for r in ref["f64"]) >= C.MIN_RELU_MARGIN
    tr = _trainer(shape, ref)
    for _ in range(2):
        tr.step(*ref["batch"], **HYPER)
    mom, w = tr.read_all(az.TRAIN_MOMENTUM), tr.read_all(az.TRAIN_WEIGHT)
    tr.close()
    r64, r32 = ref["f64"][1], ref["f32"][1]
    bias_free = lambda d: {k: v for k, v in d.items() if C.conv_bias_unit(k) is None}  # noqa: E731
    _check_tensors(mom, bias_free(r64["mom"]), r32["mom"], "momentum", shape)
    stats = {k: v for k, v in r64["w"].items() if not C.is_trainable(k)}  # Bessel factor with N = 5 * 64
    _check_tensors(w, stats, r32["w"], "w", shape)
    # weights: elementwise within one fp32 rounding of the weight plus the gradient tolerance on the update
    w0 = ref["weights"]
    for k, v64 in r64["w"].items():
        if not C.is_trainable(k) or C.conv_bias_unit(k) is not None:
            continue
        update = v64 - w0[k].astype(np.float64)
        tol = C.tolerance(C.rel_l2(r32["mom"][k], r64["mom"][k]))
        bound = np.spacing(np.abs(v64).astype(np.float32)).astype(np.float64) + tol * np.linalg.norm(update)
        assert np.all(np.abs(w[k].astype(np.float64) - v64) <= bound), k
    for k in r64["w"]:  # conv biases: a zero gradient leaves them where they were
        if C.conv_bias_unit(k) is not None:
            assert np.abs(w[k] - w0[k]).max() <= 1e-4 * HYPER["lr"] * 2 * np.linalg.norm(
                r64["grad"][C.conv_bias_unit(k) + ".gamma"]), k


def test_steps_are_bitwise_reproducible_and_isolated():
    """Equal inputs give equal bits on every tensor: between two trainers, whatever max_batch is,
    and after a larger batch went through the same trainer (stale split-K partials, padding, LDS)."""
    big = C.reference_run(9, 1, **HYPER)
    small = C.reference_run(3, 1, **HYPER)
    one = C.reference_run(1, 1, **HYPER)

    def run(ref, max_batch, steps=1, before=None):
        tr = az.ChessTrainer(max_batch=max_batch, depth=1)
        if before is not None:
            tr.set_weights(before["weights"].items())
            tr.step(*before["batch"], **HYPER)
            tr.reset_momentum()
        tr.set_weights(ref["weights"].items())
        losses = [tr.step(*ref["batch"], **HYPER) for _ in range(steps)]
        out = [losses] + _state(tr)
        tr.close()
        return out

    _assert_bitwise(run(big, 9, steps=2), run(big, 9, steps=2))
    _assert_bitwise(run(small, 3), run(small, 16))
    _assert_bitwise(run(one, 9, before=big), run(one, 9))


def test_trained_chess_model_infers_saves_and_loads(tmp_path, monkeypatch):
    import keras_ref
    from custom_alphazero.model.policy_value import PolicyValueModel
    monkeypatch.setattr(ConfigModel, "depth", 1)
    model = PolicyValueModel((8, 8, 118), 1880, seed=1)
    x, pi, z = C.make_batch(6, seed=3)
    h0 = model.content_hash
    moving0 = model.weights["stem.var"].cpu().numpy().copy()
    for _ in range(2):
        loss = model.train_on_batch(x, pi, z)
        assert np.isfinite(loss)
    assert isinstance(model.trainer(), az.ChessTrainer)
    w = dict(zip(model.weight_names, model.get_weights()))
    assert model.content_hash != h0 and not np.array_equal(w["stem.var"], moving0)
    # the chess engine's inference forward sees the trained weights and the updated moving statistics
    probs, value = model(x)
    rp, rv = keras_ref.forward(w, x, depth=1)
    assert np.abs(probs.numpy() - rp).max() < 1e-5 and np.abs(value.numpy()[:, 0] - rv).max() < 1e-5
    path = str(tmp_path / "ckpt")
    model.save_with_meta(path)
    other = PolicyValueModel((8, 8, 118), 1880, seed=2)
    other.load_with_meta(path)
    assert other.content_hash == model.content_hash


def test_chess_self_play_trains_and_plays_on(monkeypatch):
    """The wiring of the loop, self-play -> train() -> self-play; no numeric claim."""
    from custom_alphazero import self_play
    from custom_alphazero.config import ConfigGeneral, ConfigSelfPlay
    from custom_alphazero.model.policy_value import PolicyValueModel
    from custom_alphazero.model.tensorflow.train import scheduled_learning_rate, train
    monkeypatch.setattr(ConfigGeneral, "game", "chess")
    monkeypatch.setattr(ConfigModel, "depth", 1)
    monkeypatch.setattr(ConfigSelfPlay, "chess_max_plies", 12)
    monkeypatch.setattr(ConfigSelfPlay, "chess_concurrent_games", 4)
    model = PolicyValueModel((8, 8, 118), 1880, seed=5)
    states, policies, rewards, records = self_play.play_chess(model, 4, 700, sims=8)
    m = len(states)
    assert m == sum(r.length for r in records) > 8 and states.shape == (m, 8, 8, 118) and policies.shape == (m, 1880)
    before = model.content_hash
    loss = train(model, states, [policies, rewards], batch_size=8, epochs=1)
    steps = -(-m // 8)
    assert np.isfinite(loss)
    assert model.steps == steps and model.get_learning_rate() == scheduled_learning_rate(steps)
    assert model.content_hash != before
    states2, _p, _r, records2 = self_play.play_chess(model, 4, 700, sims=8)
    assert len(states2) == sum(r.length for r in records2) > 0 and np.all(np.isfinite(states2))


def test_argument_errors():
    spec = C.make_spec(1)
    weights = C.R.make_weights(spec)
    x, pi, z = C.make_batch(5)
    tr = az.ChessTrainer(max_batch=4, depth=1)
    assert (tr.height, tr.width, tr.action_space) == (8, 8, 1880) and tr.spec == spec
    with pytest.raises(az.AzError, match="error -3"):  # AZ_E_STATE: a step before set_weights
        tr.step(x[:4], pi[:4], z[:4], 1e-2)
    tr.set_weights(weights.items())
    with pytest.raises(az.AzError, match="error -1"):  # n = 0
        tr.step(x[:0], pi[:0], z[:0], 1e-2)
    with pytest.raises(az.AzError, match="error -1"):  # n > max_batch
        tr.step(x, pi, z, 1e-2)
    tr.close()
    # host-side refusals: nothing is launched
    with pytest.raises(az.AzError, match="error -1.*filters"):
        az.ChessTrainer(max_batch=4, filters=64, depth=1)
    for depth in (0, 17):
        with pytest.raises(az.AzError, match="error -1.*depth"):
            az.ChessTrainer(max_batch=4, depth=depth)
    for hidden in (0, 1025):
        with pytest.raises(az.AzError, match="error -1.*value_hidden"):
            az.ChessTrainer(max_batch=4, depth=1, value_hidden=hidden)
    assert 262144 * 64 * 128 >= 2 ** 31 > 262143 * 64 * 128
    with pytest.raises(az.AzError, match="error -1.*max_batch"):
        az.ChessTrainer(max_batch=262144, depth=1)  # the first max_batch * 64 * 128 >= 2^31
    with pytest.raises(az.AzError, match="error -1.*bn_epsilon"):
        az.ChessTrainer(max_batch=4, depth=1, bn_epsilon=0.0)
    # a Connect-N trainer refuses what it refused before
    with pytest.raises(az.AzError, match="error -1.*cells"):
        az.Trainer(12, 12, True, max_batch=4, depth=1)
    with pytest.raises(az.AzError, match="error -1.*filters"):
        az.Trainer(6, 7, True, max_batch=4, filters=64, depth=1)
    with pytest.raises(az.AzError, match="error -1.*max_batch"):
        az.Trainer(6, 7, True, max_batch=399458, depth=1)
    # and a model that is neither network, or was never constructed, gets no trainer
    from custom_alphazero.model.policy_value import PolicyValueModel
    hollow = PolicyValueModel.__new__(PolicyValueModel)
    hollow.input_dim, hollow.action_space, hollow._trainer = (8, 8, 118), 1880, None
    with pytest.raises(az.AzError, match="error -1.*no weights"):
        hollow.trainer()
    hollow.input_dim, hollow.action_space, hollow.weights = (8, 8, 118), 64, {}
    with pytest.raises(az.AzError, match="error -1.*action space 64"):
        hollow.trainer()
