"""The training step on the device (az_trainer_*, csrc/az_train.hip) against
the float64 torch restatement in tests/train_ref.py.

Tolerance, per tensor: e32 = the relative L2 error of the restatement's own
float32 CPU run against float64; the device must be within
max(8 * e32, 1e-6) and never looser than 1e-4 (train_ref.tolerance).  Each
test first asserts e32 <= 1.25e-5 for every tensor, which makes its input
kink-free: a ReLU whose input sits within rounding of zero flips between
precisions, and one flip moves that gradient by about 1e-3 of its norm.
At 64 boards and depth 4 a step has 4.5 million ReLU inputs and some always
lie within 3e-6 of zero, where fp32 runs of another summation order do flip
them (the device flipped one at 2.66e-6 that the CPU's float32 run kept), so
the inputs are kink-free by construction: train_ref.clear_kinks moves the
per-channel offsets in front of the ReLUs, on the float64 run alone, until
every ReLU input of the first step is 2e-5 from zero (asserted), and the
steps after it must keep 1e-6 (train_ref.BATCH_SEEDS: the seeds that do).  The bias of a conv in front of a training-mode BN has a
true gradient of 0: the device's must stay below 1e-4 of the norm of that
unit's gamma gradient.

Worst device error measured on an MI355X, relative L2 over every tensor
(gradient of the total loss, one step), and the losses' (total / policy /
value):
  6x7, n 3, depth 1              9.0e-7    1.1e-8 / 4.2e-8 / 1.2e-7
  5x5 without gravity, n 5, d 2  4.2e-6    7.8e-8 / 9.7e-9 / 2.3e-7
  6x7, n 37, depth 2             1.1e-6    5.2e-8 / 4.6e-9 / 7.2e-8
                                 (two steps: momentum 8.5e-7, moving statistics 2.6e-7)
  6x7, n 64, depth 4             1.8e-6    2.9e-8 / 2.4e-8 / 1.1e-7
Every tensor is at most a third of its bound (5x5: value.conv.gamma, 4.2e-6 of
1.3e-5).  The tightest bound is value.conv.beta's at 64 boards, one scalar (a
sum of 2688 terms of both signs) that the CPU's float32 run happens to hit
within 1.6e-7: 1.26e-6.  With one fp32 MFMA chain over the forward convs'
whole K the device missed it at 1.50e-6; with the chains cut to 32 channels
and added in float64 (conv_mfma_kernel) it is 1.6e-7.  The five-step loss
trajectory stays within 8.2e-8.
"""
import numpy as np
import pytest

import keras_ref
import train_ref as R
from custom_alphazero import engine as az
from custom_alphazero.config import ConfigModel

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, momentum=0.9, l2=1e-4, bn_momentum=0.99)
# (H, W, gravity, n, depth): 126 rows (less than a 32-row tile multiple); odd HW with A = 25; 1554 rows
# (several split-K parts, ragged tails); the configured depth
SHAPES = [(6, 7, True, 3, 1), (5, 5, False, 5, 2), (6, 7, True, 37, 2), (6, 7, True, 64, 4)]


def _reference(shape, steps=1, gradient_steps=None):
    """The shared CPU runs, after the condition on the inputs: no ReLU kinks in
    the steps whose gradients (or what follows from them) a test compares."""
    H, W, gravity, n, depth = shape
    ref = R.reference_run(H, W, gravity, n, depth, steps=steps, **HYPER)
    for s in range(steps if gradient_steps is None else gradient_steps):
        g64, g32 = ref["f64"][s]["grad"], ref["f32"][s]["grad"]
        for k in g64:
            if R.conv_bias_unit(k) is None:
                assert R.rel_l2(g32[k], g64[k]) <= R.KINK_FREE, (shape, s, k)
        if s == 0:  # train_ref.clear_kinks built the weights for this (less their rounding to float32)
            assert ref["f64"][s]["relu_margin"] >= 0.95 * R.CLEAR_MARGIN, (shape, s)
        elif gradient_steps is None:
            assert ref["f64"][s]["relu_margin"] >= R.MIN_RELU_MARGIN, (shape, s)
    return ref


def _trainer(shape, ref, max_batch=None):
    H, W, gravity, n, depth = shape
    tr = az.Trainer(H, W, gravity, max_batch=max_batch or n, depth=depth)
    tr.set_weights(ref["weights"].items())
    return tr


def _check_tensors(dev, ref64, ref32, what, shape, report):
    worst = 0.0
    for k, r64 in ref64.items():
        unit = R.conv_bias_unit(k)
        if unit is not None and what != "w":
            continue
        e32 = R.rel_l2(ref32[k], r64)
        err = R.rel_l2(dev[k], r64)
        worst = max(worst, err)
        report.append((err, R.tolerance(e32), k))
    err, tol, k = max(report, key=lambda r: r[0] / r[1])
    print(f"{what} {shape}: worst device error {worst:.3e}; closest to its bound: {k} {err:.3e} of {tol:.3e}")
    bad = [(k, err, tol) for err, tol, k in report if not err <= tol]
    assert not bad, (what, shape, bad[:8])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_n{s[3]}_d{s[4]}")
def test_one_step_gradients_and_losses(shape):
    ref = _reference(shape)
    tr = _trainer(shape, ref)
    losses = tr.step(*ref["batch"], **HYPER)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    dev = tr.read_all(az.TRAIN_GRAD)
    tr.close()
    assert sorted(dev) == sorted(g64)
    for i, name in enumerate(("total", "policy", "value")):
        l64, l32 = ref["f64"][0]["losses"][i], ref["f32"][0]["losses"][i]
        err = abs(losses[i] - l64) / abs(l64)
        print(f"loss {name} {shape}: device error {err:.3e} (e32 {abs(l32 - l64) / abs(l64):.3e})")
        assert err <= R.tolerance(abs(l32 - l64) / abs(l64)), (name, losses[i], l64)
    # conv biases in front of a BN: true gradient 0
    for k in g64:
        unit = R.conv_bias_unit(k)
        if unit is not None:
            assert np.linalg.norm(dev[k]) <= 1e-4 * np.linalg.norm(g64[unit + ".gamma"]), k
    _check_tensors(dev, g64, g32, "grad", shape, [])


def test_two_steps_momentum_moving_statistics_and_weights():
    shape = (6, 7, True, 37, 2)
    ref = _reference(shape, steps=2)
    tr = _trainer(shape, ref)
    for _ in range(2):
        tr.step(*ref["batch"], **HYPER)
    mom, w = tr.read_all(az.TRAIN_MOMENTUM), tr.read_all(az.TRAIN_WEIGHT)
    tr.close()
    r64, r32 = ref["f64"][1], ref["f32"][1]
    bias_free = lambda d: {k: v for k, v in d.items() if R.conv_bias_unit(k) is None}  # noqa: E731
    _check_tensors(mom, bias_free(r64["mom"]), r32["mom"], "momentum", shape, [])
    stats = {k: v for k, v in r64["w"].items() if not R.is_trainable(k)}
    _check_tensors(w, stats, r32["w"], "w", shape, [])
    # weights: elementwise within one fp32 rounding of the weight plus the gradient tolerance on the update
    w0 = ref["weights"]
    for k, v64 in r64["w"].items():
        if not R.is_trainable(k) or R.conv_bias_unit(k) is not None:
            continue
        update = v64 - w0[k].astype(np.float64)
        tol = R.tolerance(R.rel_l2(r32["mom"][k], r64["mom"][k]))
        bound = np.spacing(np.abs(v64).astype(np.float32)).astype(np.float64) + tol * np.linalg.norm(update)
        assert np.all(np.abs(w[k].astype(np.float64) - v64) <= bound), k
    for k in r64["w"]:  # conv biases: a zero gradient leaves them where they were
        if R.conv_bias_unit(k) is not None:
            assert np.abs(w[k] - w0[k]).max() <= 1e-4 * HYPER["lr"] * 2 * np.linalg.norm(
                r64["grad"][R.conv_bias_unit(k) + ".gamma"]), k


def test_two_trainers_are_bitwise_equal():
    shape = (6, 7, True, 37, 2)
    ref = R.reference_run(*shape, steps=2, **HYPER)
    runs = []
    for _ in range(2):
        tr = _trainer(shape, ref, max_batch=40)
        losses = [tr.step(*ref["batch"], **HYPER) for _ in range(2)]
        runs.append((losses, tr.read_all(az.TRAIN_WEIGHT), tr.read_all(az.TRAIN_GRAD), tr.read_all(az.TRAIN_MOMENTUM)))
        tr.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


def _fresh_model(seed=0):
    from custom_alphazero.model.policy_value import PolicyValueModel
    return PolicyValueModel((6, 7, 4), 7, seed=seed)


def _reference_fit(model, x, pi, z, batch_size, epochs, dtype):
    """The reference's model.fit(shuffle=False) with the restatement's step."""
    weights = dict(zip(model.weight_names, model.get_weights()))
    ref = R.RefTrainer(model.spec, weights, model.depth, dtype)
    n, loss = len(x), None
    for _ in range(epochs):
        weighted = 0.0
        for lo in range(0, n, batch_size):
            hi = min(n, lo + batch_size)
            total, _, _ = ref.step(x[lo:hi], pi[lo:hi], z[lo:hi], model.learning_rate, ConfigModel.momentum,
                                   ConfigModel.l2_penalization_term, ConfigModel.bn_momentum)
            weighted += total * (hi - lo)
        loss = weighted / n
    return loss


def test_train_follows_the_reference_loop():
    """train(): n = 10, batch_size = 4, 2 epochs = six steps on batches of 4, 4 and 2."""
    import torch
    from custom_alphazero.model.tensorflow.train import scheduled_learning_rate, train
    model = _fresh_model()
    x, pi, z = R.make_batch(6, 7, True, 10, seed=R.BATCH_SEEDS[(6, 7, True, 10, 4)])
    l64 = _reference_fit(model, x, pi, z, 4, 2, torch.float64)
    l32 = _reference_fit(model, x, pi, z, 4, 2, torch.float32)
    before = model.content_hash
    loss = train(model, x, [pi, z], batch_size=4, epochs=2)
    err, e32 = abs(loss - l64) / l64, abs(l32 - l64) / l64
    print(f"train() loss: device error {err:.3e} (e32 {e32:.3e})")
    assert err <= R.tolerance(e32), (loss, l64)
    assert model.steps == 6
    assert model.get_learning_rate() == scheduled_learning_rate(6) == 1e-2
    assert model.content_hash != before


def test_loss_follows_the_float64_trajectory_and_falls():
    """Thirty steps on one fixed 16-sample batch at lr 1e-2.  Only the total loss
    is compared, against its own float32 error: no 16-sample batch keeps every
    ReLU of five consecutive steps clear of zero (seeds 0..39: the float32 CPU
    run's gradients leave float64's by 1.8e-5 at the best), so the kink-free
    condition is asserted for the first step."""
    shape = (6, 7, True, 16, 4)
    ref = _reference(shape, steps=5, gradient_steps=1)
    tr = _trainer(shape, ref)
    losses = [tr.step(*ref["batch"], **HYPER)[0] for _ in range(30)]
    tr.close()
    for s in range(5):
        l64, l32 = ref["f64"][s]["losses"][0], ref["f32"][s]["losses"][0]
        err = abs(losses[s] - l64) / l64
        print(f"trajectory step {s}: device error {err:.3e} (e32 {abs(l32 - l64) / l64:.3e})")
        assert err <= R.tolerance(abs(l32 - l64) / l64), (s, losses[s], l64)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_trained_model_infers_saves_and_loads(tmp_path):
    from custom_alphazero.model.tensorflow.train import train
    model = _fresh_model(seed=1)
    x, pi, z = R.make_batch(6, 7, True, 8, seed=0)
    h0 = model.content_hash
    moving0 = {k: model.weights[k].cpu().numpy().copy() for k in ("stem.mean", "stem.var")}
    train(model, x, [pi, z], batch_size=8, epochs=2)
    w = dict(zip(model.weight_names, model.get_weights()))
    assert model.content_hash != h0
    assert not np.array_equal(w["stem.mean"], moving0["stem.mean"])  # the moving statistics moved
    assert not np.array_equal(w["stem.var"], moving0["stem.var"])
    # the inference engine sees the trained weights and the updated moving statistics
    probs, value = model(x)
    rp, rv = keras_ref.forward(w, x, depth=model.depth)
    assert np.abs(probs.numpy() - rp).max() < 1e-5 and np.abs(value.numpy()[:, 0] - rv).max() < 1e-5
    # and so does a checkpoint
    path = str(tmp_path / "ckpt")
    model.save_with_meta(path)
    other = _fresh_model(seed=2)
    other.load_with_meta(path)
    assert other.content_hash == model.content_hash and other.steps == model.steps == 2
    # set_weights pushes into an existing trainer: the next step starts from the loaded weights
    model.set_weights(_fresh_model(seed=3).get_weights())
    tr = model.trainer()
    assert np.array_equal(tr.read("stem.kernel"), dict(zip(model.weight_names, model.get_weights()))["stem.kernel"])


def test_argument_errors():
    spec = R.make_spec(6, 7, True, 1)
    weights = R.make_weights(spec)
    x, pi, z = R.make_batch(6, 7, True, 5)
    tr = az.Trainer(6, 7, True, max_batch=4, depth=1)
    with pytest.raises(az.AzError, match="error -3"):  # AZ_E_STATE: a step before set_weights
        tr.step(x[:4], pi[:4], z[:4], 1e-2)
    tr.set_weights(weights.items())
    with pytest.raises(az.AzError, match="error -1"):  # n = 0
        tr.step(x[:0], pi[:0], z[:0], 1e-2)
    with pytest.raises(az.AzError, match="error -1"):  # n > max_batch
        tr.step(x, pi, z, 1e-2)
    with pytest.raises(az.AzError, match="error -1.*unknown tensor"):
        tr.read("block9.conv1.kernel")
    with pytest.raises(az.AzError, match="error -1"):  # moving statistics have no gradient
        tr.read("stem.mean", az.TRAIN_GRAD)
    with pytest.raises(az.AzError, match="error -1"):  # one tensor short
        tr.set_weights(list(weights.items())[:-1])
    short = dict(weights, **{"stem.bias": weights["stem.bias"][:-1]})
    with pytest.raises(az.AzError, match="error -1.*numel"):
        tr.set_weights(short.items())
    tr.close()
    with pytest.raises(az.AzError, match="error -1.*filters"):
        az.Trainer(6, 7, True, max_batch=4, filters=64, depth=1)
    with pytest.raises(az.AzError, match="error -1.*depth"):
        az.Trainer(6, 7, True, max_batch=4, depth=17)
    # the refusals that guard heads_kernel's LDS arrays and the 32-bit row indices (host side, nothing is launched)
    with pytest.raises(az.AzError, match="error -1.*cells"):
        az.Trainer(12, 12, True, max_batch=4, depth=1)  # 144 cells
    with pytest.raises(az.AzError, match="error -1.*value_hidden"):
        az.Trainer(6, 7, True, max_batch=4, depth=1, value_hidden=1025)
    with pytest.raises(az.AzError, match="error -1.*value_hidden"):
        az.Trainer(6, 7, True, max_batch=4, depth=1, value_hidden=0)
    with pytest.raises(az.AzError, match="error -1.*depth"):
        az.Trainer(6, 7, True, max_batch=4, depth=0)
    assert 399458 * 6 * 7 * 128 >= 2 ** 31 > 399457 * 6 * 7 * 128
    with pytest.raises(az.AzError, match="error -1.*max_batch"):
        az.Trainer(6, 7, True, max_batch=399458, depth=1)  # the first max_batch * H * W * 128 >= 2^31
    # chess (118 planes, 1880 actions) is refused
    from custom_alphazero.model.policy_value import PolicyValueModel
    chess = PolicyValueModel.__new__(PolicyValueModel)
    chess.input_dim, chess.action_space, chess._trainer = (8, 8, 118), 1880, None
    with pytest.raises(az.AzError, match="error -1"):
        chess.trainer()
