"""The training step (az_trainer_*, csrc/az_train.hip) at the shapes and numeric
edges its ABI accepts, against the float64 restatement in tests/train_ref.py.

test_train_gpu.py pins four shapes, all with value_hidden = 256, Dirichlet
targets and fresh weights.  This module adds what az_trainer_create promises
beyond them: H > W, 9x9 and 11x11 (A = 81 and 121 action threads and LDS
entries in heads_kernel, the odd-HW tail of wgrad_mfma_kernel's cell pairs),
2x2 (every cell a border cell, a 32-row tile over eight boards), three board
parts with ragged row parts, value_hidden 1 / 300 / 1024, depth 8 and 16,
one-board batches, policy logits scaled until the 1e-7 inside the log carries
the gradient, targets with exact zeros, channels with zero variance, a
saturated value head, a bn_epsilon other than the default, state carried from
one step into the next, and the update's arithmetic against the device's own
gradient.

Tolerance: train_ref.tolerance, as in test_train_gpu.py (8 x e32, floor 1e-6,
cap 1e-4; e32 from the CPU's float32 run, never from the device).  Every parity
test first asserts its input condition on the CPU runs alone: every tensor's
e32 <= train_ref.KINK_FREE and the first step's ReLU margin >= 0.95 x
CLEAR_MARGIN.

Worst device error measured on an MI355X (relative L2 over every gradient
tensor, one step), the tensor closest to its bound, and the losses' errors
(total / policy / value).  6x7 and depth 1 unless said otherwise:
  7x6, n 3                 9.5e-7   stem.beta 8.5e-7 of 6.2e-6           4.0e-8 / 7.3e-8 / 3.7e-8
  9x9, n 2                 9.6e-7   policy.conv.gamma 2.8e-7 of 2.2e-6   8.0e-8 / 6.2e-8 / 2.6e-8
  9x9 without gravity, n 3 1.4e-6   value.conv.beta 8.1e-7 of 1.0e-6     3.2e-8 / 3.4e-9 / 1.4e-7
  11x11 w/o gravity, n 2   8.2e-7   policy.conv.gamma 1.4e-7 of 1.1e-6   1.3e-8 / 2.3e-8 / 2.7e-7
  2x2, n 9                 6.5e-7   value.conv.gamma 3.3e-7 of 1.9e-6    4.2e-8 / 3.6e-8 / 6.1e-8
  4x5, n 17                7.7e-7   stem.kernel 6.9e-7 of 6.3e-6         1.7e-8 / 2.1e-8 / 7.6e-9
  n 4, hidden 1            8.8e-7   stem.beta 8.8e-7 of 8.6e-6           7.4e-8 / 1.6e-8 / 2.9e-8
  n 4, hidden 300          8.5e-7   stem.beta 8.5e-7 of 7.2e-6           1.1e-8 / 1.6e-8 / 3.9e-9
  n 4, hidden 1024         8.2e-7   value.dense2.bias 3.4e-7 of 2.8e-6   1.7e-8 / 1.6e-8 / 2.3e-8
  n 4, depth 8             3.2e-6   policy.conv.gamma 1.9e-6 of 1.2e-5   2.5e-7 / 3.6e-7 / 3.5e-7
  n 1                      8.6e-7   policy.conv.gamma 4.1e-7 of 1.0e-6   7.8e-8 / 5.7e-8 / 5.7e-9
  9x9, n 1, depth 2        1.3e-6   policy.conv.beta 5.8e-7 of 2.5e-6    3.8e-8 / 3.2e-8 / 5.3e-7
  5x5 w/o gravity, n 1     8.7e-7   value.conv.gamma 4.0e-7 of 1.0e-6    1.8e-9 / 1.7e-8 / 3.3e-7
  n 8, depth 16            (losses only)                                 1.1e-6 / 2.9e-8 / 4.6e-6
  n 5, policy.dense x4     9.7e-7   block0.conv1.beta 8.3e-7 of 1.0e-5   1.8e-7 / 2.1e-7 / 8.5e-8
  n 5, policy.dense x8     1.3e-6   value.conv.gamma 3.2e-7 of 4.1e-6    1.4e-7 / 2.1e-7 / 8.5e-8
  n 5, sparse targets      8.1e-7   policy.conv.gamma 3.3e-7 of 1.0e-6   7.9e-8 / 5.9e-8 / 8.5e-8
  n 5, dead channels       8.9e-7   policy.conv.gamma 3.4e-7 of 1.4e-6   2.8e-8 / 2.5e-8 / 6.4e-8
                           (moving statistics 4.0e-7, the dead channels' variance 4.2e-8)
  n 5, saturated value     1.2e-6   policy.conv.gamma 4.3e-7 of 1.0e-6   8.3e-8 / 7.5e-8 / 1.4e-7
  n 5, bn_epsilon 1e-5     8.4e-7   stem.beta 7.6e-7 of 6.2e-6           2.6e-8 / 2.1e-8 / 3.4e-8
  train() on 4, 4, 1       loss 5.0e-8 (e32 1.0e-7)
  l2 = 0.5 against l2 = 0  the total moves by 0.5 sum ||W||^2 within 1.4e-8
Every tensor above a third of its bound sits at the bound's floor of 1e-6 (its
e32 is below 1.25e-7: the CPU's float32 run happens to land within a rounding
or two of float64) and is a head conv's gamma or beta: one or two scalars,
each a sum over the n*H*W rows of terms of both signs.  The closest is
value.conv.beta at 9x9 without gravity, 8.1e-7 of 1.0e-6: its 243 terms
cancel 33-fold (sum |t| / |sum t|, float64), so 8.1e-7 of the sum is 2.4e-8
of the terms, less than one float32 rounding (6e-8).  The others (policy.conv.gamma
at n 1, with sparse targets and with the saturated value head, value.conv.gamma
at 5x5 n 1: 3.3e-7..4.3e-7 of 1.0e-6) cancel 2- to 6-fold and are one or two
roundings of their terms.

Once, on a scratch build: with heads_kernel's dlogit replaced by (p - pi) / n
both cases of test_softmax_backward_keeps_the_epsilon_in_the_log fail, the
device's stem.kernel 3.09e-2 (x4) and 3.09e-1 (x8) from float64, the figures the
test's own float64 shortcut gradient predicts.
"""
import numpy as np
import pytest
import torch

import train_ref as R
from custom_alphazero import engine as az
from custom_alphazero.config import ConfigModel

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, momentum=0.9, l2=1e-4, bn_momentum=0.99)


def _reference(shape, hidden=256, weights_mod=None, batch_mod=None, gradients=True, eps=1e-3):
    """The shared CPU runs of one step, after the condition on the inputs."""
    ref = R.reference_run(*shape, steps=1, hidden=hidden, weights_mod=weights_mod, batch_mod=batch_mod, eps=eps,
                          **HYPER)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    if gradients:
        for k in g64:
            if R.conv_bias_unit(k) is None:
                assert R.rel_l2(g32[k], g64[k]) <= R.KINK_FREE, (shape, k)
    assert ref["f64"][0]["relu_margin"] >= 0.95 * R.CLEAR_MARGIN, shape
    return ref


def _trainer(shape, weights, hidden=256, max_batch=None, eps=1e-3):
    H, W, gravity, n, depth = shape
    tr = az.Trainer(H, W, gravity, max_batch=max_batch or n, depth=depth, value_hidden=hidden, bn_epsilon=eps)
    tr.set_weights(weights.items())
    return tr


def _check_tensors(dev, ref64, ref32, what, shape):
    """Every tensor of ref64 (conv biases only among the weights) within train_ref.tolerance of its e32."""
    report = []
    for k, r64 in ref64.items():
        if R.conv_bias_unit(k) is not None and what != "w":
            continue
        report.append((R.rel_l2(dev[k], r64), R.tolerance(R.rel_l2(ref32[k], r64)), k))
    worst = max(r[0] for r in report)
    err, tol, k = max(report, key=lambda r: r[0] / r[1])
    print(f"{what} {shape}: worst device error {worst:.3e}; closest to its bound: {k} {err:.3e} of {tol:.3e}")
    bad = [(k, err, tol) for err, tol, k in report if not err <= tol]
    assert not bad, (what, shape, bad[:8])


def _check_losses(losses, ref, shape):
    for i, name in enumerate(("total", "policy", "value")):
        l64, l32 = ref["f64"][0]["losses"][i], ref["f32"][0]["losses"][i]
        err, e32 = abs(losses[i] - l64) / abs(l64), abs(l32 - l64) / abs(l64)
        print(f"loss {name} {shape}: device error {err:.3e} (e32 {e32:.3e})")
        assert err <= R.tolerance(e32), (name, losses[i], l64)


def _one_step(shape, hidden=256, weights_mod=None, batch_mod=None, tag="", eps=1e-3):
    """One step on the device against the reference: the checks of
    test_train_gpu.test_one_step_gradients_and_losses.  `eps` is the reference's
    and the trainer's bn_epsilon.  Returns (ref, the device's weights after the
    step)."""
    ref = _reference(shape, hidden, weights_mod, batch_mod, eps=eps)
    tr = _trainer(shape, ref["weights"], hidden, eps=eps)
    losses = tr.step(*ref["batch"], **HYPER)
    dev, w1 = tr.read_all(az.TRAIN_GRAD), tr.read_all(az.TRAIN_WEIGHT)
    tr.close()
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    what = (shape, hidden, tag)
    assert sorted(dev) == sorted(g64)
    _check_losses(losses, ref, what)
    for k in g64:  # conv biases in front of a BN: true gradient 0
        unit = R.conv_bias_unit(k)
        if unit is not None:
            assert np.linalg.norm(dev[k]) <= 1e-4 * np.linalg.norm(g64[unit + ".gamma"]), k
    _check_tensors(dev, g64, g32, "grad", what)
    return ref, w1


# ---------------------------------------------------------------- 1. edge shapes
# (H, W, gravity, n, depth), value_hidden
EDGE_SHAPES = [
    ((7, 6, True, 3, 1), 256),     # H > W: a swapped W in the tap masks, the tap offsets or Flatten
    ((9, 9, True, 2, 1), 256),     # HW = 81 (odd: the cell pairs' tail), 162 rows
    ((9, 9, False, 3, 1), 256),    # A = 81
    ((11, 11, False, 2, 1), 256),  # HW = A = 121, seven under the cap of 128
    ((2, 2, True, 9, 1), 256),     # every cell a border cell; 36 rows, two board parts (8 + 1)
    ((4, 5, True, 17, 1), 256),    # three board parts (8 + 8 + 1), 340 rows = five row parts and 20 rows
    ((6, 7, True, 4, 1), 1),       # dense_wgrad with J = 1 twice
    ((6, 7, True, 4, 1), 300),     # the hidden loops' tail (256 + 44)
    ((6, 7, True, 4, 1), 1024),    # the bound of heads_kernel's LDS arrays
    ((6, 7, True, 4, 8), 256),     # depth 8
    ((6, 7, True, 1, 1), 256),     # one board: 42 rows of batch statistics
    ((9, 9, True, 1, 2), 256),     # one board, odd HW, depth 2
    ((5, 5, False, 1, 1), 256),    # one board without gravity
]


def _shape_id(case):
    (H, W, gravity, n, depth), hidden = case
    return f"{H}x{W}{'' if gravity else '_nogravity'}_n{n}_d{depth}_h{hidden}"


@pytest.mark.parametrize("case", EDGE_SHAPES, ids=_shape_id)
def test_one_step_at_the_edge_shapes(case):
    shape, hidden = case
    _one_step(shape, hidden)


def test_depth_16_losses():
    """The ABI's deepest tower, 6x7 at n = 8.  Only the three losses are compared
    (e32 3.1e-6): thirty-three BatchNormalizations deep, the gradient is
    ill-conditioned in float32 -- the CPU's own float32 run is 7e-3..2e-2 from
    float64 at n = 8 and 16 -- so e32 gives no bound a correct kernel must
    meet, and the gradients are only required to be finite."""
    shape = (6, 7, True, 8, 16)
    ref = _reference(shape, gradients=False)
    tr = _trainer(shape, ref["weights"])
    losses = tr.step(*ref["batch"], **HYPER)
    dev = tr.read_all(az.TRAIN_GRAD)
    tr.close()
    _check_losses(losses, ref, shape)
    assert sorted(dev) == sorted(ref["f64"][0]["grad"])
    for k, g in dev.items():
        assert np.all(np.isfinite(g)), k


# ---------------------------------------------------------------- 2. the 1e-7 inside the log
def _scale_policy_dense_4(w):
    w["policy.dense.kernel"] *= 4
    return w


def _scale_policy_dense_8(w):
    w["policy.dense.kernel"] *= 8
    return w


def _shortcut_gradient(ref, depth, names):
    """Float64 gradient of the loss with the 1e-7 left out of the log, whose
    softmax backward is (p - pi) / n: what a kernel taking that shortcut computes."""
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in ref["weights"].items()}
    for k in w:
        if R.is_trainable(k):
            w[k].requires_grad_(True)
    x, pi, z = (torch.tensor(a, dtype=torch.float64) for a in ref["batch"])
    probs, values, _ = R.forward_train(w, x, depth)
    total, lp, _ = R.loss_terms(w, probs, values, pi, z, HYPER["l2"])
    total = total - lp + (-(pi * torch.log(probs)).sum(dim=1)).mean()
    grads = torch.autograd.grad(total, [w[k] for k in names])
    return {k: g.numpy() for k, g in zip(names, grads)}, float(probs.detach().min())


@pytest.mark.parametrize("mod", [_scale_policy_dense_4, _scale_policy_dense_8], ids=["x4", "x8"])
def test_softmax_backward_keeps_the_epsilon_in_the_log(mod):
    """policy.dense.kernel x4 and x8: the smallest probability falls to 2.4e-7
    and 1.3e-13, where p + 1e-7 is no longer p.  The gradient of the loss
    without the epsilon (dlogit = (p - pi) / n) is 2.8e-2 and 3.6e-1 from the
    true one on policy.dense.bias, asserted here at 100 tolerances at least,
    so a heads_kernel that took the shortcut fails the per-tensor check."""
    shape = (6, 7, True, 5, 1)
    ref = _reference(shape, weights_mod=mod)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    short, pmin = _shortcut_gradient(ref, shape[4], ["policy.dense.bias", "stem.kernel"])
    for k in short:
        print(f"{mod.__name__} min p {pmin:.2e}: shortcut gradient of {k} is {R.rel_l2(short[k], g64[k]):.2e} away")
    k = "policy.dense.bias"
    assert R.rel_l2(short[k], g64[k]) >= 100 * R.tolerance(R.rel_l2(g32[k], g64[k]))
    _one_step(shape, weights_mod=mod, tag=mod.__name__)


# ---------------------------------------------------------------- 3. sparse targets, dead channels, saturation
def _sparse_targets(batch):
    """Targets as MCTS writes them: even rows one-hot, odd rows 0.5 / 0.25 / 0.25, exact zeros elsewhere."""
    x, pi, z = batch
    A = pi.shape[1]
    pi[:] = 0.0
    for b in range(len(pi)):
        if b % 2 == 0:
            pi[b, (2 * b + 1) % A] = 1.0
        else:
            pi[b, [b % A, (b + 2) % A, (b + 4) % A]] = [0.5, 0.25, 0.25]
    return x, pi, z


DEAD = {"stem": 5, "block0.conv1": 7, "block0.res": 9}  # unit: the output channel whose kernel is zero


def _dead_channels(w):
    for unit, c in DEAD.items():
        w[unit + ".kernel"][..., c] = 0.0
    return w


def _saturate_value_head(w):
    w["value.dense2.kernel"] *= 10
    return w


def test_targets_with_exact_zeros():
    ref, _ = _one_step((6, 7, True, 5, 1), batch_mod=_sparse_targets, tag="sparse targets")
    pi = ref["batch"][1]
    assert np.count_nonzero(pi[0]) == 1 and np.count_nonzero(pi[1]) == 3 and np.all(pi.sum(axis=1) == 1.0)


def test_channels_with_zero_variance():
    """A zero conv kernel leaves y = bias on every row: sigma^2 = 0, invstd =
    1/sqrt(eps), yhat = 0.  The gradients go through the usual check; the
    moving variance of those channels must move toward 0 by the moving-average
    rule alone, m x var (float64: asserted on the reference), which the
    device's read-back is held to like every other statistic."""
    shape = (6, 7, True, 5, 1)
    ref, w1 = _one_step(shape, weights_mod=_dead_channels, tag="dead channels")
    r64, r32, w0 = ref["f64"][0]["w"], ref["f32"][0]["w"], ref["weights"]
    stats = {k: v for k, v in r64.items() if not R.is_trainable(k)}
    _check_tensors(w1, stats, r32, "w", (shape, "dead channels"))
    pick = lambda d: {u + ".var": np.asarray(d[u + ".var"])[[c]] for u, c in DEAD.items()}  # noqa: E731
    for k, v in pick(r64).items():
        assert abs(v[0] - HYPER["bn_momentum"] * float(pick(w0)[k][0])) <= 1e-12 * v[0], k
        assert 0 < v[0] < float(pick(w0)[k][0])
    _check_tensors(pick(w1), pick(r64), pick(r32), "w", (shape, "dead channels' moving variance"))


def test_saturated_value_head():
    """value.dense2.kernel x10: |v| reaches 0.998 and the factor 1 - v^2 of the
    value head's backward falls to 4e-3.  (Not above x16: at x24 the CPU's own
    float32 run leaves float64 by 1.6e-5 and the input condition fails.)"""
    shape = (6, 7, True, 5, 1)
    ref, _ = _one_step(shape, weights_mod=_saturate_value_head, tag="saturated value head")
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in ref["weights"].items()}
    with torch.no_grad():
        _, v, _ = R.forward_train(w, torch.tensor(ref["batch"][0], dtype=torch.float64), shape[4])
    print(f"saturated value head: max |v| {float(v.abs().max()):.4f}")
    assert float(v.abs().max()) >= 0.99


def test_bn_epsilon_reaches_the_kernels():
    """bn_epsilon = 1e-5 (every other test of this trainer runs the default,
    1e-3).  On the CPU alone, the float64 gradient on the same weights and batch
    with eps = 1e-3 is 6.4e-4 (value.dense2.bias) to 2.1e-1 (value.conv.beta)
    from the eps = 1e-5 gradient, 640 tolerances at least: a trainer that
    ignored the field fails on every tensor; one at 100 tolerances is asserted."""
    shape, eps = (6, 7, True, 5, 1), 1e-5
    ref = _reference(shape, eps=eps)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    other = R.RefTrainer(ref["spec"], ref["weights"], shape[4], torch.float64, eps=1e-3)
    other.step(*ref["batch"], **HYPER)
    ratio = {k: R.rel_l2(other.grad[k].numpy(), g64[k]) / R.tolerance(R.rel_l2(g32[k], g64[k]))
             for k in g64 if R.conv_bias_unit(k) is None}
    print(f"bn_epsilon 1e-5: the eps = 1e-3 gradient is {min(ratio.values()):.0f} to {max(ratio.values()):.0f} "
          "tolerances away")
    assert max(ratio.values()) >= 100
    _one_step(shape, tag="bn_epsilon 1e-5", eps=eps)


# ---------------------------------------------------------------- 4. no state leaks between steps
def _snapshot(tr):
    return [tr.read_all(what) for what in (az.TRAIN_GRAD, az.TRAIN_MOMENTUM, az.TRAIN_WEIGHT)]


def _same_bytes(a, b):
    assert sorted(a) == sorted(b)
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("board", [(6, 7, True, 2), (5, 5, False, 1)], ids=["6x7_d2", "5x5_nogravity_d1"])
def test_a_step_depends_on_its_own_state_and_batch_only(board):
    """Bitwise.  A trainer that has stepped on 9 other boards from other weights
    and then gets A's weights, a zeroed momentum and A's 5-board batch must
    leave A's losses, gradients, momentum and weights: nothing of the earlier
    step -- partial sums, per-board scratch, rows 5..8 of every activation,
    the conv biases' gradient entries -- may reach the later one."""
    H, W, gravity, depth = board
    spec = R.make_spec(H, W, gravity, depth)
    W1, W2 = R.make_weights(spec, seed=0), R.make_weights(spec, seed=1)
    X = R.make_batch(H, W, gravity, 5, seed=0)
    Y = R.make_batch(H, W, gravity, 9, seed=7)
    shape = (H, W, gravity, 9, depth)
    a = _trainer(shape, W1)
    losses_a = a.step(*X, **HYPER)
    snap_a = _snapshot(a)
    a.close()
    b = _trainer(shape, W2)
    b.step(*Y, **HYPER)
    b.set_weights(W1.items())  # momentum is left as it is: the step differs from A's
    b.step(*X, **HYPER)
    assert not _same_bytes(b.read_all(az.TRAIN_MOMENTUM), snap_a[1])
    b.set_weights(W1.items())
    b.reset_momentum()
    losses_b = b.step(*X, **HYPER)
    snap_b = _snapshot(b)
    b.close()
    assert losses_a == losses_b
    for da, db in zip(snap_a, snap_b):
        assert sorted(da) == sorted(db)
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), k
    for snap in (snap_a, snap_b):
        for k, g in snap[0].items():
            if R.conv_bias_unit(k) is not None:
                assert not g.any(), k


# ---------------------------------------------------------------- 5. the update against the device's own gradient
def test_first_update_is_exact():
    """First step after set_weights (zero momentum): a = -(lr * g), w = w0 + a in
    float32, the same with or without a fused multiply-add, so bitwise.  g is
    the device's own gradient, L2 term included."""
    shape = (6, 7, True, 5, 1)
    w0 = R.make_weights(R.make_spec(*shape[:3], shape[4]), seed=0)
    tr = _trainer(shape, w0)
    tr.step(*R.make_batch(*shape[:4], seed=0), **HYPER)
    g, m, w1 = _snapshot(tr)
    tr.close()
    lr = np.float32(HYPER["lr"])
    for k in g:
        a = -(lr * g[k])
        assert a.dtype == np.float32
        assert np.array_equal(m[k], a), k
        assert np.array_equal(w1[k], w0[k].reshape(a.shape) + a), k
    for k in w1:  # the moving statistics are no part of this update but do move
        if not R.is_trainable(k):
            assert not np.array_equal(w1[k], w0[k].reshape(w1[k].shape)), k


def test_l2_reaches_the_kernels_and_nothing_else():
    """The same state and batch at l2 = 0 and l2 = 0.5.  The step adds
    2 * l2 * w = w to a .kernel tensor's gradient in one float32 operation, so
    the two gradients differ by w within half an ulp of the sum, which is at
    most one ulp of the larger of |w| and |g|; every other tensor's gradient,
    and the policy and value losses, are the same bits."""
    shape = (6, 7, True, 5, 1)
    w0 = R.make_weights(R.make_spec(*shape[:3], shape[4]), seed=0)
    batch = R.make_batch(*shape[:4], seed=0)
    runs = []
    for l2 in (0.0, 0.5):
        tr = _trainer(shape, w0)
        losses = tr.step(*batch, **dict(HYPER, l2=l2))
        runs.append((losses, tr.read_all(az.TRAIN_GRAD)))
        tr.close()
    (l_0, g_0), (l_5, g_5) = runs
    assert any(k.endswith(".kernel") for k in g_0) and any(not k.endswith(".kernel") for k in g_0)
    for k in g_0:
        if not k.endswith(".kernel"):
            assert g_0[k].tobytes() == g_5[k].tobytes(), k
            continue
        w = w0[k].reshape(g_0[k].shape)
        diff = g_5[k].astype(np.float64) - g_0[k].astype(np.float64)
        bound = np.spacing(np.maximum(np.abs(w), np.abs(g_0[k]))).astype(np.float64)
        assert np.all(np.abs(diff - w.astype(np.float64)) <= bound), k
    assert l_0[1:] == l_5[1:]
    sq = sum(float((w0[k].astype(np.float64) ** 2).sum()) for k in w0 if k.endswith(".kernel"))
    err = abs((l_5[0] - l_0[0]) - 0.5 * sq) / (0.5 * sq)
    print(f"l2 = 0.5: total loss moved by {l_5[0] - l_0[0]:.6f}, 0.5 * sum ||W||^2 = {0.5 * sq:.6f} (error {err:.3e})")
    assert err <= R.tolerance(0)


# ---------------------------------------------------------------- 6. a ragged last batch of one
def _fit(spec, weights, depth, x, pi, z, batch_size, dtype):
    """One epoch of the reference's model.fit(shuffle=False) with the
    restatement's step: (loss as Keras reports it, smallest ReLU margin)."""
    ref = R.RefTrainer(spec, weights, depth, dtype)
    weighted, margin = 0.0, np.inf
    for lo in range(0, len(x), batch_size):
        hi = min(len(x), lo + batch_size)
        total, _, _ = ref.step(x[lo:hi], pi[lo:hi], z[lo:hi], ConfigModel.maximum_learning_rate,
                               ConfigModel.momentum, ConfigModel.l2_penalization_term, ConfigModel.bn_momentum)
        weighted += total * (hi - lo)
        margin = min(margin, ref.relu_margin)
    return weighted / len(x), margin


def test_train_takes_a_last_batch_of_one():
    """train(): 9 samples, batch_size 4, one epoch = steps on 4, 4 and 1 samples,
    as the reference's model.fit takes them."""
    from custom_alphazero.model.policy_value import PolicyValueModel
    from custom_alphazero.model.tensorflow.train import train
    model = PolicyValueModel((6, 7, 4), 7, seed=0)
    x, pi, z = R.make_batch(6, 7, True, 9, seed=R.BATCH_SEEDS[(6, 7, True, 9, 4)])
    weights = dict(zip(model.weight_names, model.get_weights()))
    l64, margin = _fit(model.spec, weights, model.depth, x, pi, z, 4, torch.float64)
    l32, _ = _fit(model.spec, weights, model.depth, x, pi, z, 4, torch.float32)
    assert margin >= R.MIN_RELU_MARGIN, margin
    before = model.content_hash
    loss = train(model, x, [pi, z], batch_size=4, epochs=1)
    err, e32 = abs(loss - l64) / l64, abs(l32 - l64) / l64
    print(f"train() on 4, 4, 1: device error {err:.3e} (e32 {e32:.3e}, ReLU margin {margin:.2e})")
    assert err <= R.tolerance(e32), (loss, l64)
    assert model.steps == 3 and model.content_hash != before
