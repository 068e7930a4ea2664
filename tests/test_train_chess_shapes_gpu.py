"""The chess network's training step (az_chess_trainer_create, csrc/az_train.hip
chess_stem_* / chess_heads_kernel / chess_policy_wgrad_kernel and the shared
kernels at HW = 64, A = 1880, cin = 118) at the shapes and numeric edges its
ABI accepts, against the float64 restatement (tests/train_chess_ref.py): the
chess counterpart of tests/test_train_shapes_gpu.py.

test_train_chess_gpu.py pins five shapes with fresh weights, bn_epsilon = 1e-3
and l2 = 1e-4.  This module adds: exactly one, exactly two and three parts of
kBoardsPerPart = 8 boards, value_hidden 1 / 300 / 1024, depth 4 and 16, policy
logits scaled until the 1e-7 inside the log carries the gradient, a saturated
value head, channels with zero variance, a bn_epsilon other than the default,
the update's arithmetic against the device's own gradient, l2 against l2 = 0
over the chess tensor layout, and a step at the part boundary after a larger
one.

Tolerance: train_ref.tolerance (8 x e32, floor 1e-6, cap 1e-4; e32 from the
CPU's float32 run, never from the device).  Every parity case first asserts its
input condition on the CPU runs alone (train_chess_ref.input_condition: every
tensor's e32 <= KINK_FREE, ReLU margin >= 0.95 x CLEAR_MARGIN);
tests/test_train_chess_cpu.py asserts the same without a GPU.  The inputs, and
the criteria that chose them, are train_chess_ref's.

Worst device error measured on an MI355X (relative L2 over every gradient
tensor, one step), the tensor closest to its bound (error of bound), and the
losses' errors (total / policy / value).  Depth 1 and value_hidden 256 unless
said otherwise:
  n 8                      1.1e-6   value.conv.beta 2.9e-7 of 1.0e-6     2.8e-8 / 1.3e-8 / 1.7e-8
  n 16                     1.4e-6   stem.beta 1.4e-6 of 1.2e-5           1.7e-8 / 1.2e-8 / 7.2e-8
  n 17                     1.4e-5   value.conv.beta 1.4e-5 of 2.3e-5     2.9e-9 / 1.1e-8 / 1.3e-7
  n 4, hidden 1            1.7e-6   value.dense2.bias 4.7e-7 of 1.2e-6   3.0e-8 / 2.2e-8 / 1.6e-7
  n 4, hidden 300          1.0e-6   policy.conv.gamma 6.1e-7 of 1.2e-6   5.3e-8 / 2.6e-8 / 2.0e-8
  n 4, hidden 1024         9.0e-7   stem.kernel 7.5e-7 of 6.5e-6         2.1e-8 / 2.4e-9 / 3.1e-8
  n 4, depth 4             1.7e-6   value.conv.gamma 6.6e-7 of 3.3e-6    2.9e-8 / 4.1e-10 / 3.3e-7
  n 8, depth 16            (losses only)                                 5.8e-7 / 3.8e-8 / 7.4e-6
  n 5, policy.dense x4     9.9e-7   value.conv.gamma 3.8e-7 of 1.7e-6    1.2e-8 / 1.9e-8 / 2.9e-7
  n 5, policy.dense x8     9.2e-7   value.conv.gamma 3.8e-7 of 1.7e-6    5.5e-9 / 9.2e-9 / 2.9e-7
  n 5, saturated value     3.0e-6   value.dense2.bias 1.4e-6 of 2.6e-6   9.5e-8 / 3.1e-8 / 7.9e-7
  n 5, dead channels       1.1e-6   value.conv.gamma 4.6e-7 of 1.3e-6    2.0e-8 / 3.2e-8 / 2.8e-7
                           (moving statistics 5.8e-8, the dead channels' variance 3.9e-8)
  n 5, bn_epsilon 1e-5     1.2e-6   value.conv.gamma 8.8e-7 of 3.5e-6    1.3e-8 / 1.9e-8 / 5.2e-7
  l2 = 0.5 against l2 = 0  the total moves by 0.5 sum ||W||^2 = 429.1 within 9.3e-9
The update, the l2 isolation and the part-boundary step are bitwise (one ulp
where the l2 test says so) and hold.
Every tensor above a third of its bound is one scalar: a head conv's gamma or
beta, or value.dense2.bias (the sum of the boards' dpre2).  The closest is
value.conv.beta at n 17, 1.4e-5 of 2.3e-5: its 1088 terms cancel 412-fold (sum
|t| / |sum t|, float64, train_chess_ref.head_cancellation), so 1.4e-5 of the
sum is 3.4e-8 of the terms, less than one float32 rounding (6e-8).
policy.conv.gamma at hidden 300 (6.1e-7 of 1.2e-6) cancels 115-fold.

Two cases stand at batch seed 3, not 0 (train_chess_ref.BATCH_SEEDS, chosen
on the float64 run alone as the seed whose head scalars cancel least).  At
seed 0 value.conv.gamma cancels 29-fold at depth 4 and 20-fold at hidden
1024, and its e32 depended on the CPU: 3.9e-6 and 2.1e-6 on one, 1.7e-5 (over
KINK_FREE: the input condition failed) and 3.9e-7 on another, against which
the device's 3.3e-6 at hidden 1024 (1.6e-7 of the terms; the first CPU's own
float32 run is 2.1e-6 .. 3.2e-6 off, depending on its thread count) missed
8 x e32 = 3.1e-6.  No kernel was changed.

Once, on scratch builds of chess_heads_kernel:
  dlogit replaced by (p - pi) / n: both cases of
    test_softmax_backward_keeps_the_epsilon_in_the_log fail, the device's
    stem.kernel 6.81e-3 (x4) and 3.14e-1 (x8) from float64, the figures the
    test's own float64 shortcut gradient predicts; worst tensor 1.6e-2 and
    4.5e-1 (policy.conv.gamma).
  the `last` tail of the logits dropped (actions 1792 + t get no weights):
    all seven cases of test_one_step_at_the_edge_shapes fail at the total
    loss already, 9.4e-5 (n 16) to 1.7e-3 (hidden 1024) from float64.
  the `lane + 64 * FULL < A` tail of the ghp dot dropped: the losses are
    untouched and all seven cases fail in the per-tensor check, every tensor
    below the heads 2e-3 .. 9e-3 from float64, worst 8.3e-3 (depth 4) to
    1.7e-1 (hidden 1), policy.conv.beta up to 1.3e-1 against bounds of 1e-6.
"""
import numpy as np
import pytest

import train_chess_ref as C
from custom_alphazero import engine as az

pytestmark = pytest.mark.gpu

HYPER = C.HYPER


def _trainer(shape, weights, max_batch=None, **more):
    n, depth, hidden = shape
    tr = az.ChessTrainer(max_batch=max_batch or n, depth=depth, value_hidden=hidden, **more)
    tr.set_weights(weights.items())
    return tr


def _check_tensors(dev, ref64, ref32, what, case):
    """Every tensor of ref64 (conv biases only among the weights) within train_ref.tolerance of its e32."""
    report = []
    for k, r64 in ref64.items():
        if C.conv_bias_unit(k) is not None and what != "w":
            continue
        report.append((C.rel_l2(dev[k], r64), C.tolerance(C.rel_l2(ref32[k], r64)), k))
    worst = max(r[0] for r in report)
    err, tol, k = max(report, key=lambda r: r[0] / r[1])
    print(f"{what} {case}: worst device error {worst:.3e}; closest to its bound: {k} {err:.3e} of {tol:.3e}")
    bad = [(k, err, tol) for err, tol, k in report if not err <= tol]
    assert not bad, (what, case, bad[:8])


def _check_losses(losses, ref, case):
    for i, name in enumerate(("total", "policy", "value")):
        l64, l32 = ref["f64"][0]["losses"][i], ref["f32"][0]["losses"][i]
        err, e32 = abs(losses[i] - l64) / abs(l64), abs(l32 - l64) / abs(l64)
        print(f"loss {name} {case}: device error {err:.3e} (e32 {e32:.3e})")
        assert err <= C.tolerance(e32), (name, losses[i], l64)


def _one_step(case, **more):
    """One step of PARITY_CASES[case] on the device against the reference: the checks of
    test_train_chess_gpu.test_one_step_gradients_and_losses.  `more` goes to ChessTrainer.
    Returns (ref, the device's weights after the step)."""
    shape = C.PARITY_CASES[case][0]
    ref = C.parity_reference(case)
    x = ref["batch"][0]
    zero = C.zero_planes(x)
    assert set(C.ZERO_PLANES) <= set(zero)
    assert x[..., 116].max() >= 100 and np.all(x[0, :, :, :84] == 0)  # a large move counter; a game's first plies
    tr = _trainer(shape, ref["weights"], **more)
    losses = tr.step(*ref["batch"], **HYPER)
    dev, w1 = tr.read_all(az.TRAIN_GRAD), tr.read_all(az.TRAIN_WEIGHT)
    # the same step without the L2 term, for the zero input channels below
    tr.set_weights(ref["weights"].items())
    tr.reset_momentum()
    tr.step(*ref["batch"], **dict(HYPER, l2=0.0))
    stem_no_l2 = tr.read("stem.kernel", az.TRAIN_GRAD)
    tr.close()
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    assert sorted(dev) == sorted(g64)
    _check_losses(losses, ref, case)
    for k in g64:  # conv biases in front of a BN: true gradient 0
        unit = C.conv_bias_unit(k)
        if unit is not None:
            assert np.linalg.norm(dev[k]) <= 1e-4 * np.linalg.norm(g64[unit + ".gamma"]), k
    # input channels that are zero over the batch: no data gradient at all
    assert np.all(stem_no_l2[:, :, zero, :] == 0.0)
    l2_term = (np.float32(2.0) * np.float32(HYPER["l2"])) * ref["weights"]["stem.kernel"][:, :, zero, :]
    assert np.array_equal(dev["stem.kernel"][:, :, zero, :], l2_term)
    live = [c for c in range(C.PLANES) if c not in zero]
    assert np.all(np.abs(stem_no_l2[:, :, live, :]).max(axis=(0, 1, 3)) > 0)
    _check_tensors(dev, g64, g32, "grad", case)
    return ref, w1


# ---------------------------------------------------------------- 1. edge shapes
@pytest.mark.parametrize("shape", C.EDGE_SHAPES, ids=lambda s: f"n{s[0]}_d{s[1]}_h{s[2]}")
def test_one_step_at_the_edge_shapes(shape):
    """train_chess_ref.EDGE_SHAPES: one, two and three board parts, value_hidden 1 / 300 / 1024, depth 4."""
    _one_step("n%d_d%d_h%d" % shape)


def test_depth_16_losses():
    """The ABI's deepest tower at n = 8.  Only the three losses are compared (e32
    2.2e-6 / 8.7e-8 / 3.1e-5): thirty-three BatchNormalizations deep, the CPU's own
    float32 gradient is 2e-2 from float64, so e32 gives no bound a correct kernel
    must meet, and the gradients are only required to be finite."""
    case = "depth16"
    ref = C.parity_reference(case)
    tr = _trainer(C.DEEPEST, ref["weights"])
    losses = tr.step(*ref["batch"], **HYPER)
    dev = tr.read_all(az.TRAIN_GRAD)
    tr.close()
    _check_losses(losses, ref, case)
    assert sorted(dev) == sorted(ref["f64"][0]["grad"])
    for k, g in dev.items():
        assert np.all(np.isfinite(g)), k


# ---------------------------------------------------------------- 2. the 1e-7 inside the log
@pytest.mark.parametrize("case", ["policy_x4", "policy_x8"])
def test_softmax_backward_keeps_the_epsilon_in_the_log(case):
    """policy.dense.kernel x4 and x8: the smallest probability on a target move
    falls to 4.3e-7 and 2.0e-11, where p + 1e-7 is no longer p.  The gradient of
    the loss without the epsilon (dlogit = (p - pi) / n) is 3.8e-3 and 1.1e-1 from
    the true one on policy.dense.bias, 6.8e-3 and 3.1e-1 on stem.kernel, asserted
    here at 100 tolerances at least, so a chess_heads_kernel that took the
    shortcut fails the per-tensor check."""
    ref = C.parity_reference(case)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    short, pmin = C.shortcut_gradient(ref, 1, ["policy.dense.bias", "stem.kernel"])
    for k in short:
        print(f"{case} min p on a target {pmin:.2e}: shortcut gradient of {k} is {C.rel_l2(short[k], g64[k]):.2e} away")
        assert C.rel_l2(short[k], g64[k]) >= 100 * C.tolerance(C.rel_l2(g32[k], g64[k]))
    _one_step(case)


# ---------------------------------------------------------------- 3. saturation, dead channels, bn_epsilon
def test_saturated_value_head():
    """value.dense2.kernel x6 (train_chess_ref.SATURATION): |v| reaches 0.978 and
    the factor 1 - v^2 of the value head's backward falls to 4.4e-2."""
    ref, _ = _one_step("saturated")
    _, v = C.float64_forward(ref, 1)
    print(f"saturated value head: max |v| {np.abs(v).max():.4f}")
    assert np.abs(v).max() >= 0.97


def test_channels_with_zero_variance():
    """A zero conv kernel leaves y = bias on every row: sigma^2 = 0, invstd =
    1/sqrt(eps), yhat = 0.  The gradients go through the usual check; the
    moving variance of those channels must move toward 0 by the moving-average
    rule alone, m x var (float64: asserted on the reference), which the
    device's read-back is held to like every other statistic."""
    case = "dead_channels"
    ref, w1 = _one_step(case)
    r64, r32, w0 = ref["f64"][0]["w"], ref["f32"][0]["w"], ref["weights"]
    for unit, c in C.DEAD.items():
        assert not np.asarray(w0[unit + ".kernel"])[..., c].any()
    stats = {k: v for k, v in r64.items() if not C.is_trainable(k)}
    _check_tensors(w1, stats, r32, "w", case)
    pick = lambda d: {u + ".var": np.asarray(d[u + ".var"])[[c]] for u, c in C.DEAD.items()}  # noqa: E731
    for k, v in pick(r64).items():
        assert abs(v[0] - HYPER["bn_momentum"] * float(pick(w0)[k][0])) <= 1e-12 * v[0], k
        assert 0 < v[0] < float(pick(w0)[k][0])
    _check_tensors(pick(w1), pick(r64), pick(r32), "w", case + "' moving variance")


def test_bn_epsilon_reaches_the_kernels():
    """bn_epsilon = 1e-5.  On the CPU alone, the float64 gradient on the same
    weights and batch with eps = 1e-3 is 2.2e-5 (policy.dense.bias) to 2.2e-2
    (value.dense1.bias) from the eps = 1e-5 gradient, 22 to 6500 tolerances: a
    trainer that ignored the field fails on nearly every tensor; at least one at
    100 tolerances is asserted."""
    case = "eps_1e-5"
    ref = C.parity_reference(case)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    other = C.gradient_at_another_epsilon(ref, 1, 1e-3)
    ratio = {k: C.rel_l2(other[k], g64[k]) / C.tolerance(C.rel_l2(g32[k], g64[k]))
             for k in g64 if C.conv_bias_unit(k) is None}
    print(f"{case}: the eps = 1e-3 gradient is {min(ratio.values()):.0f} to {max(ratio.values()):.0f} tolerances away")
    assert max(ratio.values()) >= 100
    _one_step(case, bn_epsilon=C.EPS_CASE)


# ---------------------------------------------------------------- 4. the update against the device's own gradient
def _snapshot(tr):
    return [tr.read_all(what) for what in (az.TRAIN_GRAD, az.TRAIN_MOMENTUM, az.TRAIN_WEIGHT)]


def test_first_update_is_exact():
    """First step after set_weights (zero momentum): a = -(lr * g), w = w0 + a in
    float32, the same with or without a fused multiply-add, so bitwise.  g is
    the device's own gradient, L2 term included."""
    shape = (5, 1, 256)
    w0 = C.R.make_weights(C.make_spec(1), seed=0)
    tr = _trainer(shape, w0)
    tr.step(*C.make_batch(5, seed=0), **HYPER)
    g, m, w1 = _snapshot(tr)
    tr.close()
    lr = np.float32(HYPER["lr"])
    assert g["policy.dense.kernel"].shape == (128, 1880) and g["stem.kernel"].shape == (3, 3, 118, 128)
    for k in g:
        a = -(lr * g[k])
        assert a.dtype == np.float32
        assert np.array_equal(m[k], a), k
        assert np.array_equal(w1[k], w0[k].reshape(a.shape) + a), k
    for k in w1:  # the moving statistics are no part of this update but do move
        if not C.is_trainable(k):
            assert not np.array_equal(w1[k], w0[k].reshape(w1[k].shape)), k


def test_l2_reaches_the_kernels_and_nothing_else():
    """The same state and batch at l2 = 0 and l2 = 0.5.  The step adds
    2 * l2 * w = w to a .kernel tensor's gradient in one float32 operation, so
    the two gradients differ by w within half an ulp of the sum, which is at
    most one ulp of the larger of |w| and |g|; every other tensor's gradient,
    and the policy and value losses, are the same bits."""
    shape = (5, 1, 256)
    w0 = C.R.make_weights(C.make_spec(1), seed=0)
    batch = C.make_batch(5, seed=0)
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
    assert err <= C.tolerance(0)


# ---------------------------------------------------------------- 5. no state across steps at the part boundary
def test_a_step_at_the_part_boundary_depends_on_its_own_state_and_batch_only():
    """Bitwise.  A max_batch = 17 trainer that has stepped on 17 other boards
    (three board parts, 17 row parts) from other weights and then gets A's
    weights, a zeroed momentum and A's 8-board batch (exactly one part) must
    leave what a fresh max_batch = 8 trainer leaves: losses, gradients, momentum
    and weights.  Nothing of the earlier step -- the second and third parts'
    split-K partials, rows 512.. of every activation, boards 8..16 of the heads'
    scratch -- may reach the later one."""
    spec = C.make_spec(1)
    A, other = C.R.make_weights(spec, seed=0), C.R.make_weights(spec, seed=1)
    X, Y = C.make_batch(8, seed=0), C.make_batch(17, seed=7)
    a = _trainer((8, 1, 256), A)
    losses_a = a.step(*X, **HYPER)
    snap_a = _snapshot(a)
    a.close()
    b = _trainer((17, 1, 256), other)
    b.step(*Y, **HYPER)
    b.set_weights(A.items())  # momentum is left as it is: the step differs from A's
    b.step(*X, **HYPER)
    assert any(v.tobytes() != snap_a[1][k].tobytes() for k, v in b.read_all(az.TRAIN_MOMENTUM).items())
    b.set_weights(A.items())
    b.reset_momentum()
    losses_b = b.step(*X, **HYPER)
    snap_b = _snapshot(b)
    b.close()
    assert losses_a == losses_b
    for da, db in zip(snap_a, snap_b):
        assert sorted(da) == sorted(db)
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), k
