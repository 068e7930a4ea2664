"""CPU checks of the trainer's surroundings: the torch restatement of the
training step (tests/train_ref.py) checks itself, the replay window and the
schedule arithmetic of train() run with a stub model, and az_train.hip
compiles for gfx950 with its MFMA kernels inside the register budget."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import keras_ref
import train_ref as R
from custom_alphazero.config import ConfigModel, ConfigServing

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "custom-alphazero_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------ the restatement
def _small():
    H, W, depth = 4, 5, 2
    spec = R.make_spec(H, W, True, depth, filters=8, hidden=16)
    return H, W, depth, spec, R.make_weights(spec, 3), R.make_batch(H, W, True, 6, seed=3)


def test_autograd_matches_finite_differences():
    """Directional central differences of the total loss (float64, filters = 8)
    against autograd's gradient, along a random direction per tensor."""
    H, W, depth, spec, weights, (x, pi, z) = _small()
    ref = R.RefTrainer(spec, weights, depth, torch.float64)
    w0 = {k: v.clone() for k, v in ref.w.items()}
    ref.step(x, pi, z, lr=0.0)
    grads = ref.grad
    xt, pt, zt = (torch.tensor(a, dtype=torch.float64) for a in (x, pi, z))

    def total(w):
        probs, values, _ = R.forward_train(w, xt, depth)
        return float(R.loss_terms(w, probs, values, pt, zt, 1e-4)[0])

    gen = torch.Generator().manual_seed(0)
    eps = 1e-6
    for name in grads:
        d = torch.randn(w0[name].shape, generator=gen, dtype=torch.float64)
        plus, minus = dict(w0), dict(w0)
        plus[name] = w0[name] + eps * d
        minus[name] = w0[name] - eps * d
        fd = (total(plus) - total(minus)) / (2 * eps)
        an = float((grads[name] * d).sum())
        scale = float(grads[name].norm() * d.norm())
        if R.conv_bias_unit(name):  # a conv bias in front of a training-mode BN: exactly no effect
            assert abs(fd) < 1e-8 and abs(an) < 1e-12, (name, fd, an)
        else:
            assert abs(fd - an) <= 1e-6 * scale + 1e-9, (name, fd, an)


def test_two_momentum_steps_match_the_closed_form():
    """Keras SGD: a1 = -lr g1, w1 = w0 + a1, a2 = mu a1 - lr g2, w2 = w1 + a2."""
    H, W, depth, spec, weights, batch = _small()
    ref = R.RefTrainer(spec, weights, depth, torch.float64)
    w0 = {k: v.clone() for k, v in ref.w.items()}
    lr, mu = 0.05, 0.9
    ref.step(*batch, lr, mu)
    g1 = dict(ref.grad)
    ref.step(*batch, lr, mu)
    g2 = dict(ref.grad)
    for name in g1:
        a2 = mu * (-lr * g1[name]) - lr * g2[name]
        assert torch.allclose(ref.mom[name], a2, rtol=1e-13, atol=0)
        assert torch.allclose(ref.w[name], w0[name] - lr * g1[name] + a2, rtol=1e-13, atol=1e-18)
    # g2 is the gradient at w1, not at w0
    assert any(not torch.equal(g1[k], g2[k]) for k in g1)


def test_moving_variance_takes_bessels_correction():
    """The stem's moving statistics after one step, against numpy on the
    oracle's own convolution: mean <- m mean + (1-m) mu, var <- m var +
    (1-m) * unbiased variance (ddof = 1)."""
    H, W, depth, spec, weights, (x, pi, z) = _small()
    ref = R.RefTrainer(spec, weights, depth, torch.float64)
    m = 0.9
    ref.step(x, pi, z, lr=0.0, bn_momentum=m)
    y = keras_ref.conv2d_same(np.asarray(x, np.float64), np.asarray(weights["stem.kernel"], np.float64),
                              np.asarray(weights["stem.bias"], np.float64)).reshape(-1, 8)
    N = y.shape[0]
    mean = m * weights["stem.mean"].astype(np.float64) + (1 - m) * y.mean(axis=0)
    var = m * weights["stem.var"].astype(np.float64) + (1 - m) * y.var(axis=0, ddof=1)
    assert np.allclose(ref.w["stem.mean"].numpy(), mean, rtol=1e-12, atol=1e-15)
    assert np.allclose(ref.w["stem.var"].numpy(), var, rtol=1e-12)
    assert R.bessel_factor(N) == N / (N - 1.0)
    biased = m * weights["stem.var"].astype(np.float64) + (1 - m) * y.var(axis=0)
    assert not np.allclose(ref.w["stem.var"].numpy(), biased, rtol=1e-6)


def test_tolerance_rule():
    assert R.tolerance(0.0) == 1e-6 and R.tolerance(1e-6) == 8e-6 and R.tolerance(1.0) == 1e-4


# ------------------------------------------------------------ the loop
def test_replay_window_keeps_the_newest_samples(monkeypatch):
    from custom_alphazero.train import _append_and_limit_queues
    monkeypatch.setattr(ConfigServing, "samples_queue_size", 5)
    s, p, v = np.empty((0, 2, 2, 4)), np.empty((0, 3)), np.empty(0)

    def feed(lo, hi):
        k = np.arange(lo, hi, dtype=np.float64)
        return lambda: (np.tile(k[:, None, None, None], (1, 2, 2, 4)), np.tile(k[:, None], (1, 3)), k)

    s, p, v = _append_and_limit_queues(s, p, v, feed(0, 3))
    assert len(s) == len(p) == len(v) == 3
    s, p, v = _append_and_limit_queues(s, p, v, feed(3, 7))
    assert list(v) == [2, 3, 4, 5, 6] and list(p[:, 0]) == [2, 3, 4, 5, 6] and list(s[:, 0, 0, 0]) == [2, 3, 4, 5, 6]
    # an empty retrieval leaves the window alone
    s2, p2, v2 = _append_and_limit_queues(s, p, v, lambda: (np.empty((0, 2, 2, 4)), np.empty((0, 3)), np.empty(0)))
    assert s2 is s and p2 is p and v2 is v


class _StubModel:
    """train()'s view of a model: train_on_batch, steps, the learning rate."""

    def __init__(self):
        self.steps, self.learning_rate, self.calls = 0, 1e-2, []

    def train_on_batch(self, x, pi, z):
        assert len(x) == len(pi) == len(z)
        self.calls.append((len(x), float(x[0, 0]), self.learning_rate))
        return float(len(self.calls))  # batch i reports loss i

    def update_learning_rate(self, lr):
        self.learning_rate = float(lr)


def test_train_batches_steps_and_schedule(monkeypatch):
    from custom_alphazero.model.tensorflow.train import scheduled_learning_rate, train
    monkeypatch.setattr(ConfigModel, "learning_rates", {range(0, 5): 0.5, range(5, 8): 0.25})
    monkeypatch.setattr(ConfigModel, "minimum_learning_rate", 0.125)
    x = np.arange(10, dtype=np.float32)[:, None]
    m = _StubModel()
    loss = train(m, x, [np.zeros((10, 7)), np.zeros(10)], batch_size=4, epochs=2)
    # batches in order, the ragged last one on its own size, no shuffling
    assert [(n, first) for n, first, _ in m.calls] == [(4, 0.0), (4, 4.0), (2, 8.0)] * 2
    assert all(lr == 1e-2 for _, _, lr in m.calls)  # the rate only changes after the call
    # the last epoch's batch losses 4, 5, 6 weighted by 4, 4, 2 samples
    assert loss == pytest.approx((4 * 4 + 5 * 4 + 6 * 2) / 10)
    assert m.steps == 6 and m.learning_rate == 0.25
    train(m, x, [np.zeros((10, 7)), np.zeros(10)], batch_size=10, epochs=2)
    assert m.steps == 8 and m.learning_rate == 0.125  # outside every range: the minimum
    assert scheduled_learning_rate(0) == 0.5 and scheduled_learning_rate(4) == 0.5
    assert scheduled_learning_rate(5) == 0.25 and scheduled_learning_rate(8) == 0.125


def test_default_schedule_is_the_references():
    from custom_alphazero.model.tensorflow.train import scheduled_learning_rate
    assert scheduled_learning_rate(0) == 1e-2 and scheduled_learning_rate(149999) == 1e-2
    assert scheduled_learning_rate(150000) == 1e-3 and scheduled_learning_rate(300000) == 1e-4
    assert ConfigModel.bn_momentum == 0.99


def test_step_flop_counts_the_tower():
    from custom_alphazero.train import step_flop
    # 256 boards of 6x7 at depth 4: about 80 GFLOP
    assert step_flop(256, 6, 7, 4) == 3 * 4 * 19 * 2 * 256 * 42 * 128 * 128
    assert 79e9 < step_flop(256, 6, 7, 4) < 82e9


# ------------------------------------------------------------ compile-time
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_train_kernels_build_without_spills(tmp_path):
    """az_train.hip builds for gfx950, and its MFMA kernels -- the conv forward
    and data gradient (conv_mfma_kernel) and the weight gradient
    (wgrad_mfma_kernel) -- keep every accumulator in registers."""
    out = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "az_train.hip"),
         "-o", str(tmp_path / "t.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    spills, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    # <taps, data gradient, second (1x1) input>
    fwd = [v for k, v in spills.items() if "conv_mfma_kernelILi9ELb0ELb0E" in k or "conv_mfma_kernelILi1ELb0ELb0E" in k]
    dgrad = [v for k, v in spills.items() if "conv_mfma_kernelILi9ELb1E" in k or "conv_mfma_kernelILi1ELb1E" in k]
    wgrad = [v for k, v in spills.items() if "wgrad_mfma_kernel" in k]
    assert len(fwd) == 2 and len(dgrad) == 3 and len(wgrad) == 2, spills
    assert fwd == [0, 0] and dgrad == [0, 0, 0] and wgrad == [0, 0], spills
    assert all(v == 0 for v in spills.values()), spills


def test_bn_epsilon_case_meets_the_input_condition():
    """test_train_shapes_gpu.test_bn_epsilon_reaches_the_kernels' input (6x7, n 5, depth 1, eps 1e-5),
    without a GPU: every tensor's e32 <= KINK_FREE, ReLU margin >= 0.95 x CLEAR_MARGIN, and the
    eps = 1e-3 gradient on the same weights 100 tolerances or more away."""
    hyper = dict(lr=1e-2, momentum=0.9, l2=1e-4, bn_momentum=0.99)
    ref = R.reference_run(6, 7, True, 5, 1, eps=1e-5, **hyper)
    assert R.reference_run(6, 7, True, 5, 1, **hyper) is R.reference_run(6, 7, True, 5, 1, eps=1e-3, **hyper)
    g64, g32 = ref["f64"][0]["grad"], ref["f32"][0]["grad"]
    names = [k for k in g64 if R.conv_bias_unit(k) is None]
    assert all(R.rel_l2(g32[k], g64[k]) <= R.KINK_FREE for k in names)
    assert ref["f64"][0]["relu_margin"] >= 0.95 * R.CLEAR_MARGIN
    other = R.RefTrainer(ref["spec"], ref["weights"], 1, torch.float64, eps=1e-3)
    other.step(*ref["batch"], **hyper)
    assert max(R.rel_l2(other.grad[k].numpy(), g64[k]) / R.tolerance(R.rel_l2(g32[k], g64[k])) for k in names) >= 100
