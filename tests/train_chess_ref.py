"""The chess network's training step for tests/test_train_chess_*.py (TEST
INFRASTRUCTURE): tests/train_ref.py's float64 / float32 torch restatement,
which is generic over the weight spec, on the chess spec
weight_spec(8, 8, 1880, 128, depth, hidden, 118) and on batches shaped like
chess Board.full_state (custom_alphazero/chess/board.py, csrc/az_chess.h
state_feats / full_state4).  Nothing here touches libaz.

A batch's planes, all small integers as the encoder writes them:
  14 s + 0..12  history step s (0 oldest .. 7 the board): one-hot per cell over
                empty / six white / six black piece codes
  14 s + 13     step s's repetition flag, constant over the board
  112..115      castling rights (own / opponent, queen / king side), 0 or 1
  116           fullmove_number (1 .., one board of every batch has >= 100)
  117           halfmove_clock
Board 0 (and every third board after it) is a game's first plies: its six
oldest history steps are all zero.  Planes 13 (the oldest step's repetition
flag) and 115 are zero in every board, so every batch has input channels that
are zero over the whole batch (ZERO_PLANES; at n = 1 also planes 0..83): the
stem kernel's data gradient there is exactly zero, which the device test
asserts.  pi is sparse as self-play's is: row 0 a single 1.0, row 1 (if there
is one) 218 non-zeros, the most legal moves of any position, the other rows
2..217 non-zeros.  z is in {-1, 0, 1}.
"""
import numpy as np
import torch

import train_ref as R
from custom_alphazero.model.weights import weight_spec

PLANES, ACTIONS, HISTORY = 118, 1880, 8
ZERO_PLANES = (13, 115)

forward_train, RefTrainer, clear_kinks = R.forward_train, R.RefTrainer, R.clear_kinks
rel_l2, tolerance, conv_bias_unit = R.rel_l2, R.tolerance, R.conv_bias_unit
MIN_RELU_MARGIN, KINK_FREE, CLEAR_MARGIN = R.MIN_RELU_MARGIN, R.KINK_FREE, R.CLEAR_MARGIN
is_trainable = R.is_trainable


def make_spec(depth, hidden=256):
    return weight_spec(8, 8, ACTIONS, 128, depth, hidden, PLANES)


def make_batch(n, seed=0):
    rng = np.random.RandomState(seed)
    x = np.zeros((n, 8, 8, PLANES), np.float32)
    for s in range(HISTORY):
        x[..., 14 * s:14 * s + 13] = np.eye(13, dtype=np.float32)[rng.randint(0, 13, size=(n, 8, 8))]
        x[..., 14 * s + 13] = rng.randint(0, 2, size=(n, 1, 1))
    x[0::3, :, :, :14 * 6] = 0.0  # a game's first plies: no history yet
    x[..., 112:116] = rng.randint(0, 2, size=(n, 1, 1, 4))
    x[..., 116] = rng.randint(1, 60, size=(n, 1, 1))
    x[n - 1, :, :, 116] = 100 + rng.randint(0, 50)
    x[..., 117] = rng.randint(0, 50, size=(n, 1, 1))
    for p in ZERO_PLANES:
        x[..., p] = 0.0
    pi = np.zeros((n, ACTIONS), np.float32)
    for b in range(n):
        k = 1 if b == 0 else 218 if b == 1 else rng.randint(2, 218)
        moves = rng.choice(ACTIONS, size=k, replace=False)
        pi[b, moves] = rng.dirichlet(np.ones(k)).astype(np.float32) if k > 1 else 1.0
    z = rng.randint(-1, 2, size=n).astype(np.float32)
    return x, pi, z


def zero_planes(x):
    """The input channels that are zero over the whole batch."""
    return [int(c) for c in np.nonzero(np.abs(x).reshape(-1, PLANES).max(axis=0) == 0)[0]]


# Batch seeds per (n, depth), chosen on the float64 CPU run alone (as train_ref.BATCH_SEEDS): of
# seeds 0..19, the one whose ReLU inputs stay farthest from zero over the two steps the two-step
# test takes (0 elsewhere).
BATCH_SEEDS = {(5, 2): 5}  # margin 2.6e-5 over both steps (seed 0: 5.0e-6; the worst, seed 9: 5.4e-8)

_CACHE = {}


def reference_run(n, depth, steps=1, lr=1e-2, momentum=0.9, l2=1e-4, bn_momentum=0.99, seed=0, hidden=256,
                  batch_seed=None):
    """train_ref.reference_run for the chess network: float64 and float32 CPU runs of `steps`
    steps on one fixed batch, computed once per argument set and shared (callers must not modify
    the result).  The weights are drawn from `seed` and moved clear of the first step's ReLU
    kinks by clear_kinks.  Returns spec, weights, batch and per dtype key ('f64', 'f32') the list
    of per-step records {losses, grad, mom, w, relu_margin}."""
    if batch_seed is None:
        batch_seed = BATCH_SEEDS.get((n, depth), 0)
    key = (n, depth, steps, lr, momentum, l2, bn_momentum, seed, hidden, batch_seed)
    if key in _CACHE:
        return _CACHE[key]
    spec = make_spec(depth, hidden)
    batch = make_batch(n, batch_seed)
    weights = clear_kinks(R.make_weights(spec, seed), batch[0], depth)
    out = {"spec": spec, "weights": weights, "batch": batch}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        ref = RefTrainer(spec, weights, depth, dt)
        recs = []
        for _ in range(steps):
            losses = ref.step(*batch, lr, momentum, l2, bn_momentum)
            recs.append({"losses": losses, "relu_margin": ref.relu_margin,
                         "grad": {k: v.numpy().astype(np.float64) for k, v in ref.grad.items()},
                         "mom": {k: v.numpy().astype(np.float64) for k, v in ref.mom.items()},
                         "w": {k: v.numpy().astype(np.float64) for k, v in ref.w.items()}})
        out[tag] = recs
    _CACHE[key] = out
    return out
