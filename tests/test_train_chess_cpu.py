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
