"""The training loop (reference custom_alphazero/train.py:16-92): a replay
window fed from the self-play queue, one train_and_report on batch_size
samples drawn without replacement per iteration.

The reference reads the queue and announces a new best model over HTTP
(serving/factory.py); that control plane is not part of this package, so the
two calls are parameters: `retrieve_queue() -> (states, policies, values)` and
`update_best_model()`.

`python -m custom_alphazero.train --bench` times the training step
(az_trainer_step, csrc/az_train.hip) on 256 boards of 6x7 at depth 4 and the
same step in torch-ROCm autograd on the same GPU; one JSON line.  `--game
chess` times the chess network's step (256 boards of 8x8x118 planes, 1880
actions) the same way.
"""
import json
import os
import sys
import time
from typing import Callable, Optional, Tuple

import numpy as np

from custom_alphazero.config import ConfigGeneral, ConfigModel, ConfigPath, ConfigServing

FP32_MATRIX_PEAK = 157.3e12  # MI355X dense fp32 MFMA FLOP/s (256 CUs x 256 FLOP/clk x 2.4 GHz)


def _append_and_limit_queues(local_states_queue: np.ndarray, local_policies_queue: np.ndarray,
                             local_values_queue: np.ndarray, retrieve_queue: Callable
                             ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Append what the queue holds and keep the newest samples_queue_size
    samples; a retrieval with any empty array leaves the window as it is."""
    size = ConfigServing.samples_queue_size
    states, policies, values = retrieve_queue()
    if all(np.asarray(a).size for a in (states, policies, values)):
        local_states_queue = np.vstack([local_states_queue, states])[-size:]
        local_policies_queue = np.vstack([local_policies_queue, policies])[-size:]
        local_values_queue = np.append(local_values_queue, values)[-size:]
    return local_states_queue, local_policies_queue, local_values_queue


def last_saved_model(run_id: str):
    """The model under <run>/training if one was saved, else a fresh one (utils.py:51-61)."""
    from custom_alphazero.utils import init_model
    path = os.path.join(ConfigPath.results_dir, ConfigGeneral.game, run_id, ConfigPath.training_dir)
    if os.path.exists(os.path.join(path, ConfigPath.model_success)):
        return init_model(path)
    print(f"Warning: no model found at {path}, initializing last model with random weights")
    return init_model()


def training_loop(run_id: str, retrieve_queue: Callable, update_best_model: Optional[Callable] = None,
                  max_iterations: Optional[int] = None, model=None):
    """Runs until max_iterations training iterations are done (None: for ever).
    Returns the model it trained."""
    from custom_alphazero.model.tensorflow.train import train_and_report

    last_model = model if model is not None else last_saved_model(run_id)
    states = np.empty((0, *last_model.input_dim))
    policies = np.empty((0, last_model.action_space))
    values = np.empty(0)
    training_iteration, evaluation_iteration = 0, 0
    while max_iterations is None or training_iteration < max_iterations:
        states, policies, values = _append_and_limit_queues(states, policies, values, retrieve_queue)
        if len(states) >= ConfigServing.minimum_training_size:
            idx = np.random.choice(len(states), ConfigModel.batch_size, replace=False)
            is_evaluated, is_updated = train_and_report(run_id, last_model, states[idx], policies[idx],
                                                        values[idx], training_iteration, evaluation_iteration)
            if is_updated and update_best_model is not None:
                update_best_model()
            if is_evaluated:
                evaluation_iteration += 1
            training_iteration += 1
            if max_iterations is not None and training_iteration >= max_iterations:
                break
        time.sleep(ConfigServing.training_loop_sleep_time)
    return last_model


# ------------------------------------------------------------------ --bench
def step_flop(n: int, height: int, width: int, depth: int, filters: int = 128, stem_planes: int = 0) -> float:
    """FLOP of the 128 -> 128 convolutions of one step: per block two 3x3 and
    one 1x1 (19 taps), each once forward, once as data gradient and once as
    weight gradient; the heads and the elementwise work are not counted, and
    neither is the stem unless `stem_planes` is given (the chess stem's 118:
    a 3x3 convolution forward and as weight gradient; it has no data gradient)."""
    rows = n * height * width
    return 3.0 * depth * 19 * 2.0 * rows * filters * filters + 2.0 * 9 * 2.0 * rows * stem_planes * filters


def _torch_step_time(weights, batch, depth, steps, warmup, lr, momentum, l2, eps, bn_momentum):
    """The same step in torch-ROCm autograd (fp32, conv2d + batch_norm in training mode)."""
    import torch
    import torch.nn.functional as Fn
    dev = torch.device("cuda", 0)
    w = {}
    for k, v in weights.items():
        t = torch.from_numpy(np.asarray(v, np.float32)).to(dev)
        if k.endswith(".kernel") and t.dim() == 4:
            t = t.permute(3, 2, 0, 1).contiguous()  # OIHW
        w[k] = t
    train_names = [k for k in w if k.rsplit(".", 1)[1] not in ("mean", "var")]
    for k in train_names:
        w[k].requires_grad_(True)
    mom = {k: torch.zeros_like(w[k]) for k in train_names}
    x = torch.from_numpy(batch[0]).to(dev).permute(0, 3, 1, 2).contiguous()
    pi, z = torch.from_numpy(batch[1]).to(dev), torch.from_numpy(batch[2]).to(dev)

    def unit(h, name, relu):
        k = w[name + ".kernel"]
        y = Fn.conv2d(h, k, w[name + ".bias"], padding=k.shape[2] // 2)
        y = Fn.batch_norm(y, w[name + ".mean"], w[name + ".var"], w[name + ".gamma"], w[name + ".beta"],
                          True, 1.0 - bn_momentum, eps)
        return torch.relu(y) if relu else y

    def one():
        h = unit(x, "stem", True)
        for d in range(depth):
            a = unit(unit(h, f"block{d}.conv1", True), f"block{d}.conv2", False)
            h = torch.relu(a + unit(h, f"block{d}.res", False))
        n = x.shape[0]
        p = unit(h, "policy.conv", True).permute(0, 2, 3, 1).reshape(n, -1)
        probs = torch.softmax(p @ w["policy.dense.kernel"] + w["policy.dense.bias"], dim=1)
        v = unit(h, "value.conv", True).permute(0, 2, 3, 1).reshape(n, -1)
        v = torch.relu(v @ w["value.dense1.kernel"] + w["value.dense1.bias"])
        v = torch.tanh(v @ w["value.dense2.kernel"] + w["value.dense2.bias"]).reshape(n)
        loss = (-(pi * torch.log(probs + 1e-7)).sum(dim=1)).mean() + ((v - z) ** 2).mean()
        loss = loss + l2 * sum((w[k] ** 2).sum() for k in train_names if k.endswith(".kernel"))
        grads = torch.autograd.grad(loss, [w[k] for k in train_names])
        with torch.no_grad():
            ms = [mom[k] for k in train_names]
            torch._foreach_mul_(ms, momentum)
            torch._foreach_add_(ms, grads, alpha=-lr)
            torch._foreach_add_([w[k] for k in train_names], ms)
        return float(loss)  # synchronises, as az_trainer_step does

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _chess_batch(rng, n):
    """Planes shaped like chess Board.full_state (chess/board.py): per history
    step a one-hot over 13 planes per cell and a per-board repetition plane,
    then four castling flags and the two move counters; pi sparse over at most
    218 of the 1880 actions."""
    x = np.zeros((n, 8, 8, 118), np.float32)
    for s in range(8):
        x[..., 14 * s:14 * s + 13] = np.eye(13, dtype=np.float32)[rng.randint(0, 13, size=(n, 8, 8))]
        x[..., 14 * s + 13] = rng.randint(0, 2, size=(n, 1, 1))
    x[..., 112:116] = rng.randint(0, 2, size=(n, 1, 1, 4))
    x[..., 116] = rng.randint(1, 120, size=(n, 1, 1))
    x[..., 117] = rng.randint(0, 100, size=(n, 1, 1))
    pi = np.zeros((n, 1880), np.float32)
    for b in range(n):
        moves = rng.choice(1880, size=rng.randint(1, 219), replace=False)
        pi[b, moves] = rng.dirichlet(np.ones(len(moves)))
    return x, pi


def _host_copy_ms(x, repeats=20):
    """The median time of one copy of x from pageable host memory to the device,
    which every step makes (az_trainer_step takes host buffers)."""
    import torch
    dev = torch.device("cuda", 0)
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.from_numpy(x).to(dev)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def bench(n=256, height=6, width=7, depth=4, steps=50, warmup=5, game="connect_n"):
    from custom_alphazero import engine as az
    from custom_alphazero.model.weights import init_weights, weight_spec
    if game not in ("connect_n", "chess"):
        raise ValueError(f"bench: game must be 'connect_n' or 'chess', got {game!r}")
    chess = game == "chess"
    if chess:
        height = width = 8
    planes, actions = (118, 1880) if chess else (4, width)
    spec = weight_spec(height, width, actions, ConfigModel.filters, depth, ConfigModel.value_hidden, planes)
    weights = init_weights(spec, seed=0, randomize_bn=True)
    rng = np.random.RandomState(0)
    if chess:
        x, pi = _chess_batch(rng, n)
    else:
        x = np.eye(4, dtype=np.float32)[rng.randint(0, 4, size=(n, height, width))]
        pi = rng.dirichlet(np.ones(width), size=n).astype(np.float32)
    z = rng.randint(-1, 2, size=n).astype(np.float32)
    hyper = dict(lr=ConfigModel.minimum_learning_rate, momentum=ConfigModel.momentum,
                 l2=ConfigModel.l2_penalization_term, bn_momentum=ConfigModel.bn_momentum)
    common = dict(max_batch=n, filters=ConfigModel.filters, depth=depth, value_hidden=ConfigModel.value_hidden,
                  bn_epsilon=ConfigModel.bn_epsilon)
    tr = az.ChessTrainer(**common) if chess else az.Trainer(height, width, True, **common)
    tr.set_weights(weights.items())
    for _ in range(warmup):
        tr.step(x, pi, z, **hyper)
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x, pi, z, **hyper)
    ms = (time.perf_counter() - t0) / steps * 1e3
    tr.close()
    torch_ms = _torch_step_time(weights, (x, pi, z), depth, steps, warmup, eps=ConfigModel.bn_epsilon, **hyper)
    flop = step_flop(n, height, width, depth, stem_planes=planes if chess else 0)
    rec = {"bench": "train_step", "boards": n, "board": [height, width], "depth": depth, "steps": steps,
           "warmup": warmup, "ms_per_step": round(ms, 4), "flop_per_step": flop,
           "fp32_matrix_peak_fraction": round(flop / (ms * 1e-3) / FP32_MATRIX_PEAK, 4),
           "torch_autograd_ms_per_step": round(torch_ms, 4)}
    if chess:
        # the device step copies its batch from pageable host memory every step; the torch step above keeps
        # its batch on the device.  flop_per_step counts the stem here.
        copy_ms = _host_copy_ms(x)
        rec.update({"game": "chess", "planes": planes, "actions": actions, "x_bytes": int(x.nbytes),
                    "host_copy_ms": round(copy_ms, 4), "ms_per_step_less_copy": round(ms - copy_ms, 4)})
    return rec


if __name__ == "__main__":
    if "--bench" in sys.argv[1:]:
        args = sys.argv[1:]
        game = args[args.index("--game") + 1] if "--game" in args and args.index("--game") + 1 < len(args) \
            else "connect_n"
        print(json.dumps(bench(game=game)))
    else:
        raise SystemExit("the serving control plane (run id, sample queue, best-model update over HTTP) is not "
                         "part of this package: call training_loop(run_id, retrieve_queue, update_best_model), "
                         "or run with --bench")
