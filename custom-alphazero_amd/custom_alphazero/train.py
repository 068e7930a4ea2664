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
actions) the same way, and the same step from a device replay window
(Trainer.step_replay: ms_per_step_replay).
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


def _replay_loop(run_id, retrieve_queue, update_best_model, max_iterations, last_model, replay):
    """training_loop with the window on the device: the same iterations, the same
    np.random.choice draw over the same row order, no dense state on the host."""
    from custom_alphazero.model.tensorflow.train import train_and_report

    training_iteration, evaluation_iteration = 0, 0
    while max_iterations is None or training_iteration < max_iterations:
        records = retrieve_queue()
        if records:
            replay.push(**{k: records[k] for k in replay.KEYS})
        if len(replay) >= ConfigServing.minimum_training_size:
            idx = np.random.choice(len(replay), ConfigModel.batch_size, replace=False)
            is_evaluated, is_updated = train_and_report(run_id, last_model, idx, None, None, training_iteration,
                                                        evaluation_iteration, replay=replay)
            if is_updated and update_best_model is not None:
                update_best_model()
            if is_evaluated:
                evaluation_iteration += 1
            training_iteration += 1
            if max_iterations is not None and training_iteration >= max_iterations:
                break
        time.sleep(ConfigServing.training_loop_sleep_time)
    return last_model


def training_loop(run_id: str, retrieve_queue: Callable, update_best_model: Optional[Callable] = None,
                  max_iterations: Optional[int] = None, model=None, replay=None):
    """Runs until max_iterations training iterations are done (None: for ever).
    Returns the model it trained.  With `replay` (an engine.ChessReplay the
    caller sized to ConfigServing.samples_queue_size) the window lives on the
    device in compact form: retrieve_queue() then returns a dict with the keys
    of ChessReplay.push (engine.chess_replay_records makes one from self-play
    results), or a falsy value when the queue is empty."""
    from custom_alphazero.model.tensorflow.train import train_and_report

    last_model = model if model is not None else last_saved_model(run_id)
    if replay is not None:
        return _replay_loop(run_id, retrieve_queue, update_best_model, max_iterations, last_model, replay)
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


def _chess_records(rng, n):
    """A chess batch as compact replay records (the keys of engine.ChessReplay.push),
    whose dense form is shaped like Board.full_state (chess/board.py): per
    history step a random piece code per square, as az_chess_pos bitboards, and
    a repetition flag; random castling rights and move counters; the policy
    sparse over at most 218 of the 1880 actions, float64.  Every history entry
    is valid."""
    from custom_alphazero.chess import kernels as K
    code = rng.randint(0, 13, size=(n, 8, 64))  # Board.array codes: 0 empty, 1..6 white P..K, 7..12 black K..P
    hist = np.zeros((n, 8), K.POS_DTYPE)
    bit = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for t in range(6):
        hist["pieces"][..., t] = (((code == t + 1) | (code == 12 - t)) * bit).sum(axis=-1, dtype=np.uint64)
    hist["occupied_co"][..., 1] = (((code >= 1) & (code <= 6)) * bit).sum(axis=-1, dtype=np.uint64)
    hist["occupied_co"][..., 0] = ((code >= 7) * bit).sum(axis=-1, dtype=np.uint64)
    corners = np.array([1 << 0, 1 << 7, 1 << 56, 1 << 63], np.uint64)
    hist["castling_rights"] = (rng.randint(0, 2, size=(n, 8, 4)) * corners).sum(axis=-1, dtype=np.uint64)
    hist["ep_square"] = -1
    hist["turn"] = rng.randint(0, 2, size=(n, 8))
    hist["repetition"] = rng.randint(0, 2, size=(n, 8))
    hist["fullmove_number"] = rng.randint(1, 120, size=(n, 8))
    hist["halfmove_clock"] = rng.randint(0, 100, size=(n, 8))
    policy_n = np.zeros(n, np.int32)
    actions = np.zeros((n, K.MAX_MOVES), np.int16)
    probs = np.zeros((n, K.MAX_MOVES), np.float64)
    for b in range(n):
        k = rng.randint(1, 219)
        policy_n[b] = k
        actions[b, :k] = rng.choice(K.ACTIONS, size=k, replace=False)
        probs[b, :k] = rng.dirichlet(np.ones(k))
    return dict(hist=hist, valid=np.ones((n, 8), np.uint8), policy_n=policy_n, policy_actions=actions,
                policy_probs=probs, z=rng.randint(-1, 2, size=n).astype(np.float32))


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
    replay = None
    if chess:
        # the batch starts as compact records in a device replay window (the step_replay leg
        # below); every other leg takes the dense arrays the window gathers from them
        replay = az.ChessReplay(n)
        replay.push(**_chess_records(rng, n))
        x, pi, z = replay.gather(np.arange(n))
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
    if chess:
        idx = np.arange(n)
        for _ in range(warmup):
            tr.step_replay(replay, idx, **hyper)
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step_replay(replay, idx, **hyper)
        replay_ms = (time.perf_counter() - t0) / steps * 1e3
        replay.close()
    tr.close()
    torch_ms = _torch_step_time(weights, (x, pi, z), depth, steps, warmup, eps=ConfigModel.bn_epsilon, **hyper)
    flop = step_flop(n, height, width, depth, stem_planes=planes if chess else 0)
    rec = {"bench": "train_step", "boards": n, "board": [height, width], "depth": depth, "steps": steps,
           "warmup": warmup, "ms_per_step": round(ms, 4), "flop_per_step": flop,
           "fp32_matrix_peak_fraction": round(flop / (ms * 1e-3) / FP32_MATRIX_PEAK, 4),
           "torch_autograd_ms_per_step": round(torch_ms, 4)}
    if chess:
        # the device step copies its batch from pageable host memory every step; the torch step above keeps
        # its batch on the device, and ms_per_step_replay is the step from the device replay window
        # (Trainer.step_replay on the same boards: no dense batch on the host).  flop_per_step counts
        # the stem here.
        copy_ms = _host_copy_ms(x)
        rec.update({"game": "chess", "planes": planes, "actions": actions, "x_bytes": int(x.nbytes),
                    "host_copy_ms": round(copy_ms, 4), "ms_per_step_less_copy": round(ms - copy_ms, 4),
                    "ms_per_step_replay": round(replay_ms, 4)})
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
