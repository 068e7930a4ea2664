"""train / train_and_report with the reference's signatures
(custom_alphazero/model/tensorflow/train.py:14-116).

`model.fit(..., shuffle=False)` becomes a loop over PolicyValueModel.
train_on_batch (libaz's az_trainer_step): batches in order, a ragged last
batch trains on its own size, and the returned loss is the last epoch's mean
of the batch losses weighted by batch size, which is what Keras' History
reports.  TensorBoard is not part of this package: the scalars the reference
writes go, one JSON object per line, to <tensorboard_dir>/scalars.jsonl.
"""
import json
import math
import os
from typing import List, Tuple

import numpy as np

from custom_alphazero.config import ConfigGeneral, ConfigModel, ConfigPath, ConfigServing


def scheduled_learning_rate(steps: int) -> float:
    """ConfigModel.learning_rates' value for the range holding `steps`, else the minimum."""
    for steps_range, rate in ConfigModel.learning_rates.items():
        if steps in steps_range:
            return rate
    return ConfigModel.minimum_learning_rate


def train(model, inputs: np.ndarray, labels: List[np.ndarray], batch_size: int, epochs: int) -> float:
    policy_labels, value_labels = labels
    n = int(inputs.shape[0])
    batches = int(math.ceil(n / batch_size))
    loss = float("nan")
    for _ in range(epochs):
        weighted = 0.0
        for b in range(batches):
            sl = slice(b * batch_size, min(n, (b + 1) * batch_size))
            weighted += model.train_on_batch(inputs[sl], policy_labels[sl], value_labels[sl]) * (sl.stop - sl.start)
        loss = weighted / n
    model.steps += epochs * batches
    model.update_learning_rate(scheduled_learning_rate(model.steps))
    return loss


def train_replay(model, replay, idx: np.ndarray, batch_size: int, epochs: int) -> float:
    """train() on the samples idx of an engine.ChessReplay window, batch by batch through
    PolicyValueModel.train_on_replay: the same slices, loss weighting, steps and
    learning-rate schedule; no dense batch is built on the host."""
    idx = np.ascontiguousarray(idx, np.int64).reshape(-1)
    n = int(idx.shape[0])
    batches = int(math.ceil(n / batch_size))
    loss = float("nan")
    for _ in range(epochs):
        weighted = 0.0
        for b in range(batches):
            sl = slice(b * batch_size, min(n, (b + 1) * batch_size))
            weighted += model.train_on_replay(replay, idx[sl]) * (sl.stop - sl.start)
        loss = weighted / n
    model.steps += epochs * batches
    model.update_learning_rate(scheduled_learning_rate(model.steps))
    return loss


def _run_path(run_id: str, *parts) -> str:
    return os.path.join(ConfigPath.results_dir, ConfigGeneral.game, run_id, *parts)


def _write_scalars(directory: str, step: int, **scalars):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "scalars.jsonl"), "a") as fp:
        for tag, value in scalars.items():
            fp.write(json.dumps({"tag": tag, "step": int(step), "value": float(value)}) + "\n")


def train_and_report(run_id: str, last_model, states_batch: np.ndarray, policies_batch: np.ndarray,
                     values_batch: np.ndarray, training_iteration: int,
                     evaluation_iteration: int, replay=None) -> Tuple[bool, bool]:
    """One training iteration: train on the batch, checkpoint every
    model_checkpoint_frequency iterations, and every model_evaluation_frequency
    iterations play the arena against the best model so far and save the
    winner as the new best.  Returns (is_evaluated, is_updated).  With `replay`
    (an engine.ChessReplay) the batch is the window's samples states_batch, an
    index array, and policies_batch / values_batch are ignored (train_replay)."""
    from custom_alphazero.evaluation.evaluate import evaluate_two_models
    from custom_alphazero.utils import best_saved_model

    board = _run_path(run_id, ConfigPath.tensorboard_dir)
    if replay is not None:
        loss = train_replay(last_model, replay, states_batch, epochs=ConfigModel.training_epochs,
                            batch_size=ConfigModel.batch_size)
    else:
        loss = train(last_model, states_batch, [policies_batch, values_batch],
                     epochs=ConfigModel.training_epochs, batch_size=ConfigModel.batch_size)
    if (training_iteration + 1) % ConfigServing.model_checkpoint_frequency == 0:
        last_model.save_with_meta(_run_path(run_id, ConfigPath.training_dir))
    _write_scalars(board, training_iteration, **{"loss": loss, "steps": last_model.steps,
                                                  "learning rate": last_model.get_learning_rate()})
    is_evaluated = (training_iteration + 1) % ConfigServing.model_evaluation_frequency == 0
    is_updated = False
    if is_evaluated:
        previous_model = best_saved_model(run_id)  # the best so far, challenged in this iteration
        new_path = _run_path(run_id, ConfigPath.evaluation_dir, f"iteration_{evaluation_iteration}")
        os.makedirs(new_path, exist_ok=True)
        score, solver_score = evaluate_two_models(model=last_model, other_model=previous_model,
                                                  evaluate_with_mcts=ConfigServing.evaluate_with_mcts,
                                                  evaluate_with_solver=ConfigServing.evaluate_with_solver)
        is_updated = score >= ConfigServing.replace_min_score
        if is_updated:
            print(f"The current model is better, saving best model trained at {new_path}...")
            last_model.save_with_meta(new_path)
        else:
            print(f"The previous model was better, saving best model at {new_path}...")
            previous_model.save_with_meta(new_path)
        scalars = {"last model winning score": score}
        if solver_score is not None:
            scalars["solver score"] = solver_score
        _write_scalars(board, evaluation_iteration, **scalars)
    return is_evaluated, is_updated
