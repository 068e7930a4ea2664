"""What ConfigMCTS.enable_dirichlet_noise costs chess self-play: expansions/s
of the benchmark's engine shape (800 sims/move, 256 games, the network
evaluator on random-init weights, 2 untimed and 3 timed moves) with root
noise off and with it drawn on the device at alpha 0.03 and 0.3, the
settings interleaved over `--rounds` rounds.  One JSON line per run, then a
summary line with each setting's median and its ratio to noise off.

    python profiles/chess_noise/noise_cost.py [--rounds 3] [--sims 800] [--slots 256]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "custom-alphazero_amd"))


def run(az, named, args, alpha):
    eng = az.ChessEngine(mcts_iterations=args.sims, slots=args.slots, evaluator=az.EVAL_NETWORK, max_plies=512,
                         dirichlet_noise=alpha is not None, dirichlet_alpha=alpha or 0.03, dirichlet_ratio=0.25)
    eng.set_weights(named)
    eng.selfplay_begin(0, 2 * args.slots, 0)
    eng.selfplay_step(args.warmup)
    st0 = eng.stats()
    t0 = time.perf_counter()
    st1 = eng.selfplay_step(args.steps)  # synchronous: waits for the moves
    dt = time.perf_counter() - t0
    eng.close()
    assert st1["errors"] == 0
    return (st1["expansions"] - st0["expansions"]) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    from custom_alphazero import engine as az
    from custom_alphazero.model.weights import init_weights, weight_spec
    named = list(init_weights(weight_spec(8, 8, 1880, depth=4, in_channels=118), seed=0).items())
    settings = [("off", None), ("alpha_0.03", 0.03), ("alpha_0.3", 0.3)]
    rates = {name: [] for name, _ in settings}
    for r in range(args.rounds):
        for name, alpha in settings:
            v = run(az, named, args, alpha)
            rates[name].append(v)
            print(json.dumps({"round": r, "noise": name, "expansions_per_s": round(v, 1)}), flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    print(json.dumps({"median_expansions_per_s": {k: round(v, 1) for k, v in med.items()},
                      "spread": {k: [round(min(v), 1), round(max(v), 1)] for k, v in rates.items()},
                      "over_noise_off": {k: round(v / med["off"], 4) for k, v in med.items()}}), flush=True)


if __name__ == "__main__":
    main()
