"""`python -m custom_alphazero.exact_solvers --bench` times the device solver
(engine.Solver) on seeded random-playout positions and prints one JSON line
per case: positions solved per second and search nodes per second, each the
median of three runs around the synchronous call (host clock), after a
warm-up call; the table is cleared before every run.

  --board HxW[xN]   (default 6x7x4: H rows, W columns)
  --stones LO-HI    stones on the sampled positions (default 14-36)
  --count K         positions per call (default 4096)
  --budget B        node budget per position (default 2^26)
  --split S --steps T --tt L   az_solver_configure / tt_log2 (defaults: the library's, 24)
"""
import json
import sys
import time

import numpy as np


def random_positions(height, width, n, count, lo, hi, seed=0):
    """Seeded random playouts stopped at lo..hi stones, unfinished; +1 the side to move."""
    from custom_alphazero.config import ConfigConnectN
    from custom_alphazero.connect_n.board import Board
    saved = (ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity)
    ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity = \
        height, width, n, True
    try:
        rng = np.random.RandomState(seed)
        out = []
        while len(out) < count:
            target = int(rng.randint(lo, hi + 1))
            board = Board()
            while board.fullmove_number < target and not board.is_game_over():
                moves = board.moves
                board.play(moves[int(rng.randint(len(moves)))], keep_same_player=True)
            if not board.is_game_over():
                out.append(board.array.copy())
        return np.stack(out)
    finally:
        (ConfigConnectN.board_height, ConfigConnectN.board_width, ConfigConnectN.n, ConfigConnectN.gravity) = saved


def bench(height=6, width=7, n=4, lo=14, hi=36, count=4096, budget=1 << 26, split=0, steps=0, tt_log2=24,
          runs=3):
    from custom_alphazero import engine as az
    boards = random_positions(height, width, n, count, lo, hi)
    with az.Solver(height, width, n, tt_log2=tt_log2) as solver:
        solver.configure(split_stones=split, steps_per_launch=steps)
        solver.solve(boards[:64], budget)  # warm-up: the first launch, the allocations
        secs, nodes, unsolved = [], [], []
        for _ in range(runs):
            solver.clear()
            t0 = time.perf_counter()
            _, status, nd = solver.solve(boards, budget)
            secs.append(time.perf_counter() - t0)
            nodes.append(int(nd.sum()))
            unsolved.append(int((status != 0).sum()))
    k = int(np.argsort(secs)[len(secs) // 2])
    return {"bench": "solver", "board": [height, width, n], "stones": [lo, hi], "positions": count,
            "budget": budget, "split_stones": split, "steps_per_launch": steps, "tt_log2": tt_log2,
            "seconds": secs[k], "positions_per_s": count / secs[k], "nodes": nodes[k],
            "nodes_per_s": nodes[k] / secs[k], "unsolved": unsolved[k], "runs_s": secs}


def _arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


if __name__ == "__main__":
    if "--bench" not in sys.argv[1:]:
        raise SystemExit("usage: python -m custom_alphazero.exact_solvers --bench [--board HxW[xN]] "
                         "[--stones LO-HI] [--count K] [--budget B] [--split S] [--steps T] [--tt L]")
    dims = [int(v) for v in _arg("--board", "6x7x4").split("x")]
    lo_hi = [int(v) for v in _arg("--stones", "14-36").split("-")]
    print(json.dumps(bench(dims[0], dims[1], dims[2] if len(dims) > 2 else 4, lo_hi[0], lo_hi[1],
                           int(_arg("--count", 4096)), int(_arg("--budget", 1 << 26)), int(_arg("--split", 0)),
                           int(_arg("--steps", 0)), int(_arg("--tt", 24)))))
