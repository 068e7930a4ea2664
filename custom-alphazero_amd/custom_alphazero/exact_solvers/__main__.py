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

`--build-book PATH --depth D [--board HxW[xN]] [--budget B] [--chunk N]
[--tt-log2 K] [--seconds S]` builds the opening book of depth D into PATH
(engine.Solver.build_book), resuming from PATH when it exists: one JSON line
per chunk (positions done, remaining, unsolved, elapsed), saved after each, and
a last line saying "finished" or "stopped" (the time was up, or the budget is
too small for what is left); exit status 0 either way.

`--book-bench [--depth D] [--sample K] [--budget B] [--tt-log2 K] [--seconds S]`
measures what a 7x6 book of depth 12 and 14 (or D) would cost: book_begin's time
and level counts, and a strided sample of the deepest level solved on a cleared
table, scaled to the whole level.
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


def build_book(path, depth, height=6, width=7, n=4, budget=1 << 26, chunk=1 << 16, tt_log2=24, seconds=None):
    """--build-book: builds the book of `depth` into `path`, resuming from the
    file when it exists; one JSON line per chunk and a last one saying whether
    the book is finished or the time was up.  -> that last line's dict."""
    import os

    from custom_alphazero import engine as az
    t0 = time.perf_counter()
    with az.Solver(height, width, n, tt_log2=tt_log2) as solver:
        resumed = os.path.isfile(path)
        if resumed:
            solver.book_load(path)
            have = solver.book_info()[0]
            if have != depth:
                raise SystemExit(f"{path} holds a book of depth {have}, not {depth}")
        else:
            solver.book_begin(depth)
        counts = solver.book_info()[2]
        print(json.dumps({"book": "levels", "board": [height, width, n], "depth": depth, "resumed": resumed,
                          "level_counts": [int(c) for c in counts], "seconds": time.perf_counter() - t0}), flush=True)

        def report(done, remaining, unsolved):
            print(json.dumps({"book": "chunk", "done": done, "remaining": remaining, "unsolved": unsolved,
                              "budget": budget, "seconds": time.perf_counter() - t0}), flush=True)

        finished = solver.build_book(depth, budget, chunk=chunk, path=path, seconds=seconds, report=report)
        depth_, state, _ = solver.book_info()
        out = {"book": "finished" if finished else "stopped", "path": path, "depth": depth_,
               "seconds": time.perf_counter() - t0}
        if finished:
            scores, status, nodes = solver.solve(np.zeros((1, height, width), np.int8), 1)
            out["empty_board_score"] = int(scores[0])
            assert status[0] == az.SOLVER_SOLVED and nodes[0] == 0
        else:
            out["why"] = "the time was up" if seconds is not None and out["seconds"] >= seconds else \
                "every position left went over the budget: raise --budget"
    print(json.dumps(out), flush=True)
    return out


def book_bench(depths=(12, 14), height=6, width=7, n=4, sample=1 << 16, budget=1 << 26, tt_log2=28, seconds=240.0,
               slices=8):
    """--book-bench: what a book of each depth would cost.  Times book_begin,
    reads an evenly strided sample of the deepest level, solves it with the
    ordinary solve on a cleared table, in `slices` interleaved parts so that the
    call can stop at `seconds`, and scales the time to the whole level (an upper
    estimate: a real build's table fills).  One JSON line per depth."""
    from custom_alphazero import engine as az
    out = []
    with az.Solver(height, width, n, tt_log2=tt_log2) as solver:
        solver.book_begin(2)  # warm-up: the first launches, the sort's code
        for depth in depths:
            t0 = time.perf_counter()
            counts = solver.book_begin(depth)
            begin_s = time.perf_counter() - t0
            level = int(counts[depth])
            take = min(sample, level)
            stride = max(1, level // take)
            boards, _ = solver.book_level(depth, 0, take, stride)
            solver.clear()
            secs, nodes, worst, unsolved, done = 0.0, 0, 0, 0, 0
            for part in range(slices):
                if secs >= seconds:
                    break
                t0 = time.perf_counter()
                _, status, nd = solver.solve(boards[part::slices], budget)
                secs += time.perf_counter() - t0
                nodes += int(nd.sum())
                worst = max(worst, int(nd.max()))
                unsolved += int((status != 0).sum())
                done += len(status)
            row = {"bench": "solver_book", "board": [height, width, n], "depth": depth, "tt_log2": tt_log2,
                   "budget": budget, "begin_s": begin_s, "level_counts": [int(c) for c in counts],
                   "sample": done, "sample_asked": take, "sample_s": secs, "sample_nodes": nodes,
                   "sample_max_nodes": worst, "sample_unsolved": unsolved,
                   "estimated_full_solve_s": secs * level / max(done, 1), "retrograde_s": "not timed"}
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


if __name__ == "__main__":
    if "--build-book" in sys.argv[1:]:
        dims = [int(v) for v in _arg("--board", "6x7x4").split("x")]
        secs = _arg("--seconds", None)
        build_book(_arg("--build-book", None), int(_arg("--depth", 14)), dims[0], dims[1],
                   dims[2] if len(dims) > 2 else 4, int(_arg("--budget", 1 << 26)), int(_arg("--chunk", 1 << 16)),
                   int(_arg("--tt-log2", 24)), None if secs is None else float(secs))
        raise SystemExit(0)
    if "--book-bench" in sys.argv[1:]:
        depth = _arg("--depth", None)
        book_bench((12, 14) if depth is None else (int(depth),), sample=int(_arg("--sample", 1 << 16)),
                   budget=int(_arg("--budget", 1 << 26)), tt_log2=int(_arg("--tt-log2", 28)),
                   seconds=float(_arg("--seconds", 240)))
        raise SystemExit(0)
    if "--bench" not in sys.argv[1:]:
        raise SystemExit("usage: python -m custom_alphazero.exact_solvers --bench [--board HxW[xN]] "
                         "[--stones LO-HI] [--count K] [--budget B] [--split S] [--steps T] [--tt L]\n"
                         "       python -m custom_alphazero.exact_solvers --build-book PATH --depth D [--board HxW[xN]] "
                         "[--budget B] [--chunk N] [--tt-log2 K] [--seconds S]\n"
                         "       python -m custom_alphazero.exact_solvers --book-bench [--depth D] [--sample K] "
                         "[--budget B] [--tt-log2 K] [--seconds S]")
    dims = [int(v) for v in _arg("--board", "6x7x4").split("x")]
    lo_hi = [int(v) for v in _arg("--stones", "14-36").split("-")]
    print(json.dumps(bench(dims[0], dims[1], dims[2] if len(dims) > 2 else 4, lo_hi[0], lo_hi[1],
                           int(_arg("--count", 4096)), int(_arg("--budget", 1 << 26)), int(_arg("--split", 0)),
                           int(_arg("--steps", 0)), int(_arg("--tt", 24)))))
