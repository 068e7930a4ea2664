"""bench.py's flagship loop (same engine arguments, same untimed rule, enqueue
move m / drain move m-1) with many timed windows in one process instead of
one: ms/step of every window, with the tower events of bench.py's window
(ev=1) and without them (ev=0), alternating -- a library's spread from one
process, for A/B runs on a box where single bench.py windows scatter.
2 x <windows> windows of <steps> moves.  Not the headline: bench.py is.
Usage: AZ_LIB_PATH=<libaz.so> python profiles/bench_windows.py <windows> <steps>"""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "custom-alphazero_amd"))
nwin, steps = int(sys.argv[1]), int(sys.argv[2])
sys.argv = [sys.argv[0], "--gpus", "1"]
import bench  # noqa: E402

args = bench.parse()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from custom_alphazero import engine as az  # noqa: E402
from custom_alphazero.model.weights import init_weights, weight_spec  # noqa: E402

spec = weight_spec(args.height, args.width, args.width, depth=args.depth)
host_w = init_weights(spec, seed=0)
dev = torch.device("cuda", 0)
named, _flat = bench._device_weights(spec, host_w, 0, 1, args, dev)
eng = az.Engine(args.height, args.width, args.n, True, args.sims, slots=args.slots,
                evaluator=az.EVAL_NETWORK, depth=args.depth, device=0,
                cache_log2=args.cache_log2, lanes=args.lanes, conv_algo=args.conv_algo,
                compact=bool(args.compact), arena_edges=bench.arena_edges_arg(args), rng_skip=args.rng_skip)
eng.set_weights(named)
total = bench.MAX_PREROLL + 2 * nwin * steps + 64
eng.selfplay_begin(first_game=0, n_games=args.slots * (2 + total // 7), base_seed=0)
t_un = time.perf_counter()
pre, ahead = 0, bench.untimed_moves_planned(args, eng.stats())
while True:
    for _ in range(ahead):
        eng.selfplay_step(1, sync=False)
        eng.selfplay_drain()
        pre += 1
    ahead = min(bench.UNTIMED_BLOCK, bench.MAX_PREROLL - pre)
    st = eng.stats()
    ok = (st["cache_inserts"] >= bench.CACHE_TURNOVER * st["cache_capacity"]
          and st["cache_entries"] >= bench.CACHE_FULL * st["cache_capacity"])
    if (pre >= bench.MIN_PREROLL and ok) or pre >= bench.MAX_PREROLL:
        break
eng.selfplay_drain()
torch.cuda.synchronize()
un = time.perf_counter() - t_un
res = {}
for ev in (0, 1, 0, 1):
    eng.timer(bool(ev), tree=False, every=1)
    for _ in range(nwin // 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.selfplay_step(1, sync=False)
            eng.selfplay_drain()
        torch.cuda.synchronize()
        eng.selfplay_drain()
        res.setdefault(ev, []).append(1e3 * (time.perf_counter() - t0) / steps)
        eng.stats()  # (collects the window's events, as bench.py's check_device does)
    eng.timer(False)
bench.check_device(eng, "windows")
tag = os.environ.get("AZ_LIB_TAG") or os.path.basename(os.path.dirname(os.environ.get("AZ_LIB_PATH", "tree/")))
for ev in (0, 1):
    v = np.array(res[ev])
    print(f"{tag} ev={ev} untimed {pre} moves {un:.2f} s | ms/step min {v.min():.3f} median {np.median(v):.3f} "
          f"max {v.max():.3f} | " + " ".join(f"{x:.2f}" for x in v), flush=True)
