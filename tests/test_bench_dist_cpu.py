"""bench.py's N>1 glue at world size 2 over gloo on the CPU: the weight
broadcast (_device_weights), the max/sum reductions of the timing and the
counters (_reduce), and the window games' gather to rank 0 (WindowGames +
distributed.gather_games) -- the same functions bench.main runs per rank,
fed with drained-game records of the engine's layout (selfplay_drain).
The GPU side of the same path is tests/test_distributed_gpu.py."""
import argparse
import importlib.util
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 6, 7


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _drained(rank, step, n):
    """n finished games as selfplay_drain returns them (leading game axis,
    padded to H*W plies); contents tagged by (rank, step, game)."""
    P = H * W
    rng = np.random.RandomState(1000 * rank + step)
    lengths = rng.randint(7, P + 1, n).astype(np.int32)
    out = dict(game_ids=np.arange(n, dtype=np.int64) + 100 * rank + 10 * step,
               lengths=lengths, results=rng.randint(-1, 2, n).astype(np.int32),
               expansions=rng.randint(1, 5000, n).astype(np.int32),
               boards=np.zeros((n, P, H, W), np.int8), policies=np.zeros((n, P, W)),
               moves=np.zeros((n, P), np.int32))
    for g in range(n):
        T = lengths[g]
        out["boards"][g, :T] = rng.randint(-1, 2, (T, H, W))
        out["policies"][g, :T] = rng.dirichlet(np.ones(W), T)
        out["moves"][g, :T] = rng.randint(0, W, T)
    return out


def _worker(rank, world, port, outdir):
    import torch
    import torch.distributed as dist
    bench = _bench()
    from custom_alphazero import distributed as D
    from custom_alphazero.model.weights import init_weights, weight_spec
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    args = argparse.Namespace(dist_backend="gloo")
    dev = torch.device("cpu")

    spec = weight_spec(H, W, W, depth=1)
    host_w = init_weights(spec, seed=0) if rank == 0 else init_weights(spec, seed=123)
    named, flat = bench._device_weights(spec, host_w, rank, world, args, dev)
    ref = init_weights(spec, seed=0)
    for (name, t), (n2, shape) in zip(named, spec):
        assert name == n2
        np.testing.assert_array_equal(t.numpy(), ref[name].reshape(-1))

    (el,) = bench._reduce([1.5 + rank], dist.ReduceOp.MAX, world, args, dev)
    assert el == 1.5 + world - 1
    tot = bench._reduce([rank + 1, 10], dist.ReduceOp.SUM, world, args, dev)
    assert tot == [world * (world + 1) / 2, 10 * world]

    window = bench.WindowGames()
    for step, n in enumerate((2, 0, 3 + rank)):  # a step that drained nothing is skipped
        window.add(_drained(rank, step, n))
    g = D.gather_games(window.results(), device=None)
    if rank == 0:
        np.savez(os.path.join(outdir, "gathered.npz"), **g)
    dist.barrier()
    dist.destroy_process_group()


def test_bench_glue_world2(tmp_path):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, start_method="spawn")
    got = dict(np.load(tmp_path / "gathered.npz"))
    bench = _bench()
    from custom_alphazero import distributed as D
    expect = []
    for r in range(world):
        w = bench.WindowGames()
        for step, n in enumerate((2, 0, 3 + r)):
            w.add(_drained(r, step, n))
        expect.append(D._pack(w.results()))
    for k in ("lengths", "results", "expansions", "boards", "policies", "moves"):
        np.testing.assert_array_equal(got[k], np.concatenate([e[k] for e in expect]), err_msg=k)
    assert len(got["lengths"]) == 2 + 3 + 2 + 4
    # and the gathered games expand to the reference's sample layout
    states, pol, rew = D.to_samples(got)
    assert states.shape == (int(got["lengths"].sum()), H, W, 4) and len(rew) == len(pol) == len(states)


def test_bench_refuses_a_mislabelled_world():
    """--gpus N is authoritative: under a launcher whose WORLD_SIZE differs,
    bench.py exits non-zero before touching the GPU or printing a line."""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=120, cwd=REPO, env=env)
    assert r.returncode == 2 and "WORLD_SIZE=3" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_launch_command_for_n_ranks(monkeypatch):
    """Without a launcher and N > 1, bench.py starts N ranks itself: one
    torch.distributed.run child on 127.0.0.1 with the same arguments."""
    import subprocess
    bench = _bench()
    seen = {}

    class Done:
        returncode = 0

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(subprocess, "run", fake_run)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    args = argparse.Namespace(gpus=4)
    assert bench.launch_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # one rank, or already under a launcher with the same world: run in-process
    assert bench.launch_ranks(argparse.Namespace(gpus=1)) is None
    monkeypatch.setenv("WORLD_SIZE", "4")
    assert bench.launch_ranks(args) is None


def test_bench_refuses_more_ranks_than_gpus(monkeypatch):
    """One rank per GPU: a world larger than the visible devices exits with
    status 2 before any GPU call (unless --share-devices asks for a
    rehearsal that shares them)."""
    import torch
    bench = _bench()
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    with pytest.raises(SystemExit) as ex:
        bench.check_devices(argparse.Namespace(share_devices=False), 4)
    assert ex.value.code == 2
    assert bench.check_devices(argparse.Namespace(share_devices=True), 4) == 2
    assert bench.check_devices(argparse.Namespace(share_devices=False), 2) == 2


def test_roofline_traffic_only_from_the_same_build(tmp_path):
    """the line's PMC traffic and MFMA-busy fraction come
    from a profile that recorded the libaz build it measured; a profile of
    another build yields null with the reason."""
    import json
    from custom_alphazero import engine as az
    bench = _bench()
    build, _ = az.build_id()
    entry = {"boards_per_launch": 672, "mean_hbm_bytes_per_board_per_launch": 1000.0, "mfma_busy": 0.5}
    f = tmp_path / "pmc.json"
    args = argparse.Namespace()
    for bid, want in ((build, 672 * 1000), ("0123456789abcdef", None)):
        f.write_text(json.dumps({"build_id": bid, "tower16": entry}))
        r = bench.conv_roofline(args, 0, 1, 672.0, 0.2, 10.0, 6720, 10, 104.6e6, 270.5e6, str(f), "tower16")
        assert r["traffic"] == want, r["pmc"]
        assert r["mfma_busy"] == (0.5 if want else None)
        assert r["build_id"] == build
    r = bench.conv_roofline(args, 0, 1, 672.0, 0.2, 10.0, 6720, 10, 104.6e6, 270.5e6, str(tmp_path / "no"), "tower16")
    assert r["traffic"] is None and "no PMC profile" in r["pmc"]


def test_tree_arena_rule_states_the_pool_it_holds():
    """the line's arena rule is the size the pools hold --
    per slot, the pools' edges over both halves and all slots, not the
    requested average (a lane half is also capped at 2^31 - 1 edges)."""
    bench = _bench()
    args = argparse.Namespace(width=7, height=6, sims=100, slots=4096, compact=True, lanes=0,
                              arena_edges="proof")
    safe = 100 * 42 * 7 + 7
    st = dict(arena_edges=safe, arena_pool_edges=2 * 4096 * safe, arena_pool_high=10, max_retained=5)
    r = bench.tree_arena(args, st, 2)
    assert r["overflow_proof"] and r["pool_edges_per_half_per_slot"] == safe and "no game can overflow" in r["rule"]
    capped = dict(st, arena_pool_edges=2 * 2 * ((1 << 31) - 1))  # two lanes, each half at the index cap
    args.slots, args.sims = 65536, 400
    r = bench.tree_arena(args, capped, 2)
    assert not r["overflow_proof"] and r["pool_edges_per_half_per_slot"] == 2 * ((1 << 31) - 1) // 65536
    assert "share the pool" in r["rule"]


def test_bounded_arena_is_sized_from_the_measured_high_water_mark():
    """--arena-edges bounded (the default) asks for
    8*S*A + H*W*A edges per slot -- 5,894 at configs[1], ~5.8x the 1,020 per
    slot a lane half held at its high-water mark in round 4 -- instead of
    the overflow-proof 29,407; the line states the pool and the fraction the
    window's high-water mark used."""
    bench = _bench()
    args = argparse.Namespace(width=7, height=6, sims=100, slots=4096, compact=True, lanes=0,
                              arena_edges="bounded")
    assert bench.arena_edges_arg(args) == 8 * 100 * 7 + 42 * 7 == 5894
    assert bench.arena_edges_arg(argparse.Namespace(**dict(vars(args), arena_edges="proof"))) == 0
    assert bench.arena_edges_arg(argparse.Namespace(**dict(vars(args), arena_edges="1234"))) == 1234
    st = dict(arena_edges=5894, arena_pool_edges=2 * 4096 * 5894, arena_pool_high=2_090_000, max_retained=2485)
    r = bench.tree_arena(args, st, 2)
    assert not r["overflow_proof"] and r["sizing"] == "bounded"
    assert r["lane_half_edges"] == 2048 * 5894 and r["high_water_fraction"] == round(2_090_000 / (2048 * 5894), 4)
    assert "measured high-water mark" in r["rule"]


def test_dump_outputs_orders_by_game_id_and_zeroes_rows_past_the_game(tmp_path):
    """--dump-outputs: one float .npy per drained array, rows ordered by game
    id whatever order the drains delivered them in, rows past a game's length
    zero; how the games were split over the window's drains changes nothing."""
    bench = _bench()
    a, b = _drained(0, 1, 5), _drained(0, 2, 4)
    for d in (a, b):  # rows past the end hold whatever the buffer held
        for g, T in enumerate(d["lengths"]):
            d["policies"][g, T:] = 7.0
            d["moves"][g, T:] = 3
    w1, w2 = bench.WindowGames(), bench.WindowGames()
    for d in (b, a):
        w1.add(d)
    w2.add({k: np.concatenate([a[k], b[k][:1]]) for k in a})
    w2.add({k: v[:0] for k, v in a.items()})
    w2.add({k: v[1:] for k, v in b.items()})
    r1 = bench.dump_outputs(str(tmp_path / "one"), w1.drained())
    r2 = bench.dump_outputs(str(tmp_path / "two"), w2.drained())
    assert r1["games"] == r1["of"] == 9 and r1["arrays"] == r2["arrays"] == sorted(a)
    ref = {k: np.concatenate([a[k], b[k]]) for k in a}
    assert np.all(np.diff(ref["game_ids"]) > 0)
    for k in ref:
        x, y = np.load(tmp_path / "one" / f"{k}.npy"), np.load(tmp_path / "two" / f"{k}.npy")
        assert x.dtype == (np.float64 if ref[k].dtype.itemsize == 8 else np.float32), k
        assert x.tobytes() == y.tobytes() and x.shape == ref[k].shape, k
    pol, mov = np.load(tmp_path / "one" / "policies.npy"), np.load(tmp_path / "one" / "moves.npy")
    for g, T in enumerate(ref["lengths"]):
        np.testing.assert_array_equal(pol[g, :T], ref["policies"][g, :T])
        np.testing.assert_array_equal(mov[g, :T], ref["moves"][g, :T])
        assert not pol[g, T:].any() and not mov[g, T:].any()
    assert r1["bytes"] == sum(np.load(tmp_path / "one" / f).nbytes for f in os.listdir(tmp_path / "one"))


def test_dump_outputs_keeps_a_seeded_sample_under_the_size_limit(tmp_path, monkeypatch):
    """Above the limit the dump keeps a sample of the games that depends only
    on how many there are; an empty window writes empty arrays."""
    bench = _bench()
    games = _drained(0, 3, 40)
    per_game = sum(np.zeros(v.shape[1:], np.float64 if v.dtype.itemsize == 8 else np.float32).nbytes
                   for v in games.values())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * per_game + 5)
    shuffled = {k: v[::-1] for k, v in games.items()}
    r1 = bench.dump_outputs(str(tmp_path / "a"), games)
    r2 = bench.dump_outputs(str(tmp_path / "b"), shuffled)
    assert r1["games"] == r2["games"] == 10 and r1["of"] == 40 and r1["bytes"] <= bench.DUMP_MAX_BYTES
    ids = np.load(tmp_path / "a" / "game_ids.npy")
    assert np.all(np.diff(ids) > 0) and set(ids) <= set(games["game_ids"])
    for k in games:
        assert np.load(tmp_path / "a" / f"{k}.npy").tobytes() == np.load(tmp_path / "b" / f"{k}.npy").tobytes()
    r0 = bench.dump_outputs(str(tmp_path / "none"), {k: v[:0] for k, v in games.items()})
    assert r0["games"] == 0 and np.load(tmp_path / "none" / "boards.npy").shape == (0, H * W, H, W)
    assert bench.DUMP_MAX_BYTES == 10 * per_game + 5 and _bench().DUMP_MAX_BYTES == 64 << 20


def test_dump_outputs_writes_packed_chess_positions_as_bytes(tmp_path):
    """The chess drain's arrays: the 80-byte position records are written as
    their bytes, rows follow the game ids, plies past a game's length are zero."""
    from custom_alphazero.chess.kernels import MAX_MOVES, POS_DTYPE
    bench = _bench()
    G, P = 4, 3
    g = dict(game_ids=np.array([3, 1, 2, 0], np.int64), lengths=np.array([3, 2, 3, 1], np.int32),
             results=np.zeros(G, np.int32), terminations=np.zeros(G, np.int32), expansions=np.ones(G, np.int32),
             positions=np.zeros((G, P), POS_DTYPE), moves=np.ones((G, P), np.uint16),
             policy_n=np.full((G, P), 20, np.int32), policy_actions=np.ones((G, P, MAX_MOVES), np.int16),
             policy_probs=np.full((G, P, MAX_MOVES), 0.5))
    g["positions"]["turn"] = 1 + np.arange(G)[:, None]
    r = bench.dump_outputs(str(tmp_path), g)
    assert r["games"] == 4 and r["arrays"] == sorted(g)
    pos = np.load(tmp_path / "positions.npy")
    assert pos.shape == (G, P, 80) and pos.dtype == np.float32
    turn_byte = POS_DTYPE.fields["turn"][1]
    lengths = np.load(tmp_path / "lengths.npy").astype(int)
    assert list(lengths) == [1, 2, 3, 3]  # game ids 0, 1, 2, 3
    assert list(pos[:, 0, turn_byte]) == [4, 2, 3, 1]
    probs = np.load(tmp_path / "policy_probs.npy")
    for i, T in enumerate(lengths):
        assert probs[i, :T].all() and not probs[i, T:].any() and not pos[i, T:].any()


def test_untimed_moves_are_a_function_of_the_arguments():
    """The number of untimed moves comes from the arguments alone (the timed
    steps then start from the same position in every run): at least
    max(--warmup, MIN_PREROLL) and, with the cache on, UNTIMED_PER_TURNOVER
    x capacity / (slots x sims), capped at MAX_PREROLL; the cache's counters,
    which vary from run to run, do not enter."""
    bench = _bench()
    args = argparse.Namespace(warmup=5, cache_log2=26, slots=4096, sims=100)
    st = dict(cache_gen_size=1 << 22, cache_capacity=1 << 26, cache_inserts=0, cache_entries=0)
    n = bench.untimed_moves_planned(args, st)
    assert n == 1262 == -(-int(bench.UNTIMED_PER_TURNOVER * (1 << 26)) // (4096 * 100))
    assert bench.untimed_moves_planned(args, dict(st, cache_inserts=3 << 26, cache_entries=1 << 26)) == n
    # configs[1]'s rule (CACHE_FULL, CACHE_TURNOVER) first held at move 1234-1235: inside the plan
    assert 1235 < n < 1300
    assert bench.untimed_moves_planned(argparse.Namespace(**dict(vars(args), warmup=2000)), st) == 2000
    assert bench.untimed_moves_planned(argparse.Namespace(**dict(vars(args), cache_log2=0)), st) == bench.MIN_PREROLL
    assert bench.untimed_moves_planned(args, dict(st, cache_gen_size=0)) == bench.MIN_PREROLL  # a table that only fills
    small = argparse.Namespace(warmup=60, cache_log2=14, slots=256, sims=16)
    assert bench.untimed_moves_planned(small, dict(st, cache_capacity=1 << 14)) == 60
    assert bench.untimed_moves_planned(argparse.Namespace(**dict(vars(args), slots=8, sims=16)), st) == bench.MAX_PREROLL


def test_plain_run_options(monkeypatch):
    """--full is off by default; --dump-outputs takes the directory."""
    bench = _bench()
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "somewhere" and a.steps == 30
