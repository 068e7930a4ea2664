"""The chess replay window on the device (engine.ChessReplay, az_chess_replay_*,
csrc/az_replay.hip) and the step that trains from it (Trainer.step_replay,
az_trainer_step_replay).

The reference here is the host path the window replaces, and every comparison
is bitwise: a sample gathered from the window is the dense sample
self_play.play_chess builds (chess.kernels.encode of the same history, the
float64 policy scattered densely and cast to float32, the reward cast to
float32); a step from the window is Trainer.step on those arrays; and
train.training_loop ends in the same model with the window on the device as
with the numpy window.  Samples come from four short synthetic-evaluator chess
games (no network) and from hand-made records at the format's edges.
"""
import numpy as np
import pytest

from custom_alphazero import engine as az
from custom_alphazero.chess import kernels as K
from custom_alphazero.config import ConfigModel, ConfigPath, ConfigServing

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, momentum=0.9, l2=1e-4, bn_momentum=0.99)  # test_train_chess_gpu.py's


def _start():
    from custom_alphazero.chess.board import Board
    return Board()._pos  # host bookkeeping only


@pytest.fixture(scope="module")
def games():
    """Four synthetic self-play games: the engine's compact results, and the dense samples
    self_play.play_chess makes of them (its code, not ChessReplay's)."""
    from custom_alphazero.self_play import alternating_rewards
    eng = az.ChessEngine(8, slots=4, evaluator=az.EVAL_SYNTHETIC, max_plies=12)
    eng.selfplay_run(0, 4, 21)
    r = eng.selfplay_results()
    eng.close()
    start = _start()
    hists, valids, policies, rewards = [], [], [], []
    for g in range(4):
        T = int(r["lengths"][g])
        hist = np.zeros((T, K.HISTORY), K.POS_DTYPE)
        valid = np.zeros((T, K.HISTORY), np.uint8)
        hist[:, 7], valid[:, 7] = r["positions"][g, :T], 1
        hist[1:, 6], valid[1:, 6] = start, 1
        pol = np.zeros((T, K.ACTIONS), np.float64)
        for t in range(T):
            n = int(r["policy_n"][g, t])
            pol[t, r["policy_actions"][g, t, :n]] = r["policy_probs"][g, t, :n]
        hists.append(hist), valids.append(valid), policies.append(pol)
        rewards.append(alternating_rewards(int(r["results"][g]), T))
    hist, valid = np.concatenate(hists), np.concatenate(valids)
    out = dict(results=r, hist=hist, valid=valid, states=K.encode(hist, valid), policies=np.vstack(policies),
               rewards=np.concatenate(rewards))
    assert len(out["states"]) >= 24, "the games are too short for these tests"
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _sparse(rows):
    """[(actions, probs)] -> policy_n, policy_actions [n, 256], policy_probs [n, 256]; unused entries
    hold values a kernel reading past policy_n would trip over"""
    n = len(rows)
    pn = np.zeros(n, np.int32)
    pa = np.full((n, K.MAX_MOVES), -7, np.int16)
    pp = np.full((n, K.MAX_MOVES), np.nan, np.float64)
    for i, (a, p) in enumerate(rows):
        pn[i] = len(a)
        pa[i, :len(a)] = a
        pp[i, :len(a)] = p
    return pn, pa, pp


def _dense(rows):
    pi = np.zeros((len(rows), K.ACTIONS), np.float64)
    for i, (a, p) in enumerate(rows):
        pi[i, np.asarray(a, np.int64)] = p
    return pi.astype(np.float32)


def _numbered(n, first=0):
    """n distinguishable samples: sample i carries fullmove_number first + i + 1, one action, z = first + i"""
    hist = np.zeros((n, K.HISTORY), K.POS_DTYPE)
    valid = np.zeros((n, K.HISTORY), np.uint8)
    hist[:, 7], valid[:, 7] = _start(), 1
    hist["fullmove_number"][:, 7] = first + np.arange(n) + 1
    rows = [([(first + i) % K.ACTIONS], [0.5]) for i in range(n)]
    z = (first + np.arange(n)).astype(np.float32)
    return dict(zip(az.ChessReplay.KEYS, (hist, valid) + _sparse(rows) + (z,))), rows


def _window_is(rp, hist, valid, rows, z):
    """the whole window, oldest first, equals these samples"""
    assert len(rp) == len(z)
    x, pi, zz = rp.gather(np.arange(len(z)))
    assert np.array_equal(x, K.encode(hist, valid))
    assert np.array_equal(pi, _dense(rows))
    assert np.array_equal(zz, z)


def test_gather_is_the_host_path_bitwise(games):
    m = len(games["states"])
    rp = az.ChessReplay(m + 3)
    assert rp.capacity == m + 3 and len(rp) == 0
    rp.push_games(games["results"])
    assert len(rp) == m
    idx = np.concatenate([np.arange(m)[::-1], [0, m - 1, m - 1, 5, 5, 0]])
    x, pi, z = rp.gather(idx)
    assert x.dtype == pi.dtype == z.dtype == np.float32
    assert np.array_equal(x, games["states"][idx])
    assert np.array_equal(pi, games["policies"].astype(np.float32)[idx])
    assert np.array_equal(z, games["rewards"].astype(np.float32)[idx])
    assert pi.any(axis=1).all() and x[..., 98:111].any()  # live data, not zeros
    rp.close()


def test_hand_made_edge_records():
    start = _start()
    n = 6
    hist = np.zeros((n, K.HISTORY), K.POS_DTYPE)
    valid = np.zeros((n, K.HISTORY), np.uint8)
    hist[:, 7], valid[:, 7] = start, 1
    # 0: only the last entry valid, all four castling flags set (the start position's), an empty policy
    # 1: all 8 history entries valid, each its own position
    hist[1, :], valid[1, :] = start, 1
    hist["fullmove_number"][1] = np.arange(8) + 2
    hist["repetition"][1, ::2] = 1
    hist["turn"][1, 1::2] = 0
    # 2: repetition = 1 on the board itself; an invalid entry that holds data is still written as zeros
    hist["repetition"][2, 7] = 1
    hist[2, 3] = start
    # 3: the counters at their ends
    hist["fullmove_number"][3, 7], hist["halfmove_clock"][3, 7] = 65535, 150
    # 4: no castling rights; 5: black to move with the queen-side rights only
    hist["castling_rights"][4, 7] = 0
    hist["turn"][5, 7] = 0
    hist["castling_rights"][5, 7] = (1 << 0) | (1 << 56)
    others = np.setdiff1d(np.arange(K.ACTIONS), [0, 1879])
    full = np.concatenate([[1879, 0], np.random.RandomState(3).permutation(others)[:254]])
    assert len(np.unique(full)) == 256
    third = 1.0 / 3.0
    assert np.float64(np.float32(third)) != third  # inexact in float32: pins the rounding
    rows = [([], []),
            (full, np.random.RandomState(4).dirichlet(np.ones(256))),
            ([7, 1000], [third, 2.0 / 3.0]),
            ([1879], [1.0]),
            ([0], [0.1]),
            # a tie to even and its neighbours: 1 + 2^-24 rounds down to 1, the next float64 up to 1 + 2^-23
            ([3, 4, 5], [1.0 + 2.0 ** -24, np.nextafter(1.0 + 2.0 ** -24, 2.0), 1e-30])]
    z = np.array([1, -1, 0, 0.5, -0.25, 1], np.float32)
    rp = az.ChessReplay(n)
    rp.push(hist, valid, *_sparse(rows), z)
    x, pi, zz = rp.gather(np.arange(n))
    assert np.array_equal(x, K.encode(hist, valid))
    assert np.array_equal(pi, _dense(rows))
    assert np.array_equal(zz, z)
    # what the records were made to show
    assert not pi[0].any() and (pi[1] != 0).sum() == 256 and pi[1, 0] > 0 and pi[1, 1879] > 0
    assert pi[2, 7] == np.float32(third) and pi[5, 3] == 1.0 and pi[5, 4] == np.float32(1.0 + 2.0 ** -23)
    assert not x[0, ..., :98].any() and x[0, ..., 112:116].all()
    assert all(x[1, ..., 14 * h:14 * h + 13].any() for h in range(8))
    assert np.array_equal(x[1, 0, 0, 13:112:14], hist["repetition"][1].astype(np.float32))
    assert (x[2, ..., 111] == 1).all() and not x[2, ..., 42:56].any()
    assert (x[3, ..., 116] == 65535).all() and (x[3, ..., 117] == 150).all()
    assert not x[4, ..., 112:116].any()
    assert np.array_equal(x[5, 0, 0, 112:116], [1, 0, 1, 0])
    rp.close()


def test_ring_keeps_the_newest_in_age_order():
    a, rows_a = _numbered(5)
    b, rows_b = _numbered(5, first=5)
    rp = az.ChessReplay(7)
    rp.push(**a)
    _window_is(rp, a["hist"], a["valid"], rows_a, a["z"])
    rp.push(**b)  # wraps: the window is samples 3..9
    hist, valid = np.concatenate([a["hist"], b["hist"]])[-7:], np.concatenate([a["valid"], b["valid"]])[-7:]
    _window_is(rp, hist, valid, (rows_a + rows_b)[-7:], np.concatenate([a["z"], b["z"]])[-7:])
    rp.clear()
    assert len(rp) == 0
    rp.push(**{k: v[:2] for k, v in b.items()})  # starts at index 0 again
    _window_is(rp, b["hist"][:2], b["valid"][:2], rows_b[:2], b["z"][:2])
    rp.close()

    rp = az.ChessReplay(3)  # one push larger than the window keeps its last 3
    rp.push(**a)
    _window_is(rp, a["hist"][-3:], a["valid"][-3:], rows_a[-3:], a["z"][-3:])
    rp.push(**{k: v[:1] for k, v in b.items()})
    _window_is(rp, np.concatenate([a["hist"][-2:], b["hist"][:1]]), np.concatenate([a["valid"][-2:], b["valid"][:1]]),
               rows_a[-2:] + rows_b[:1], np.concatenate([a["z"][-2:], b["z"][:1]]))
    rp.close()

    rp = az.ChessReplay(1)
    for i in (0, 3, 4):
        rp.push(**{k: v[i:i + 1] for k, v in a.items()})
        _window_is(rp, a["hist"][i:i + 1], a["valid"][i:i + 1], rows_a[i:i + 1], a["z"][i:i + 1])
    rp.push(**a)
    _window_is(rp, a["hist"][-1:], a["valid"][-1:], rows_a[-1:], a["z"][-1:])
    rp.close()


def test_step_replay_is_step_bitwise(games):
    from custom_alphazero.model.weights import init_weights, weight_spec
    spec = weight_spec(8, 8, 1880, 128, 1, 40, 118)
    weights = init_weights(spec, seed=0, randomize_bn=True)
    m = len(games["states"])
    rp = az.ChessReplay(m)
    rp.push_games(games["results"])
    host = az.ChessTrainer(max_batch=9, depth=1, value_hidden=40)
    dev = az.ChessTrainer(max_batch=16, depth=1, value_hidden=40)  # max_batch larger than either n
    for tr in (host, dev):
        tr.set_weights(weights.items())
    # n = 9 crosses the 8-board part of the weight gradients; then one board, another index
    for idx in (np.array([m - 1, 0, 3, 3, 11, 7, 2, 20, 5]), np.array([13])):
        a = host.step(*rp.gather(idx), **HYPER)
        b = dev.step_replay(rp, idx, **HYPER)
        assert a == b and np.all(np.isfinite(a))
        for what in (az.TRAIN_WEIGHT, az.TRAIN_GRAD, az.TRAIN_MOMENTUM):
            wa, wb = host.read_all(what), dev.read_all(what)
            assert wa.keys() == wb.keys()
            for k in wa:
                assert np.array_equal(wa[k], wb[k]), (what, k)
    assert not np.array_equal(dev.read("stem.kernel"), weights["stem.kernel"])  # it did train
    for h in (host, dev, rp):
        h.close()


def test_training_loop_with_and_without_replay(games, monkeypatch, tmp_path):
    from custom_alphazero import train
    from custom_alphazero.model.policy_value import PolicyValueModel
    monkeypatch.setattr(ConfigModel, "batch_size", 8)
    monkeypatch.setattr(ConfigModel, "depth", 1)
    monkeypatch.setattr(ConfigServing, "minimum_training_size", 8)
    monkeypatch.setattr(ConfigServing, "samples_queue_size", 20)
    monkeypatch.setattr(ConfigServing, "training_loop_sleep_time", 0)
    monkeypatch.setattr(ConfigServing, "model_checkpoint_frequency", 1000)
    monkeypatch.setattr(ConfigServing, "model_evaluation_frequency", 1000)
    monkeypatch.setattr(ConfigPath, "results_dir", str(tmp_path))
    records = az.chess_replay_records(games["results"])
    chunks = [slice(0, 9), slice(9, 17), slice(17, 24)]  # 9, 17, then 24 > 20: the window drops its oldest 4
    dense = [(games["states"][c], games["policies"][c], games["rewards"][c]) for c in chunks]
    compact = [{k: v[c] for k, v in records.items()} for c in chunks]

    def queue(items, empty):
        it = iter(items)
        return lambda: next(it, empty)

    models = []
    for replay in (None, az.ChessReplay(ConfigServing.samples_queue_size)):
        model = PolicyValueModel((8, 8, 118), 1880, seed=1)
        np.random.seed(11)
        if replay is None:
            train.training_loop("replay_test", queue(dense, (np.empty(0),) * 3), max_iterations=3, model=model)
        else:
            train.training_loop("replay_test", queue(compact, None), max_iterations=3, model=model, replay=replay)
            assert len(replay) == 20
            x, pi, _ = replay.gather(np.arange(20))  # the numpy window's rows: samples 4..23
            assert np.array_equal(x, games["states"][4:24])
            assert np.array_equal(pi, games["policies"][4:24].astype(np.float32))
            replay.close()
        models.append(model)
    a, b = models
    assert a.steps == b.steps == 3
    wa, wb = a.get_weights(), b.get_weights()
    assert len(wa) == len(wb) and all(np.array_equal(p, q) for p, q in zip(wa, wb))
    fresh = PolicyValueModel((8, 8, 118), 1880, seed=1)
    assert not all(np.array_equal(p, q) for p, q in zip(wa, fresh.get_weights()))


def test_errors_leave_the_replay_and_the_trainer_usable(games):
    from custom_alphazero.model.weights import init_weights, weight_spec
    with pytest.raises(az.AzError, match="error -1.*capacity"):
        az.ChessReplay(0)
    a, rows = _numbered(4)
    rp = az.ChessReplay(6)
    tr = az.ChessTrainer(max_batch=2, depth=1, value_hidden=40)
    with pytest.raises(az.AzError, match="error -3.*no weights"):  # AZ_E_STATE: before set_weights
        tr.step_replay(rp, [0], 1e-2)
    tr.set_weights(init_weights(weight_spec(8, 8, 1880, 128, 1, 40, 118), seed=0, randomize_bn=True).items())
    with pytest.raises(az.AzError, match="error -3.*empty"):  # AZ_E_STATE: an empty window
        rp.gather([0])
    with pytest.raises(az.AzError, match="error -3.*empty"):
        tr.step_replay(rp, [0], 1e-2)
    rp.push(**a)

    def refused(**change):
        bad = {k: v.copy() for k, v in a.items()}
        for k, (where, value) in change.items():
            bad[k][where] = value
        with pytest.raises(az.AzError, match="error -1"):
            rp.push(**bad)
        _window_is(rp, a["hist"], a["valid"], rows, a["z"])  # nothing was copied

    refused(policy_actions=((2, 0), 1880))
    refused(policy_actions=((3, 0), -1))
    refused(policy_n=(1, 2), policy_actions=((1, 1), a["policy_actions"][1, 0]))  # a repeated action
    refused(policy_n=(0, 257))
    refused(policy_n=(3, -1))
    for bad in ([-1], [4], [0, 4]):  # 4 == size
        with pytest.raises(az.AzError, match="error -1.*index"):
            rp.gather(bad)
        with pytest.raises(az.AzError, match="error -1.*index"):
            tr.step_replay(rp, bad, 1e-2)
    with pytest.raises(az.AzError, match="error -1.*max_batch"):  # n > max_batch
        tr.step_replay(rp, [0, 1, 2], 1e-2)
    with pytest.raises(az.AzError, match="error -1.*max_batch"):  # n = 0
        tr.step_replay(rp, [], 1e-2)
    connect = az.Trainer(6, 7, True, max_batch=2, depth=1)
    with pytest.raises(az.AzError, match="error -1.*chess"):
        connect.step_replay(rp, [0], 1e-2)
    connect.close()
    # all of it refused: the window and the trainer are what they were, and work
    _window_is(rp, a["hist"], a["valid"], rows, a["z"])
    before = tr.read("stem.kernel")
    losses = tr.step_replay(rp, [3, 0], **HYPER)
    assert np.all(np.isfinite(losses)) and not np.array_equal(tr.read("stem.kernel"), before)
    rp.push(**a)
    assert len(rp) == 6
    tr.close()
    rp.close()
