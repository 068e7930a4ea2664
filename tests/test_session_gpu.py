"""The entry rule both engines share (csrc/az_session.h, Session::enter): an
ABI call that touches engine buffers first waits for the moves an asynchronous
selfplay_step left running on the lanes' streams.  A forward, a results read
and a tree export issued right behind such a step must neither disturb the
search nor see it half done."""
import numpy as np
import pytest

import chess_forward_ref as cr
import chess_oracle as C
import forward_ref as fr
from custom_alphazero import engine as az
from test_chess_forward_layouts_gpu import SHIPPED, _batch1, _compare, make_engine
from test_forward_layouts_gpu import check_outputs

pytestmark = pytest.mark.gpu


def _by_game(parts):
    """Drained chunks -> one dict in game order; every game drained once."""
    r = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    order = np.argsort(r["game_ids"], kind="stable")
    return {k: v[order] for k, v in r.items()}


def test_chess_forward_between_asynchronous_steps():
    """selfplay_step(sync=False), at once forward(x), then selfplay_drain(),
    until the batch is done: every forward is the idle engine's bit for bit
    (and within the float64 reference's tolerance), and every game is the
    oracle's.  x alternates between 4 boards (one engine chunk, covering both
    lanes' slices of x, act, probs and values) and 6 boards (two chunks).
    Before az_chess_forward waited for the queued moves this raced -- the
    forward wrote the buffers the running simulations read -- and so failed or
    passed with the timing; with the entry guard it is deterministic."""
    d = cr.case_data(SHIPPED)
    eng = make_engine(d, slots=4, sims=8, plies=6, lanes=2)
    batches = [slice(0, 4), slice(20, 26)]  # (the second: three one-hot boards and three of arbitrary floats)
    idle = [eng.forward(d["x"][rows]) for rows in batches]
    eng.selfplay_begin(0, 8, 77)
    parts, drained = [], 0
    for move in range(40):
        if drained == 8:
            break
        rows = batches[move % 2]
        eng.selfplay_step(1, sync=False)
        p, v = eng.forward(d["x"][rows])
        parts.append(eng.selfplay_drain())
        drained += len(parts[-1]["game_ids"])
        check_outputs(d, p, v, rows, f"move {move}")
        np.testing.assert_array_equal(p, idle[move % 2][0], err_msg=f"move {move}")
        np.testing.assert_array_equal(v, idle[move % 2][1], err_msg=f"move {move}")
    st = eng.stats()
    parts.append(eng.selfplay_drain())
    r = _by_game(parts)
    assert st["errors"] == 0 and st["games_done"] == 8
    assert r["game_ids"].tolist() == list(range(8))
    cb = _batch1(eng)
    for g in range(8):
        _compare(r, g, C.play_game(8, 77 + g, 6, callback=cb), "forward between steps")
    eng.close()


def test_chess_results_and_tree_export_wait_for_an_asynchronous_step():
    """selfplay_results() and tree_export(0) right behind selfplay_step(sync=
    False) return what they return behind a synchronous step of a second
    engine with the same seeds: the calls that always waited still do."""
    kw = dict(mcts_iterations=8, slots=4, lanes=2, max_plies=6, evaluator=az.EVAL_SYNTHETIC)
    a, b = az.ChessEngine(**kw), az.ChessEngine(**kw)
    for eng in (a, b):
        eng.selfplay_begin(0, 4, 31)
    for move in range(3):
        a.selfplay_step(1, sync=False)
        ra, ta = a.selfplay_results(), a.tree_export(0)
        st = b.selfplay_step(1, sync=True)
        rb, tb = b.selfplay_results(), b.tree_export(0)
        assert st["errors"] == 0 and (rb["policy_n"][:, move] > 0).all()  # (the move's samples are there)
        assert ra.keys() == rb.keys() and ta.keys() == tb.keys()
        for k in rb:
            assert ra[k].tobytes() == rb[k].tobytes(), (move, k)
        for k in tb:
            assert np.array_equal(ta[k], tb[k]), (move, k)
    assert a.stats()["errors"] == 0
    a.close()
    b.close()


def test_connect_n_forward_between_asynchronous_steps():
    """The Connect-N engine under the same rule: with a forward between every
    asynchronous step and its drain, the games are those of synchronous steps
    with no forward, and the forwards those of the idle engine."""
    x = fr.make_batch(6, 7)
    w = fr.lively_weights(6, 7, True, 1, 256, x)

    def engine():
        eng = az.Engine(6, 7, 4, True, 8, slots=6, lanes=2, evaluator=az.EVAL_NETWORK, depth=1)
        eng.set_weights(w.items())
        return eng

    ref = engine()
    ref.selfplay_begin(0, 10, 77)
    while ref.selfplay_step(1, sync=True)["active_slots"]:
        pass
    want = _by_game([ref.selfplay_drain()])
    ref.close()

    eng = engine()
    batches = [x[:6], x[18:27]]  # one engine chunk, two chunks
    idle = [eng.forward(b) for b in batches]
    eng.selfplay_begin(0, 10, 77)
    parts, drained = [], 0
    for move in range(6 * 7 * 10):
        if drained == 10:
            break
        eng.selfplay_step(1, sync=False)
        p, v = eng.forward(batches[move % 2])
        parts.append(eng.selfplay_drain())
        drained += len(parts[-1]["game_ids"])
        np.testing.assert_array_equal(p, idle[move % 2][0], err_msg=f"move {move}")
        np.testing.assert_array_equal(v, idle[move % 2][1], err_msg=f"move {move}")
    st = eng.stats()
    parts.append(eng.selfplay_drain())
    r = _by_game(parts)
    assert st["errors"] == 0 and st["games_done"] == 10
    assert r["game_ids"].tolist() == list(range(10))
    for k, v in want.items():
        assert r[k].tobytes() == v.tobytes(), k
    eng.close()
