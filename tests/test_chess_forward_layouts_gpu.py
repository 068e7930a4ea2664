"""The chess inference forward against the float64 restatement with lively
heads and a batch that feeds all 118 planes (tests/chess_forward_ref.py: the
case table, and per case a tolerance an eighth of what the mildest of seven
mutants does -- DESIGN section 3 has the measured errors), with every conv
algorithm; batch invariance across tiles and engine chunks; the same bits at
every launch size around the kernels' switches (64- / 128-row tower tiles, the
policy dense's two forms, the tail's grid stride, the per-layer chain's tile
tiers); and the search's own input path -- the tower's in-stem leaf encode,
the chain's encode_queue_kernel rows -- by oracle replay."""
import numpy as np
import pytest

import chess_forward_ref as cr
import chess_oracle as C
from custom_alphazero import engine as az
from test_chess_selfplay_gpu import _compare
from test_chess_tree_gpu import ROOTS, _check_root
from test_forward_layouts_gpu import check_outputs

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in cr.CASES]
ALGOS = {"tower": az.CONV_F16X2, "direct": az.CONV_DIRECT, "layers": az.CONV_F16X2_LAYERS}
SHIPPED, SMALL_HIDDEN = "chess_d4_h256", "chess_d2_h100"


def make_engine(d, algo="tower", slots=64, sims=1, plies=4, **kw):
    c = d["case"]
    eng = az.ChessEngine(mcts_iterations=sims, slots=slots, evaluator=az.EVAL_NETWORK, max_plies=plies, depth=c.depth,
                         value_hidden=c.hidden, conv_algo=ALGOS[algo], **kw)
    eng.set_weights(d["w"].items())
    return eng


@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("name", NAMES)
def test_chess_forward_case_matches_float64(name, algo):
    d = cr.case_data(name)
    eng = make_engine(d, algo)
    p, v = eng.forward(d["x"])
    st = eng.stats()
    eng.close()
    check_outputs(d, p, v, slice(None), algo)
    assert st["errors"] == 0
    if algo == "tower":  # the engine runs the tower the chooser lays out (self-play's stem: two input chunks)
        L = cr.layouts()[name]
        assert L["tower"] and st["issued_flop_per_board"] == L["flop_chunks2"], (st["issued_flop_per_board"], L)
    else:
        assert st["issued_flop_per_board"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_chess_forward_case_is_batch_invariant(name):
    """One board, three boards that start in the middle of a two-board tile,
    the whole batch, and the batch in engine chunks of 8: the same bits per
    board."""
    d = cr.case_data(name)
    x = d["x"]
    for algo in ALGOS:
        eng = make_engine(d, algo)
        p, v = eng.forward(x)
        for lo, hi in ((0, 1), (3, 6)):
            q, u = eng.forward(x[lo:hi])
            np.testing.assert_array_equal(q, p[lo:hi], err_msg=f"{algo} [{lo}:{hi}]")
            np.testing.assert_array_equal(u, v[lo:hi], err_msg=f"{algo} [{lo}:{hi}]")
        assert eng.stats()["errors"] == 0
        eng.close()
        eng = make_engine(d, algo, slots=8)
        q, u = eng.forward(x)
        assert eng.stats()["errors"] == 0
        eng.close()
        np.testing.assert_array_equal(q, p, err_msg=f"{algo} chunks of 8")
        np.testing.assert_array_equal(u, v, err_msg=f"{algo} chunks of 8")


# n boards in one launch (an engine of 2056 slots).  Above 256 the policy dense takes 32 boards a workgroup
# instead of 8 (partial groups, clamped feature reads); from 512 the tower runs 128-row tiles of two boards
# instead of 64-row tiles of one (an odd n: the last tile half empty); past 2048 heads_tail_kernel strides its
# grid; the per-layer chain's conv16 tiles grow above 384 and above 1024 boards
SIZES = {"tower": (2, 255, 256, 257, 384, 385, 511, 512, 513, 1024, 1025, 2048, 2053),
         "layers": (2, 256, 257, 384, 385, 1024, 1025, 2048, 2053),
         "direct": (2, 255, 257, 2053)}


@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("name", [SHIPPED, SMALL_HIDDEN])
def test_chess_forward_bits_do_not_depend_on_launch_size(name, algo):
    d = cr.case_data(name)
    x = d["x"]
    eng = make_engine(d, algo, slots=2056, lanes=1)
    p29, v29 = eng.forward(x)
    for n in SIZES[algo]:
        rows = (np.arange(n) * 7 + 3) % len(x)
        p, v = eng.forward(x[rows])
        np.testing.assert_array_equal(p, p29[rows], err_msg=f"{algo} n = {n}")
        np.testing.assert_array_equal(v, v29[rows], err_msg=f"{algo} n = {n}")
    assert eng.stats()["errors"] == 0
    eng.close()
    check_outputs(d, p, v, rows, f"{algo}-{n}")


def _batch1(eng):
    """callback(pos, initial) of the chess oracle: the engine's batch-1 forward
    on the reference's full_state; .seen: (position, initial) -> its outputs."""
    seen = {}

    def cb(pos, initial):
        key = (pos.tobytes(), int(initial))
        if key not in seen:
            x = C.full_state(*C.reference_history(pos, bool(initial)), pos)[None].astype(np.float32)
            p, v = eng.forward(x)
            seen[key] = (p[0], float(v[0]))
        return seen[key]

    cb.seen = seen
    return cb


@pytest.mark.parametrize("cfg", [
    ("tower", dict(slots=3)),             # 64-row tiles; the leaves' planes 64-117 built in the stem, first_chunk 2
    ("tower", dict(slots=640, lanes=1)),  # the 128-row two-board tiles (n_max = 640) with a device count of 3
    ("tower", dict(slots=64, lanes=2, cache_log2=18)),
    ("layers", dict(slots=3)),            # encode_queue_kernel's rows, conv16 with first_chunk 2
], ids=["tower-3", "tower-640", "tower-cache", "layers-3"])
def test_chess_selfplay_replays_on_oracle_with_lively_weights(cfg):
    """Self-play never reads x: the oracle, fed the engine's own batch-1
    forward of every position it asks about, reproduces every move, position,
    policy and expansion count bit for bit -- with heads whose priors and
    values depend on the board."""
    algo, kw = cfg
    d = cr.case_data(SHIPPED)
    eng = make_engine(d, algo, sims=16, plies=12, **kw)
    st = eng.selfplay_run(0, 3, 77)
    r = eng.selfplay_results()
    assert st["errors"] == 0 and st["games_done"] == 3
    if "cache_log2" in kw:
        assert st["evaluations"] + st["cache_hits"] < st["expansions"]
    cb = _batch1(eng)
    for g in range(3):
        _compare(r, g, C.play_game(16, 77 + g, 12, callback=cb), f"{algo} {kw}")
    values = {v for _, v in cb.seen.values()}
    assert len(cb.seen) > 100 and len(values) > len(cb.seen) // 2, (len(values), len(cb.seen))  # the value head is live
    eng.close()


def test_chess_tree_root_history_form_with_lively_weights():
    """tree_reset on a root that is not the start position: its history is
    [0 x 7, start-position state] (`initial`), its children's [0 x 6, start,
    cur] -- priors and W of the root's edges bitwise the oracle's."""
    d = cr.case_data(SHIPPED)
    eng = make_engine(d, slots=2, sims=24, plies=64, arena_edges=50_000)
    cb = _batch1(eng)
    roots = [C.from_fen(ROOTS[1]), C.from_fen(ROOTS[0])]
    eng.tree_reset([0, 1], np.array(roots, C.POS_DTYPE))
    trees = [C.Tree(r, callback=cb) for r in roots]
    eng.tree_search(24)
    for s, tr in enumerate(trees):
        tr.search(24)
        _check_root(eng, s, tr, s)
    assert any(initial for _, initial in cb.seen) and not all(initial for _, initial in cb.seen)
    assert len({v for _, v in cb.seen.values()}) > len(cb.seen) // 2
    assert eng.stats()["errors"] == 0
    eng.close()
