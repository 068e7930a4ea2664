"""The one-launch tower's two ends -- the stem's operand and the heads' dense,
softmax and tanh phases -- bit for bit against the build before they were
rescheduled: every sum keeps its operands and its order, so the outputs of
Engine.forward (uint32 views of probs and values) and of a short self-play
(the stem's Board path: moves and visit-count policies) must equal the arrays
under tests/golden/tower_ends/.

The goldens were written by this file's main() on an MI355X with the parent
commit's library (AZ_LIB_PATH=<parent libaz.so> python3
tests/test_tower_ends_gpu.py <directory>): the inputs, the lively weights of
tests/forward_ref.py and the engine settings are the ones the tests rebuild.
They are no reference for accuracy (tests/test_forward_layouts_gpu.py is):
they pin the bits.

Shapes: 6x7 at depth 1 and 2 with 1..5 boards (the 96-row tiles of two boards,
whole and partial) and at the dual launch's threshold + 1..3 boards (the
128-row tiles of three); 7x6 (the pad-filled top|bottom plan); 9x9 at 1 and 3
boards (192-row tiles in place); value hidden sizes 1, 255 and 256 (P = 512,
2, 2 partials per unit; the late wv1 copy's padding); one-hot and float planes;
the natural order against the planned one; chess at 1 and 2 boards (the
input-row form ends in the shared 1x1 phase: its per-pixel features have no
accessor, the dense heads' outputs computed from them stand in).  The Board
path again at the shapes where it differs: 6x7 depth 2 with 320 boards per
lane launch (above the threshold: the 128-row tiles), 7x6, and 9x9 (cells past
63 come from the board's second word) -- their moves and policies as SHA-256
digests beside the game lengths."""
import hashlib
import os
import sys

import numpy as np
import pytest

import conftest  # noqa: F401  (the import paths, also when run as a program)
import forward_ref as fr
from custom_alphazero import engine as az

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tower_ends")

# name -> (H, W, gravity, depth, hidden, board counts)
CONFIGS = {
    "6x7_d1_h256": (6, 7, True, 1, 256, (1, 2, 3, 4, 5)),
    "6x7_d2_h256": (6, 7, True, 2, 256, (1, 2, 3, 4, 5)),
    "6x7_d1_h1": (6, 7, True, 1, 1, (2, 5)),
    "6x7_d1_h255": (6, 7, True, 1, 255, (2, 5)),
    "7x6_d1_h256": (7, 6, True, 1, 256, (1, 2, 3)),
    "9x9_d1_h256": (9, 9, True, 1, 256, (1, 3)),
}


def _engine(name, **kw):
    H, W, grav, depth, hidden, _ = CONFIGS[name]
    w = fr.lively_weights(H, W, grav, depth, hidden, fr.make_batch(H, W))
    eng = az.Engine(H, W, min(4, H, W), grav, 8, slots=256, lanes=8, evaluator=az.EVAL_NETWORK, depth=depth,
                    value_hidden=hidden, **kw)
    eng.set_weights(w.items())
    return eng


def _forward_outputs(name, **kw):
    """key -> uint32 array: probs and values of every batch of the config."""
    H, W, _, _, _, counts = CONFIGS[name]
    x = fr.make_batch(H, W)
    eng = _engine(name, **kw)
    thr = eng.stats()["tower_small_max_boards"]
    batches = {}
    for n in counts:
        batches[f"onehot{n}"] = x[:n]
        batches[f"float{n}"] = x[-n:]  # the last four boards are float planes
    assert (thr > 0) == (H * W <= 48), thr  # boards of 33-48 cells: 96- and 128-row tiles in one dual launch
    if thr > 0:
        assert thr + 3 <= 256, thr
        for n in (thr + 1, thr + 2, thr + 3):  # the primary tiles, every remainder of three boards
            batches[f"big{n - thr}"] = x[np.arange(n) % len(x)]
    out = {"thr": np.array([thr], np.int32)}
    for key, xb in batches.items():
        p, v = eng.forward(xb)
        out[key + "_p"], out[key + "_v"] = p.view(np.uint32), v.view(np.uint32)
    assert eng.stats()["errors"] == 0
    eng.close()
    return out


def _selfplay_outputs():
    """The stem's Board path (the eval queue's boards, never x): four short games."""
    eng = _engine("6x7_d1_h256")
    eng.selfplay_run(0, 4, 31)
    r = eng.selfplay_results()
    st = eng.stats()
    eng.close()
    assert st["errors"] == 0 and st["games_done"] == 4
    return {"lengths": r["lengths"], "moves": r["moves"], "policies": r["policies"].view(np.uint64)}


# name -> (config, games = slots, lanes, sims per move)
SELFPLAY = {
    "selfplay_6x7_d2_big": ("6x7_d2_h256", 640, 2, 4),
    "selfplay_7x6_d1": ("7x6_d1_h256", 4, 1, 8),
    "selfplay_9x9_d1": ("9x9_d1_h256", 4, 1, 8),
}


def _selfplay_digest(name):
    cfg, games, lanes, sims = SELFPLAY[name]
    H, W, grav, depth, hidden, _ = CONFIGS[cfg]
    w = fr.lively_weights(H, W, grav, depth, hidden, fr.make_batch(H, W))
    eng = az.Engine(H, W, min(5 if H == 9 else 4, H, W), grav, sims, slots=games, lanes=lanes,
                    evaluator=az.EVAL_NETWORK, depth=depth, value_hidden=hidden)
    eng.set_weights(w.items())
    thr = eng.stats()["tower_small_max_boards"]
    eng.selfplay_run(0, games, 17)
    r = eng.selfplay_results()
    st = eng.stats()
    eng.close()
    assert st["errors"] == 0 and st["games_done"] == games
    if name.endswith("_big"):
        assert 0 < thr < games // lanes, thr  # a lane's first launches hold more boards than the small tiles take
    sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
    return {"lengths": r["lengths"], "moves_sha256": sha(r["moves"]), "policies_sha256": sha(r["policies"])}


def _chess_outputs():
    import chess_forward_ref as cr
    d = cr.case_data("chess_d1_h256")
    eng = az.ChessEngine(mcts_iterations=1, slots=64, evaluator=az.EVAL_NETWORK, max_plies=4, depth=1,
                         value_hidden=256)
    eng.set_weights(d["w"].items())
    out = {}
    for n in (1, 2):
        for key, xb in ((f"planes{n}", d["x"][:n]), (f"float{n}", d["x"][-n:])):
            p, v = eng.forward(xb)
            out[key + "_p"], out[key + "_v"] = p.view(np.uint32), v.view(np.uint32)
    assert eng.stats()["errors"] == 0
    eng.close()
    return out


def _load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_bits_are_the_parents(name):
    _assert_same(_forward_outputs(name), _load(name))


@pytest.mark.parametrize("name", ["6x7_d2_h256", "7x6_d1_h256", "9x9_d1_h256"])
def test_natural_order_bits_are_the_planned_orders(name):
    _assert_same(_forward_outputs(name, tower_natural_order=True), _load(name))


def test_selfplay_board_path_bits_are_the_parents():
    _assert_same(_selfplay_outputs(), _load("selfplay_6x7_d1"))


@pytest.mark.parametrize("name", list(SELFPLAY))
def test_selfplay_board_path_digests_are_the_parents(name):
    _assert_same(_selfplay_digest(name), _load(name))


def test_chess_input_row_form_bits_are_the_parents():
    _assert_same(_chess_outputs(), _load("chess_d1_h256"))


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for name in CONFIGS:
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **_forward_outputs(name))
    np.savez_compressed(os.path.join(out_dir, "selfplay_6x7_d1.npz"), **_selfplay_outputs())
    for name in SELFPLAY:
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **_selfplay_digest(name))
    np.savez_compressed(os.path.join(out_dir, "chess_d1_h256.npz"), **_chess_outputs())
    print("wrote", sorted(os.listdir(out_dir)))


if __name__ == "__main__":
    main(sys.argv[1])
