"""Reference side of the chess forward's shape tests (TEST INFRASTRUCTURE):
tests/forward_ref.py's restatement, lively heads and mutants on the chess
network (8 x 8 x 118 planes, 1880 actions).

  chess_batch     29 boards in which every one of the 118 planes is live:
                  Board.full_state of eight-step histories from the chess
                  oracle, two boards in the search's own forms, and last
                  boards of floats that fp16 cannot hold
  lively_chess_weights  forward_ref's calibration with 118 input planes
  mutants         forward_ref's M1..M5 and two that only chess can suffer
                  (M6, M7 below)
  CASES           the (depth, hidden) table
  case_data       everything of one case, computed once per process

Nothing here touches libaz (layouts() runs the layout check program against
it, as forward_ref.layouts() does)."""
import collections
import functools
import json
import tempfile

import numpy as np

import chess_oracle as C
import forward_ref as fr

PLANES, ACTIONS = 118, 1880
BATCH = fr.BATCH
N_FLOAT = 6  # the last boards: arbitrary floats

Case = collections.namedtuple("ChessCase", "name depth hidden seed")


def _case(depth, hidden, seed=0):
    return Case(f"chess_d{depth}_h{hidden}", depth, hidden, seed)


# what each row is in the table for (tests/test_chess_forward_cases_cpu.py asserts the layout of each
# against the library's chooser: 128-row tiles of two boards, double-buffered, at every depth)
CASES = [
    _case(4, 256),          # the shipped network
    # (depths 1 and 2 with seed 2.  Seed 0 leaves the last policy feature all but dead at depth 1 -- M5 moves
    # the policy 1.1e-5, tol_p 6.6 e32 -- and ReLU-dead on all 29 boards at depth 2 -- M5 exactly 0 -- where
    # at hidden 1 its one dense1 unit is alive on 2 boards; seed 1 leaves the value conv dead on the float
    # boards at depth 2 -- M7 exactly 0 on the value)
    _case(1, 256, 2),       # one block: the last conv2's head epilogue follows the stem directly
    _case(2, 1, 2),         # hidden = 1: one live thread in the tail's value layer
    _case(2, 100, 2),       # t < hidden guards, 156 idle tail threads
    _case(2, 255, 2),       # one idle tail thread, wv1 rows that are no multiple of 4 floats
    _case(2, 300, 2),       # the tail's loop form (hidden > 256); tower16_heads_fit does not apply: still the tower
    _case(16, 256),         # the blob prefix at its largest (what is left of the LDS: 1672 bytes)
]
CASE_BY_NAME = {c.name: c for c in CASES}

# planes 14 h + 0..12 one-hot pieces of history step h, 14 h + 13 its repetition count; 112..115
# castling rights, 116 the full-move number, 117 the half-move clock (Board.full_state)
PLANE_RANGE = np.ones(PLANES)
PLANE_RANGE[13:112:14] = 2.0
PLANE_RANGE[116] = 150.0
PLANE_RANGE[117] = 100.0


@functools.lru_cache(maxsize=None)
def chess_batch(seed=5):
    """[29, 8, 8, 118] float32 (read-only).  Boards 0-13: eight valid history
    steps, each an independent position of seeded random playouts, some with
    a repetition count; 14-20: random `valid` patterns with step 7 valid; 21,
    22: the search's own forms [0 x 6, start, cur] and (a root's) [0 x 7,
    start] with cur's castling rights and counters; the last N_FLOAT:
    non-negative floats, uniform in each plane's real range (the counters of
    planes 116-117 reach 100 and more)."""
    rng = np.random.RandomState(seed)
    pool, _ = C.random_positions(400, seed=seed)
    n_hist = BATCH - N_FLOAT - 2
    x = np.zeros((BATCH, 8, 8, PLANES), np.float64)
    for b in range(n_hist):
        hist = pool[rng.choice(len(pool), 8, replace=False)].copy()
        hist["repetition"] = rng.randint(0, 3, 8) * (rng.rand(8) < 0.3)
        valid = np.ones(8, np.uint8)
        if b >= 14:
            valid[:7] = rng.randint(0, 2, 7)
        x[b] = C.full_state(hist, valid, hist[7])
    for b, is_root in ((n_hist, False), (n_hist + 1, True)):
        cur = pool[rng.randint(1, len(pool))]
        x[b] = C.full_state(*C.reference_history(cur, is_root), cur)
    x[-N_FLOAT:] = rng.rand(N_FLOAT, 8, 8, PLANES) * PLANE_RANGE
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def lively_chess_weights(depth, hidden, x, seed=0):
    """forward_ref.lively_weights for the chess network: float32 arrays by name."""
    return fr._lively(8, 8, False, depth, hidden, x, seed, in_channels=PLANES, A=ACTIONS)[0]


MUTANTS = fr.MUTANTS + ("M6", "M7")
MOVES_POLICY = fr.MOVES_POLICY + ("M6", "M7")
MOVES_VALUE = fr.MOVES_VALUE + ("M6", "M7")


def mutants(w, x, depth, h=None):
    """forward_ref.mutants' M1..M5 and
    M6 the stem kernel's input plane 63 zeroed: the last plane of the two
       32-plane chunks the self-play stem skips (a forward that wrongly ran
       first_chunk = 2, or a K loop a chunk short, does far more);
    M7 the input rounded to fp16 before the stem (a lost second term of the
       input rows: pad_rows_kernel's split, the tower's t1_unscale)."""
    out = fr.mutants(w, x, depth, h)
    w6 = dict(w)
    w6["stem.kernel"] = np.array(w["stem.kernel"], np.float64)
    w6["stem.kernel"][:, :, 63, :] = 0
    out["M6"] = fr.restate(w6, x, depth)
    out["M7"] = fr.restate(w, fr.fp16(x), depth)
    return out


@functools.lru_cache(maxsize=None)
def layouts():
    """case name -> the row tests/native/tower_layout_check.cpp --rows-stem
    prints for it; "depths": the rows of depth 1..16 at hidden 256."""
    args = ["--rows-stem"] + [str(v) for c in CASES for v in (c.depth, c.hidden)]
    sweep = ["--rows-stem"] + [str(v) for d in range(1, 18) for v in (d, 256)]
    with tempfile.TemporaryDirectory() as tmp:
        rows = json.loads(fr.run_layout_check(tmp, args))
        depths = json.loads(fr.run_layout_check(tmp, sweep))
    assert len(rows) == len(CASES)
    out = {c.name: r for c, r in zip(CASES, rows)}
    out["depths"] = depths
    return out


@functools.lru_cache(maxsize=None)
def case_data(name):
    """One case's batch, weights, float64 reference, float32 error, mutant
    errors and tolerances (a dict; computed once, treat as read-only): the
    keys of forward_ref.case_data."""
    c = CASE_BY_NAME[name]
    x = chess_batch()
    w, h = fr._lively(8, 8, False, c.depth, c.hidden, x, c.seed, in_channels=PLANES, A=ACTIONS)
    p, v = fr.heads(w, h)
    pf, _, _, z, _ = fr.head_parts(w, h)
    p32, v32 = fr.restate(w, x, c.depth, np.float32)
    e32_p, e32_v = float(np.abs(p32 - p).max()), float(np.abs(v32 - v).max())
    mut_p, mut_v = {}, {}
    for m, (mp, mv) in mutants(w, x, c.depth, h).items():
        mut_p[m], mut_v[m] = float(np.abs(mp - p).max()), float(np.abs(mv - v).max())
    d = dict(case=c, x=x, w=w, p=p, v=v, e32_p=e32_p, e32_v=e32_v, mut_p=mut_p, mut_v=mut_v,
             tol_p=min(mut_p[m] for m in MOVES_POLICY) / 8, tol_v=min(mut_v[m] for m in MOVES_VALUE) / 8,
             dense1_active=float((z > 0).mean()), dense1_units_alive=float((z > 0).any(axis=0).mean()),
             last_policy_feature_live=bool((pf[:, -1] > 0).any()))
    for a in (p, v):
        a.setflags(write=False)
    return d
