"""Evaluator outputs at the edges of float32, shared by the select-order tests
(test_select_order_cpu.py on the CPU, test_host_eval_edges_gpu.py and
test_chess_host_eval_edges_gpu.py on the device).

An evaluator here is the synthetic evaluator (oracle/synth.py, or the chess
plane model) with one oddity applied on the boards whose hash falls in a
residue class, so most of a game is ordinary and the games go on.  Every
output is a deterministic function of the board alone.  The reference takes
whatever its model returns: a negative, cancelling, subnormal, huge, infinite
or NaN output is normalised, searched and backed up like any other, and the
best edge is np.argmax over the UCBs as Python floats (mcts.py:64-68) -- the
first NaN wins, else the first maximum.
"""
import contextlib

import numpy as np

import refport
import synth

# ------------------------------------------------------------------- np.argmax
ALPHABET = [float("nan"), float("-inf"), -1.0, -0.0, 0.0, 1.0, float("inf")]


def kept_rule_argmax(v):
    """The best-edge loop the oracles and the plain descents had before they
    followed np.argmax: the first element, then strict `>` (a NaN after index
    0 is never taken, a NaN at index 0 is never left)."""
    best = 0
    for i in range(1, len(v)):
        if v[i] > v[best]:
            best = i
    return best


# ------------------------------------------------------------------- Connect-N
# (height, width, n, gravity, sims): the smallest shape of each descent
SHAPES = {
    "c4_6x7": (6, 7, 4, True, 25),        # L = 8, the compile-time Connect-4 play
    "grav_4x5": (4, 5, 4, True, 16),      # L = 8, runtime masks
    "nograv_4x4": (4, 4, 3, False, 16),   # L = 16: the first row-mirror step
    "nograv_5x5": (5, 5, 4, False, 16),   # L = 32: the first shuffle step
    "nograv_6x6": (6, 6, 4, False, 12),   # L = 64
    "nograv_5x13": (5, 13, 4, False, 8),  # 65 actions: the serial descent
}
FINITE = ["neg", "cancel", "subnormal", "big", "negzero", "illegal_junk"]
NONFINITE = ["nan_value", "inf_value", "inf_prob", "nan_prob"]
KINDS = FINITE + NONFINITE
SEEDS = (100, 101)


# The cases the device tests run.  +inf values part np.argmax from the earlier
# loop only on the gravity boards (W reaches inf - inf where a column is
# revisited), so that kind runs there; every other kind runs on every shape.
GPU_CASES = [(shape, kind) for shape in SHAPES for kind in KINDS
             if kind != "inf_value" or SHAPES[shape][3]]
# ... of which the non-finite ones are live (test_select_order_cpu.py).  Not
# nan_prob: with every UCB of a node NaN a serial loop takes edge 0 under
# either rule; what that kind checks on the device is that lanes agree.
LIVE_CASES = [(shape, kind) for shape, kind in GPU_CASES if kind in NONFINITE and kind != "nan_prob"]


def action_space(shape):
    H, W, _n, gravity, _s = SHAPES[shape]
    return W if gravity else W * H


def stone_hash(board):
    """stones on the board + 3 x the mover's stones on the bottom row"""
    b = np.asarray(board)
    return int(np.count_nonzero(b)) + 3 * int(np.count_nonzero(b[-1] == 1))


def legal_actions(board, gravity):
    """legal action indices, ascending (x with gravity, x * H + y without)"""
    b = np.asarray(board)
    H, W = b.shape
    if gravity:
        return [x for x in range(W) if b[0, x] == 0]
    return [x * H + y for x in range(W) for y in range(H) if b[y, x] == 0]


def odd_board(kind, board):
    h = stone_hash(board)
    if kind == "inf_value":
        return h % 4 == 1
    if kind == "cancel":
        return h % 3 == 1
    return h % 5 == 2


def cancelling(k):
    """k >= 2 nonzero small integers summing to zero: every partial sum is
    exact in float32, so the sum is 0.0f in any order of addition"""
    out = []
    for i in range(k // 2):
        out += [1.0 + i % 7, -(1.0 + i % 7)]
    if k % 2:
        out[-2:] = [1.0, 1.0, -2.0]
    return out


def oddify(kind, p, v, legal, odd):
    """apply `kind` to the float32 outputs (p [A], v) of a board whose legal actions are `legal`"""
    p = np.array(p, np.float32)
    v = np.float32(v)
    if not odd or kind is None:
        return p, v
    if kind == "neg":
        p = p - np.float32(0.3)
    elif kind == "cancel":
        if len(legal) >= 2:
            p[legal] = np.array(cancelling(len(legal)), np.float32)
    elif kind == "subnormal":
        p = p * np.float32(1e-39)
    elif kind == "big":
        v = v * np.float32(1e30)
    elif kind == "negzero":
        v = np.float32(-0.0)
    elif kind == "illegal_junk":
        illegal = np.ones(len(p), bool)
        illegal[legal] = False
        junk = np.where(np.arange(len(p)) % 2 == 0, np.float32("nan"), np.float32("inf"))
        p = np.where(illegal, junk, p).astype(np.float32)
    elif kind == "nan_value":
        v = np.float32("nan")
    elif kind == "inf_value":
        v = np.float32("inf")
    elif kind == "inf_prob":
        p[legal[-1]] = np.float32("inf")  # the node's last prior inf / inf = NaN, the others x / inf = 0
    elif kind == "nan_prob":
        p[legal[-1]] = np.float32("nan")  # the float32 sum is NaN: every prior of the node is NaN
    else:
        raise ValueError(kind)
    return p, v


class BoardEval:
    """board [H, W] int8 (canonical: the mover is +1) -> (probs f32 [A], value f32)"""

    def __init__(self, kind, shape):
        self.kind = kind
        self.H, self.W, _n, self.gravity, _s = SHAPES[shape]
        self.A = action_space(shape)

    def __call__(self, board):
        b = np.asarray(board, np.int8)
        own, opp = synth.masks_from_array(b, self.W)
        p, v = synth.synth_eval(own, opp, self.A)
        if self.kind is None:
            return np.asarray(p, np.float32), np.float32(v)
        with np.errstate(all="ignore"):
            return oddify(self.kind, p, v, legal_actions(b, self.gravity), odd_board(self.kind, b))


class PlaneModel:
    """the engine's host evaluator: x [n, H, W, 4] full_state planes -> (probs [n, A], values [n])"""

    def __init__(self, kind, shape):
        self.f = BoardEval(kind, shape)

    def __call__(self, x):
        boards = (x[..., 1] == 1.0).astype(np.int8) - (x[..., 2] == 1.0).astype(np.int8)
        rows = [self.f(b) for b in boards]
        return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32)


class KeptRuleMCTS(refport.PortMCTS):
    """PortMCTS with kept_rule_argmax in place of np.argmax in select"""

    def search(self, sims):
        for _ in range(sims):
            node, path = self.root, []
            while node.edges:
                e = node.edges[kept_rule_argmax([e.ucb() for e in node.edges])]
                path.append(e)
                node = e.child
            v = -self._expand(node) if not node.board.over else node.board.result()
            for e in reversed(path):
                e.visits += 1
                e.value_sum += v
                v = -v


@contextlib.contextmanager
def _mcts_class(cls):
    saved = refport.PortMCTS
    refport.PortMCTS = cls
    try:
        yield
    finally:
        refport.PortMCTS = saved


_GAMES = {}


def port_game(shape, kind, seed, kept_rule=False):
    """refport.play_game under BoardEval(kind, shape): np.argmax on Python floats, as mcts.py
    (kept_rule: the earlier loop instead).  Computed once per process."""
    key = (shape, kind, seed, kept_rule)
    if key not in _GAMES:
        H, W, n, gravity, sims = SHAPES[shape]
        f = BoardEval(kind, shape)

        def ev(board):
            p, v = f(board.cells)
            return p, float(v)

        with np.errstate(all="ignore"), _mcts_class(KeptRuleMCTS if kept_rule else refport.PortMCTS):
            _GAMES[key] = refport.play_game(H, W, n, gravity, sims, seed, ev)
    return _GAMES[key]


def same_game(a, b):
    return (a["T"] == b["T"] and np.array_equal(a["moves"], b["moves"])
            and np.array_equal(np.asarray(a["policies"]).view(np.uint64), np.asarray(b["policies"]).view(np.uint64))
            and a["expansions"] == b["expansions"])


# ----------------------------------------------------------------------- chess
CHESS_SIMS, CHESS_PLIES, CHESS_GAMES, CHESS_SEED = 8, 10, 3, 900
_ALL_MOVES = []


class ChessEval:
    """The chess oracle's callback (pos, initial) -> (probs f32 [1880], value):
    a seeded function of the bytes of the position's (8, 8, 118) full_state
    planes -- what the engine hands its host evaluator -- with `kind` applied
    where the bytes' CRC falls in the residue class.  Every row is kept by
    those bytes, so model() below is the same function on the engine's side
    without the position: a state this evaluator never saw is a search that
    left the oracle's, and raises."""

    def __init__(self, kind):
        self.kind = kind
        self.rows = {}

    def __call__(self, pos, initial):
        import zlib

        import chess_oracle as C
        if not _ALL_MOVES:
            _ALL_MOVES.append(C.all_moves())
        x = C.full_state(*C.reference_history(pos, bool(initial)), pos).astype(np.float32)
        key = x.tobytes()
        if key not in self.rows:
            h = zlib.crc32(key)
            rng = np.random.RandomState(h)
            p = rng.random_sample(1880).astype(np.float32)
            v = np.float32(rng.random_sample() * 2.0 - 1.0)
            odd = {"inf_value": h % 4 == 1, "cancel": h % 3 == 1}.get(self.kind, h % 5 == 2)
            legal = np.flatnonzero(C.legal_mask(pos, _ALL_MOVES[0]))
            with np.errstate(all="ignore"):
                self.rows[key] = oddify(self.kind, p, v, legal, odd and len(legal) > 0)
        p, v = self.rows[key]
        return p, float(v)

    def model(self, x):
        rows = [self.rows[np.ascontiguousarray(xi, np.float32).tobytes()] for xi in x]
        return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.float32)


def chess_games(ev):
    import chess_oracle as C
    return [C.play_game(CHESS_SIMS, CHESS_SEED + g, CHESS_PLIES, callback=ev) for g in range(CHESS_GAMES)]


def same_chess_game(a, b):
    return (a["T"] == b["T"] and np.array_equal(a["moves"], b["moves"]) and a["expansions"] == b["expansions"]
            and np.array_equal(a["policy_probs"].view(np.uint64), b["policy_probs"].view(np.uint64)))
