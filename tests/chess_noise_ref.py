"""Plain-Python chess MCTS with Dirichlet root noise: the reference for the
chess engine's noisy search (tests/test_chess_noise_*.py).

The chess oracle (oracle/chess_oracle.c) has no root noise, so this restates
mcts/mcts.py:58-222 in the shape of oracle/refport.py's PortMCTS on the
oracle's chess primitives (legal_moves, legal_mask, play_canonical, outcome,
synth) and the package's normalize_probabilities.  The noisy selection is the
reference's own numpy expression (get_best_edge_with_noise, mcts.py:70-85) on
a np.random.RandomState, so the dtypes fall out as they do there: the priors
array is float32 after normalize_probabilities' quotient and float64 after its
uniform branch.  With noise off it must equal the oracle
(tests/test_chess_noise_cpu.py), which is what licenses it with noise on.
"""
import numpy as np

import chess_oracle as C
from custom_alphazero.mcts.utils import normalize_probabilities

_ALL = None
_INDEX = None


def _actions():
    global _ALL, _INDEX
    if _ALL is None:
        _ALL = C.all_moves()
        _INDEX = {int(m): i for i, m in enumerate(_ALL)}
    return _ALL, _INDEX


class Edge:
    __slots__ = ("parent", "child", "action", "prior", "visits", "value_sum")

    def __init__(self, parent, action, prior):
        self.parent, self.action = parent, int(action)
        self.child = None  # made on the first visit (its board is a function of parent and action)
        self.prior = prior  # the numpy scalar normalize_probabilities gave: np.float32 or np.float64
        self.visits = 0
        self.value_sum = 0.0

    def node(self):
        if self.child is None:
            self.child = Node(C.play_canonical(self.parent.pos, self.action), 0)
        return self.child

    def ucb(self, c, override_prior=None):
        # exploitation_term + exploration_term (mcts.py:39-55); a stored prior
        # enters as a Python float (legacy promotion of the np.float32 scalar)
        prior = override_prior if override_prior is not None else float(self.prior)
        try:
            q = self.value_sum / self.visits
        except ZeroDivisionError:
            q = 0.0
        total = sum(e.visits for e in self.parent.edges)
        return q + c * prior * (total ** 0.5) / (1 + self.visits)


class Node:
    __slots__ = ("pos", "initial", "edges", "value")

    def __init__(self, pos, initial):
        self.pos, self.initial = pos, initial
        self.edges = []
        self.value = None


class Tree:
    """One MCTS object on a chess root.  noise = (alpha, ratio) or None;
    callback(pos, initial) -> (probs f32[1880], value) replaces the oracle's
    synthetic evaluator; rng is the np.random.RandomState root noise and
    play() draw from (rows given to search() take the noise's place)."""

    def __init__(self, root, c_puct=1.5, callback=None, noise=None, rng=None):
        self.root_node = Node(np.array([root], C.POS_DTYPE)[0], 1)
        self.c, self.callback, self.noise, self.rng = c_puct, callback, noise, rng
        self.expansions = 0
        self.rows_used = 0

    def _expand(self, node):
        all_mv, _ = _actions()
        if self.callback is None:
            probs, value = C.synth(node.pos, node.initial)
        else:
            probs, value = self.callback(node.pos, node.initial)
            probs, value = np.asarray(probs, np.float32), float(np.float32(value))
        mask = C.legal_mask(node.pos, all_mv).astype(bool)
        priors = normalize_probabilities(probs[mask])  # action order ...
        for prior, move in zip(priors, C.legal_moves(node.pos)):  # ... zipped positionally (mcts.py:147-160)
            node.edges.append(Edge(node, move, prior))
        node.value = value
        self.expansions += 1
        return value

    def _best_edge_with_noise(self, node, row):
        alpha, ratio = self.noise
        priors = np.asarray([e.prior for e in node.edges])
        if row is None:
            d = self.rng.dirichlet(np.ones(len(priors)) * alpha)
        else:
            d = np.asarray(row, np.float64)[:len(priors)]
        noisy_priors = (1 - ratio) * priors + ratio * d
        return node.edges[int(np.argmax([e.ucb(self.c, override_prior=p)
                                         for e, p in zip(node.edges, noisy_priors)]))]

    def search(self, sims, rows=None):
        """rows: [r, 256] pre-drawn noise vectors, one per simulation whose
        root has edges, in order (the tree API's host-drawn noise)."""
        used = 0
        for _ in range(sims):
            node, path = self.root_node, []
            while node.edges:
                if node is self.root_node and self.noise is not None:
                    row = None
                    if rows is not None:
                        row = rows[used]
                        used += 1
                    e = self._best_edge_with_noise(node, row)
                else:
                    e = node.edges[int(np.argmax([x.ucb(self.c) for x in node.edges]))]
                path.append(e)
                node = e.node()
            oc = C.outcome(node.pos)
            if oc == 0:
                v = -self._expand(node)
            else:
                v = 1.0 if oc == 1 else 0.0
            for e in reversed(path):
                e.visits += 1
                e.value_sum += v
                v = -v
        self.rows_used = used

    def play(self, u=None, greedy=False, deterministic=False):
        """-> (move, outcome of the new root, policy actions, policy probs);
        u: the random_sample np.random.choice consumes (None: drawn from rng)."""
        _, index = _actions()
        node = self.root_node
        if not node.edges:
            raise RuntimeError("play() before search")
        visits = [e.visits for e in node.edges]
        if greedy:
            p = np.zeros(len(node.edges)).astype(float)
            p[int(np.argmax(visits))] = 1.0
        else:
            p = normalize_probabilities(np.asarray(visits).astype(float))
        if deterministic:
            idx = int(np.argmax(p))
        else:
            if u is None:
                u = self.rng.random_sample()
            cdf = p.cumsum()  # np.random.choice: cumsum, normalise, searchsorted right
            cdf /= cdf[-1]
            idx = min(int(cdf.searchsorted(u, side="right")), len(p) - 1)
        e = node.edges[idx]
        self.root_node = e.node()
        pa = np.array([index[x.action] for x in node.edges], np.int16)
        return e.action, C.outcome(self.root_node.pos), pa, p

    def root(self):
        ed = self.root_node.edges
        return dict(moves=np.array([e.action for e in ed], np.uint16),
                    prior=np.array([float(e.prior) for e in ed], np.float64),
                    n=np.array([e.visits for e in ed], np.int64),
                    w=np.array([e.value_sum for e in ed], np.float64),
                    child_n=np.array([len(e.child.edges) if e.child is not None else 0 for e in ed], np.int32))


def play_game(sims, seed, max_plies, greedy_ply=8, c_puct=1.5, callback=None, noise=None):
    """One chess self-play game as oracle/chess_oracle.c orc_chess_play_game
    plays it, from np.random.RandomState(seed): every move's root-noise
    vectors in simulation order, then play's one random_sample."""
    rng = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    t = Tree(C.from_fen(), c_puct, callback, noise, rng)
    positions, moves, pol_a, pol_p = [], [], [], []
    term = 0
    while True:
        term = C.outcome(t.root_node.pos)
        if term != 0:
            break
        if len(moves) >= max_plies:
            term = 5
            break
        t.search(sims)
        pos = t.root_node.pos
        mv, _oc, pa, pp = t.play(None, int(pos["fullmove_number"]) >= greedy_ply, False)
        positions.append(pos)
        moves.append(mv)
        pol_a.append(pa)
        pol_p.append(pp)
    return dict(T=len(moves), result=1 if term == 1 else 0, termination=term, expansions=t.expansions,
                positions=np.array(positions, C.POS_DTYPE), moves=np.array(moves, np.uint16),
                policy_n=np.array([len(a) for a in pol_a], np.int32), policy_actions=pol_a, policy_probs=pol_p)
