"""Reference side of the one-term fp16 forward's tests (AZ_CONV_F16; TEST
INFRASTRUCTURE, on forward_ref / chess_forward_ref).

  restate16      the forward in numpy with the mode's rounding: BN folded into
                 each conv in float64 (az_net_load.hip fold_unit), the folded
                 weights prescaled by 2^-e (conv16_prescale; conv2 and its 1x1
                 projection jointly) and rounded float64 -> float32 -> float16,
                 the input and every activation kept between convs (stem,
                 conv1 and block outputs except the last) rounded to float16,
                 sums in `dtype`; the heads are forward_ref.heads in float64
  costs          per case the max-abs distance of restate16(float64) from the
                 case's float64 outputs: cost_p, cost_v -- what the mode costs
                 in accuracy, and the unit every bound of its tests is in
  moved          how far the structural mutants M3 (a dropped tap at one
                 pixel), M4 / M5 (a head one row short) and, chess, M6 (a stem
                 plane lost) move restate16(float64).  chess_forward_ref's M7
                 -- the input rounded to fp16 -- is this mode's own arithmetic:
                 on restate16 it is the identity, moves nothing, and is no
                 mutant here
  exact_network  a network whose trunk is exact in fp16 (integer weights in
                 {-1, 0, 1} after folding, integer activations): the one-term
                 and the three-term kernels then sum the same products in the
                 same order and must agree bit for bit

Nothing here touches libaz."""
import functools

import numpy as np

import forward_ref as fr
from custom_alphazero.model.weights import init_weights, weight_spec


def _fold(w, unit, eps):
    """fold_unit: kernel * gamma / sqrt(var + eps), (bias - mean) * that + beta (float64)."""
    g, b, m, v = (np.asarray(w[f"{unit}.{f}"], np.float64) for f in ("gamma", "beta", "mean", "var"))
    sc = g / np.sqrt(v + eps)
    return np.asarray(w[unit + ".kernel"], np.float64) * sc, (np.asarray(w[unit + ".bias"], np.float64) - m) * sc + b


def prescale(*kernels):
    """conv16_prescale: e with max |w * 2^-e| in (4, 8]."""
    m = max(float(np.abs(k).max()) for k in kernels)
    return 0 if m == 0.0 else int(np.floor(np.log2(m / 8.0))) + 1


def _quant(k, e):
    return (k * 2.0 ** -e).astype(np.float32).astype(np.float16)


def trunk16(w, x, depth, dtype=np.float64, eps=fr.EPS, drop_corner_tap=False, stored=None):
    """-> the last block's output [B,H,W,F] in `dtype`, not rounded.  stored:
    a list that takes every activation kept between convs (after rounding)."""
    dt = np.dtype(dtype).type
    zero = np.zeros(1, dt)

    def keep(a):
        a = a.astype(np.float16).astype(dt)
        if stored is not None:
            stored.append(a)
        return a

    def conv(h, unit, res=None, drop=False):
        """relu(2^e (h * q + res_in * q_res) + bias): h, res_in fp16 values in dt."""
        k, b = _fold(w, unit, eps)
        folded = [k] if res is None else [k, _fold(w, res[1], eps)[0]]
        e = prescale(*folded)
        q = _quant(k, e).astype(dt)
        acc = fr._conv(h, q, zero)
        if drop:  # M3: the last pixel's conv without its (-1, -1) neighbour
            H, W = h.shape[1:3]
            acc[:, H - 1, W - 1, :] -= h[:, H - 2, W - 2, :] @ q[0, 0]
        if res is not None:
            acc = acc + fr._conv(res[0], _quant(folded[1], e).astype(dt), zero)
            b = b + _fold(w, res[1], eps)[1]
        return np.maximum(acc * dt(2.0 ** e) + b.astype(dt), dt(0))

    h = keep(conv(keep(np.asarray(x, dt)), "stem"))
    if stored is not None:
        del stored[0]  # (the input is no stored activation)
    for d in range(depth):
        a = keep(conv(h, f"block{d}.conv1"))
        h = conv(a, f"block{d}.conv2", res=(h, f"block{d}.res"), drop=drop_corner_tap and d == depth - 1)
        if d + 1 < depth:
            h = keep(h)
    return h


def restate16(w, x, depth, dtype=np.float64, eps=fr.EPS, **mutation):
    """(probs [B,A], values [B]): the one-term trunk in `dtype`, the heads in float64."""
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
    h = trunk16(w64, x, depth, dtype, eps, **mutation).astype(np.float64)
    if eps != fr.EPS:
        return _heads_eps(w64, h, eps)
    return fr.heads(w64, h)


def _heads_eps(w, h, eps):
    """forward_ref.heads with another BN epsilon (the exact network's 1.0):
    the head convs' BN rewritten to forward_ref's epsilon."""
    w = dict(w)
    for unit in ("policy.conv", "value.conv"):
        w[unit + ".var"] = np.asarray(w[unit + ".var"], np.float64) + (eps - fr.EPS)
    return fr.heads(w, h)


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


def _data(name):
    if name in fr.CASE_BY_NAME:
        return fr.case_data(name), False
    import chess_forward_ref as cr
    return cr.case_data(name), True


@functools.lru_cache(maxsize=None)
def costs(name):
    """One case (of forward_ref.CASES or chess_forward_ref.CASES): the
    float64 one-term outputs p16 / v16 and their distance cost_p / cost_v
    from the case's float64 outputs.  Computed once; read-only."""
    d, _ = _data(name)
    c = d["case"]
    w = {k: np.asarray(v, np.float64) for k, v in d["w"].items()}
    h = trunk16(w, d["x"], c.depth)
    p, v = fr.heads(w, h)
    for a in (p, v, h):
        a.setflags(write=False)
    return dict(p16=p, v16=v, h16=h, cost_p=_dist(p, d["p"]), cost_v=_dist(v, d["v"]))


@functools.lru_cache(maxsize=None)
def moved(name):
    """mutant -> (policy, value) distance from restate16(float64), the mutant on top of it."""
    d, chess = _data(name)
    c, k = d["case"], costs(name)
    w = {n: np.asarray(v, np.float64) for n, v in d["w"].items()}
    out = {}

    def put(m, pv):
        out[m] = (_dist(pv[0], k["p16"]), _dist(pv[1], k["v16"]))

    put("M3", fr.heads(w, trunk16(w, d["x"], c.depth, drop_corner_tap=True)))
    for m, key in (("M4", "value.dense1.kernel"), ("M5", "policy.dense.kernel")):
        wm = dict(w)
        wm[key] = np.array(w[key])
        wm[key][-1, :] = 0
        put(m, fr.heads(wm, k["h16"]))
    if chess:
        w6 = dict(w)
        w6["stem.kernel"] = np.array(w["stem.kernel"])
        w6["stem.kernel"][:, :, 63, :] = 0
        put("M6", fr.heads(w6, trunk16(w6, d["x"], c.depth)))
    return out


EXACT_EPS = 1.0


def exact_network(H, W, gravity, depth, hidden, seed, in_channels=4, A=None):
    """Weights (float32 by name) whose trunk is exact in fp16 at bn_epsilon
    = EXACT_EPS: var 3, gamma 2 (the folded scale is 2 / sqrt(3 + 1) = 1),
    mean 0, bias 0, integer beta in [-2, 1]; kernels in {-1, 0, 1} with 6
    non-zeros per output channel (the stem 18, half of Connect-N's 36 inputs);
    the heads Keras init.  On one-hot boards every activation is an integer."""
    A = A if A is not None else W if gravity else H * W
    spec = weight_spec(H, W, A, depth=depth, hidden=hidden, in_channels=in_channels)
    w = {k: np.asarray(v, np.float64) for k, v in init_weights(spec, seed=seed).items()}
    rng = np.random.RandomState(seed)
    units = ["stem"] + [f"block{d}.{u}" for d in range(depth) for u in ("conv1", "conv2", "res")]
    for unit in units:
        shape = w[unit + ".kernel"].shape
        n_in, F = shape[0] * shape[1] * shape[2], shape[3]
        nz = 18 if unit == "stem" else 6
        k = np.zeros((n_in, F))
        for co in range(F):
            k[rng.choice(n_in, nz, replace=False), co] = rng.choice([-1.0, 1.0], nz)
        w[unit + ".kernel"] = k.reshape(shape)
        w[unit + ".bias"] = np.zeros(F)
        w[unit + ".mean"] = np.zeros(F)
        w[unit + ".var"] = np.full(F, 3.0)
        w[unit + ".gamma"] = np.full(F, 2.0)
        w[unit + ".beta"] = rng.randint(-2, 2, F).astype(np.float64)
    return {k: v.astype(np.float32) for k, v in w.items()}


def onehot_batch(H, W, boards=fr.BATCH, seed=5):
    """forward_ref.make_batch without its float boards."""
    x = np.array(fr.make_batch(H, W, boards + 4, seed)[:boards])
    x.setflags(write=False)
    return x


# the exact network's shapes: (H, W, gravity, depth, hidden, seed)
EXACT_SHAPES = [(6, 7, True, 2, 256, 3), (9, 9, True, 2, 256, 3), (3, 3, True, 1, 256, 3)]
EXACT_CHESS = (1, 256, 3)  # depth, hidden, seed


def exact_chess_batch():
    """chess_forward_ref.chess_batch's boards (integer planes), without its float boards."""
    import chess_forward_ref as cr
    return cr.chess_batch()[:-cr.N_FLOAT]
