"""Reference side of the inference forward's shape tests (TEST INFRASTRUCTURE).

  lively_weights  Keras-init weights whose heads are calibrated on a batch so
                  that both outputs depend on every head matrix: with
                  init_weights(randomize_bn=True) alone the one-channel value
                  conv is negative everywhere after its batch norm, the value
                  is tanh of a constant and the value dense goes unchecked
  restate         the forward in numpy with the dtype as a parameter: float64
                  is the reference (equal to keras_ref.forward), float32 the
                  run whose own error e32 the tolerances are measured against
  mutants         five wrong forwards in float64 (M1..M5 below), each the kind
                  of error a kernel can make; the tolerance of a case is an
                  eighth of what the mildest of them does to that output
  CASES           the board / depth / hidden table, one row per tower layout
                  (tests/native/tower_layout_check.cpp states which)
  FALLBACK_CASES  networks the default conv_algo gives a per-layer form
                  (tests/native/net_form_check.cpp states which)
  case_data       everything of one case, computed once per process

Nothing here touches libaz.
"""
import collections
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

from custom_alphazero.model.weights import init_weights, weight_spec

EPS = 1e-3  # tf.keras BatchNormalization default (oracle/keras_ref.py)

Case = collections.namedtuple("Case", "name H W n gravity depth hidden")


def _case(H, W, gravity, depth, hidden=256, n=None):
    n = n if n is not None else min(4, H, W)
    name = f"{H}x{W}{'g' if gravity else 'n'}_d{depth}_h{hidden}"
    return Case(name, H, W, n, gravity, depth, hidden)


# the layout each row is in the table for: tests/test_forward_cases_cpu.py
# asserts them against the library's own chooser
CASES = [
    _case(6, 7, True, 4),            # 128 rows x 3 boards, wv1 by X tile; dual, the 96-row tiles stage the blob
    _case(6, 7, False, 2),           # A = 42: wpd from L2; the alt layout has wpd in LDS and wv1 from L2
    _case(6, 7, True, 16),           # 16 blocks of biases: what is left of the LDS
    _case(6, 7, True, 2, 1),         # hidden = 1
    _case(6, 7, True, 2, 100),       # P = 5, 12 idle threads
    _case(6, 7, True, 2, 255),       # HW * hidden not a multiple of 4: wv1 from L2
    _case(6, 6, True, 2, 64),        # wv1 in LDS in the primary layout; dual
    _case(5, 5, False, 4),           # 5 boards per tile, the 8-board value pass
    _case(5, 5, False, 16),
    _case(2, 2, False, 1, n=2),      # 96 rows, 8 boards (the cap), no plan
    _case(3, 3, True, 1, n=3),       # 96 rows, 8 boards
    _case(4, 4, False, 2),           # 96 rows, 6 boards
    _case(6, 8, True, 2),            # 96-row primary tiles of 2 boards
    _case(2, 9, True, 2, n=2),       # no plan (H = 2)
    _case(9, 2, True, 2, n=2),       # no plan (W = 2)
    _case(7, 7, True, 2),            # 128 rows, 2 boards
    _case(8, 8, False, 2),           # wpd and wv1 from L2
    _case(8, 8, False, 16),
    _case(9, 9, True, 4),            # 192 rows
    _case(9, 9, False, 2),           # 192 rows, wpd from L2
    _case(8, 12, True, 2),           # 192 rows, full
    _case(10, 10, True, 2),          # 1 board per tile
    _case(11, 11, False, 2),         # A = 121: both matrices from L2, 4 policy passes
    _case(11, 11, False, 16),
    _case(8, 16, True, 1),           # HW = 128: no pad row
    _case(16, 8, True, 1),
    _case(2, 20, True, 1, n=2),      # W > 16 (the per-layer fp16 kernels refuse it)
]
# what AZ_CONV_F16X2 runs where the one-launch tower does not take the network (csrc/az_net_form.h):
# tests/test_net_form_cpu.py asserts the forms, tests/test_forward_forms_gpu.py runs them
FALLBACK_CASES = [
    _case(3, 3, True, 17, n=3),        # depth > 16: the per-layer fp16x2 chain
    _case(3, 3, True, 1, 300, n=3),    # hidden > 256: the same
    _case(2, 20, True, 17, n=2),       # depth > 16 and W > 16: the fp32 MFMA chain
    _case(3, 3, True, 0, n=3),         # no block: the fp32 MFMA chain.  No block conv either, so mutant M3
                                       # does not exist here: it is left out of this case's minima
]
CASE_BY_NAME = {c.name: c for c in CASES + FALLBACK_CASES}
# boards of 33-48 cells: 128-row tiles of three, or 96-row tiles of two for small launches
DUAL_CASES = ("6x7g_d4_h256", "6x7n_d2_h256", "6x7g_d2_h1", "6x7g_d2_h100", "6x7g_d2_h255", "6x6g_d2_h64",
              "2x20g_d1_h256")
BATCH = 29  # prime: every tile size leaves a partial tile


def action_space(c):
    return c.W if c.gravity else c.H * c.W


def make_batch(H, W, boards=BATCH, seed=5):
    """Random one-hot boards (full_state planes: empty, own, other, turn = 1)
    and, last, four boards of arbitrary float planes."""
    rng = np.random.RandomState(seed)
    b = rng.randint(-1, 2, (boards, H, W))
    x = np.zeros((boards, H, W, 4), np.float32)
    x[..., 0] = b == 0
    x[..., 1] = b == 1
    x[..., 2] = b == -1
    x[..., 3] = 1.0
    x[-4:] = rng.rand(4, H, W, 4).astype(np.float32)
    return x


def fp16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _conv(x, kernel, bias):
    """x [B,H,W,Cin], kernel [k,k,Cin,Cout]; stride 1, SAME; in x's dtype."""
    k = kernel.shape[0]
    p = k // 2
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    out = np.zeros((B, H, W, kernel.shape[3]), x.dtype)
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ kernel[ky, kx]
    return out + bias


def _bn(y, w, unit, dt):
    g, b, m, v = (np.asarray(w[f"{unit}.{f}"], dt) for f in ("gamma", "beta", "mean", "var"))
    return (y - m) / np.sqrt(v + dt(EPS)) * g + b


def _unit(x, w, unit, dt, relu=True, kernel_map=None, drop_corner_tap=False):
    K = np.asarray(w[unit + ".kernel"], dt)
    if kernel_map is not None and K.shape[0] == 3:
        K = kernel_map(K).astype(dt)
    y = _conv(x, K, np.asarray(w[unit + ".bias"], dt))
    if drop_corner_tap:  # M3: the last pixel's conv without its (-1, -1) neighbour
        H, W = x.shape[1:3]
        y[:, H - 1, W - 1, :] -= x[:, H - 2, W - 2, :] @ K[0, 0]
    y = _bn(y, w, unit, dt)
    return np.maximum(y, dt(0)) if relu else y


def trunk(w, x, depth, dtype=np.float64, store=None, kernel_map=None, drop_corner_tap=False):
    """The stem and the residual blocks -> [B,H,W,F].  store: applied to every
    activation a kernel keeps between convs (stem, conv1 and block outputs);
    kernel_map: applied to the 3x3 kernels; drop_corner_tap: the last block's
    conv2 leaves tap (-1, -1) out at pixel (H-1, W-1)."""
    dt = np.dtype(dtype).type
    keep = (lambda a: a) if store is None else (lambda a: store(a).astype(dt))
    h = keep(_unit(np.asarray(x, dt), w, "stem", dt, kernel_map=kernel_map))
    for d in range(depth):
        a = keep(_unit(h, w, f"block{d}.conv1", dt, kernel_map=kernel_map))
        a = _unit(a, w, f"block{d}.conv2", dt, relu=False, kernel_map=kernel_map,
                  drop_corner_tap=drop_corner_tap and d == depth - 1)
        r = _unit(h, w, f"block{d}.res", dt, relu=False)
        h = keep(np.maximum(a + r, dt(0)))
    return h


def head_parts(w, h, dtype=np.float64):
    """-> policy features [B,2HW], logits [B,A], value features [B,HW], dense1
    pre-activations [B,hidden], pre-tanh value [B]."""
    dt = np.dtype(dtype).type
    B = h.shape[0]
    pf = _unit(h, w, "policy.conv", dt).reshape(B, -1)  # Flatten on NHWC: (H, W, C)
    logits = pf @ np.asarray(w["policy.dense.kernel"], dt) + np.asarray(w["policy.dense.bias"], dt)
    vf = _unit(h, w, "value.conv", dt).reshape(B, -1)
    z = vf @ np.asarray(w["value.dense1.kernel"], dt) + np.asarray(w["value.dense1.bias"], dt)
    u = np.maximum(z, dt(0)) @ np.asarray(w["value.dense2.kernel"], dt) + np.asarray(w["value.dense2.bias"], dt)
    return pf, logits, vf, z, u.reshape(B)


def heads(w, h, dtype=np.float64):
    _, logits, _, _, u = head_parts(w, h, dtype)
    logits = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(logits)
    return e / e.sum(axis=1, keepdims=True), np.tanh(u)


def restate(w, x, depth, dtype=np.float64, **mutation):
    """(probs [B,A], values [B]) in `dtype`."""
    return heads(w, trunk(w, x, depth, dtype, **mutation), dtype)


def _lively(H, W, gravity, depth, hidden, x, seed, in_channels=4, A=None):
    """A: the action space where it is not the board's own (chess, tests/chess_forward_ref.py)."""
    A = A if A is not None else W if gravity else H * W
    spec = weight_spec(H, W, A, depth=depth, hidden=hidden, in_channels=in_channels)
    w = {k: np.asarray(v, np.float64) for k, v in init_weights(spec, seed=seed, randomize_bn=True).items()}
    w["value.conv.beta"] = np.full_like(w["value.conv.beta"], 0.5)
    w["policy.conv.beta"] = np.full_like(w["policy.conv.beta"], 0.3)
    h = trunk(w, x, depth)  # the trunk stays Keras init
    _, logits, _, z, _ = head_parts(w, h)
    w["policy.dense.kernel"] = w["policy.dense.kernel"] / logits.std()
    w["value.dense1.kernel"] = w["value.dense1.kernel"] / z.std()
    w["value.dense2.bias"] = np.zeros_like(w["value.dense2.bias"])
    u = head_parts(w, h)[4]
    w["value.dense2.kernel"] = w["value.dense2.kernel"] * (0.5 / u.std())
    w["value.dense2.bias"] = np.full_like(w["value.dense2.bias"], -head_parts(w, h)[4].mean())
    return {k: v.astype(np.float32) for k, v in w.items()}, h


def lively_weights(H, W, gravity, depth, hidden, x, seed=0):
    """init_weights(seed, randomize_bn=True) with the heads calibrated in
    float64 on the batch x: the head convs' beta 0.5 (value) and 0.3 (policy),
    the policy dense scaled to logits of standard deviation 1, value dense1 to
    pre-activations of standard deviation 1, value dense2 to a pre-tanh value
    of standard deviation 0.5 and mean 0.  float32 arrays by name."""
    return _lively(H, W, gravity, depth, hidden, x, seed)[0]


MUTANTS = ("M1", "M2", "M3", "M4", "M5")
MOVES_POLICY = ("M1", "M2", "M3", "M5")
MOVES_VALUE = ("M1", "M2", "M3", "M4")


def mutants(w, x, depth, h=None):
    """name -> (probs, values), float64.
    M1 every stored activation rounded to fp16 (a lost split16 second term);
    M2 the 3x3 kernels rounded to fp16 (a lost weight term);
    M3 the last block's conv2 without tap (-1, -1) at pixel (H-1, W-1) (a
       border skip too many);
    M4 the last row of value.dense1.kernel zeroed, M5 of policy.dense.kernel
       (a head that stops one row short).
    h: the unmutated trunk output, if the caller has it."""
    h = trunk(w, x, depth) if h is None else h
    w4, w5 = dict(w), dict(w)
    w4["value.dense1.kernel"] = np.array(w["value.dense1.kernel"], np.float64)
    w4["value.dense1.kernel"][-1, :] = 0
    w5["policy.dense.kernel"] = np.array(w["policy.dense.kernel"], np.float64)
    w5["policy.dense.kernel"][-1, :] = 0
    return {"M1": restate(w, x, depth, store=fp16),
            "M2": restate(w, x, depth, kernel_map=fp16),
            "M3": restate(w, x, depth, drop_corner_tap=True),
            "M4": heads(w4, h),
            "M5": heads(w5, h)}


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "custom-alphazero_amd", "custom_alphazero", "_lib")


def have_lib():
    return os.path.exists(os.path.join(LIB, "libaz.so"))


@functools.lru_cache(maxsize=None)
def layouts():
    """case name -> the layout row tests/native/tower_layout_check.cpp prints
    for it (built against libaz.so and run once per process)."""
    args = [str(v) for c in CASES for v in (c.H, c.W, action_space(c), c.depth, c.hidden)]
    with tempfile.TemporaryDirectory() as tmp:
        rows = json.loads(run_layout_check(tmp, args))
    assert len(rows) == len(CASES)
    return {c.name: r for c, r in zip(CASES, rows)}


def run_layout_check(tmp, args):
    """Builds tests/native/tower_layout_check.cpp in tmp against libaz.so and
    the library's layout header, runs it with args -> its stdout."""
    return run_native_check(tmp, "tower_layout_check", args)


def run_native_check(tmp, program, args):
    """Builds tests/native/<program>.cpp in tmp against libaz.so and the
    library's host-only headers, runs it with args -> its stdout."""
    exe = os.path.join(tmp, program)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(REPO, "custom-alphazero_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "native", program + ".cpp"),
                    os.path.join(LIB, "libaz.so"), f"-Wl,-rpath,{LIB}"], check=True)
    return subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout


@functools.lru_cache(maxsize=None)
def case_data(name):
    """One case's (of CASES or FALLBACK_CASES) batch, weights, float64
    reference, float32 error, mutant errors, the mutants that move each output
    and the tolerances (a dict; computed once, treat as read-only)."""
    c = CASE_BY_NAME[name]
    x = make_batch(c.H, c.W)
    w, h = _lively(c.H, c.W, c.gravity, c.depth, c.hidden, x, 0)
    p, v = heads(w, h)
    z = head_parts(w, h)[3]
    p32, v32 = restate(w, x, c.depth, np.float32)
    e32_p, e32_v = float(np.abs(p32 - p).max()), float(np.abs(v32 - v).max())
    mut_p, mut_v = {}, {}
    for m, (mp, mv) in mutants(w, x, c.depth, h).items():
        mut_p[m], mut_v[m] = float(np.abs(mp - p).max()), float(np.abs(mv - v).max())
    # (M3 drops a tap of the last block's conv2: without a block it is the unmutated forward)
    moves_p, moves_v = ([m for m in ms if m != "M3" or c.depth > 0] for ms in (MOVES_POLICY, MOVES_VALUE))
    d = dict(case=c, x=x, w=w, p=p, v=v, e32_p=e32_p, e32_v=e32_v, mut_p=mut_p, mut_v=mut_v,
             moves_p=moves_p, moves_v=moves_v,
             tol_p=min(mut_p[m] for m in moves_p) / 8, tol_v=min(mut_v[m] for m in moves_v) / 8,
             dense1_active=float((z > 0).mean()), dense1_units_alive=float((z > 0).any(axis=0).mean()))
    for a in (x, p, v):
        a.setflags(write=False)
    return d
