"""ctypes binding of libaz (include/az.h): the only way this package computes.

There is deliberately no CPU fallback: if ``_lib/libaz.so`` is missing or no
HIP device is visible, every entry point raises.  The reference's evaluator,
tree and worker seams all land here.
"""
import ctypes
import os
import time

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libaz.so")

EVAL_NETWORK = 0
EVAL_SYNTHETIC = 1
EVAL_HOST = 2  # include/az.h AZ_EVAL_HOST: a Python callable (Engine / ChessEngine.set_host_evaluator)
CONV_F16X2 = 0  # include/az.h AZ_CONV_F16X2 (default)
CONV_DIRECT = 1
CONV_F16X2_LAYERS = 2  # AZ_CONV_F16X2_LAYERS: the same arithmetic one layer per launch (A/B runs)
CONV_F16 = 3  # AZ_CONV_F16: one fp16 product per MAC on the one-launch tower (opt-in, for self-play; not fp32-accurate)


class AzError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [
        ("board_height", ctypes.c_int32), ("board_width", ctypes.c_int32),
        ("n", ctypes.c_int32), ("gravity", ctypes.c_int32),
        ("mcts_iterations", ctypes.c_int32), ("index_move_greedy", ctypes.c_int32),
        ("exploration_constant", ctypes.c_double), ("slots", ctypes.c_int32),
        ("evaluator", ctypes.c_int32), ("filters", ctypes.c_int32), ("depth", ctypes.c_int32),
        ("value_hidden", ctypes.c_int32), ("bn_epsilon", ctypes.c_double),
        ("arena_edges", ctypes.c_int64), ("max_tree_visits", ctypes.c_int64),
        ("cache_log2", ctypes.c_int32), ("conv_algo", ctypes.c_int32),
        ("lanes", ctypes.c_int32), ("compact", ctypes.c_int32),
        ("tower_natural_order", ctypes.c_int32), ("dirichlet_noise", ctypes.c_int32),
        ("dirichlet_alpha", ctypes.c_double), ("dirichlet_ratio", ctypes.c_double),
        ("rng_skip", ctypes.c_int32), ("reserved", ctypes.c_int32 * 1),
    ]


class ChessConfig(ctypes.Structure):
    """az_chess_config (include/az_chess.h)."""
    _fields_ = [
        ("mcts_iterations", ctypes.c_int32), ("index_move_greedy", ctypes.c_int32),
        ("exploration_constant", ctypes.c_double), ("slots", ctypes.c_int32),
        ("evaluator", ctypes.c_int32), ("filters", ctypes.c_int32), ("depth", ctypes.c_int32),
        ("value_hidden", ctypes.c_int32), ("max_plies", ctypes.c_int32),
        ("bn_epsilon", ctypes.c_double), ("arena_edges", ctypes.c_int64),
        ("conv_algo", ctypes.c_int32), ("lanes", ctypes.c_int32), ("cache_log2", ctypes.c_int32),
        ("dirichlet_noise", ctypes.c_int32), ("dirichlet_alpha", ctypes.c_double),
        ("dirichlet_ratio", ctypes.c_double),
    ]


class Tensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("numel", ctypes.c_int64),
                ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Stats(ctypes.Structure):
    _fields_ = [
        ("expansions", ctypes.c_int64), ("terminal_visits", ctypes.c_int64),
        ("games_done", ctypes.c_int64), ("simulations", ctypes.c_int64),
        ("plies", ctypes.c_int64), ("active_slots", ctypes.c_int64), ("errors", ctypes.c_int64),
        ("conv_launches", ctypes.c_int64), ("conv_ms", ctypes.c_double),
        ("cache_hits", ctypes.c_int64), ("evaluations", ctypes.c_int64),
        ("conv_busy_ms", ctypes.c_double), ("tree_launches", ctypes.c_int64), ("tree_ms", ctypes.c_double),
        ("path_edges", ctypes.c_int64), ("cache_inserts", ctypes.c_int64),
        ("cache_generation", ctypes.c_int64), ("cache_gen_size", ctypes.c_int64),
        ("cache_capacity", ctypes.c_int64), ("games_drained", ctypes.c_int64),
        ("max_retained", ctypes.c_int64), ("cache_entries", ctypes.c_int64),
        ("arena_edges", ctypes.c_int64), ("issued_flop_per_board", ctypes.c_double),
        ("arena_pool_edges", ctypes.c_int64), ("arena_pool_high", ctypes.c_int64),
        ("issued_flop_per_board_small", ctypes.c_double), ("tower_small_max_boards", ctypes.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# az_eval_fn (include/az.h): (user, x [n][H][W][4], n, probs [n][A], values [n]) -> 0 / nonzero
EVAL_FN = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int32,
                           ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float))


def _as_numpy(t):
    """A model output (numpy, torch or TF tensor, list) as a numpy array."""
    if hasattr(t, "detach"):
        t = t.detach().cpu()
    if hasattr(t, "numpy"):
        t = t.numpy()
    return np.asarray(t)


EXPORTED = (
    "az_abi_version", "az_last_error", "az_build_id", "az_build_flags", "az_engine_create", "az_engine_destroy",
    "az_engine_lanes",
    "az_engine_set_weights", "az_encode", "az_forward", "az_selfplay_begin", "az_selfplay_step",
    "az_selfplay_run", "az_selfplay_results", "az_selfplay_drain", "az_tree_reset", "az_tree_release", "az_tree_search", "az_tree_search_noise", "az_tree_play",
    "az_tree_info", "az_tree_export", "az_stats_get", "az_timer_enable", "az_pow_table",
    "az_cache_clear", "az_cache_enable", "az_engine_set_evaluator",
    "az_trainer_create", "az_trainer_destroy", "az_trainer_set_weights", "az_trainer_reset_momentum",
    "az_trainer_read", "az_trainer_step",
    # include/az_chess.h
    "az_chess_all_moves", "az_chess_legal", "az_chess_encode", "az_chess_play", "az_chess_perft",
    "az_chess_engine_create", "az_chess_engine_destroy", "az_chess_engine_set_weights",
    "az_chess_engine_set_evaluator",
    "az_chess_forward", "az_chess_selfplay_begin", "az_chess_selfplay_step", "az_chess_selfplay_run",
    "az_chess_selfplay_results", "az_chess_selfplay_drain", "az_chess_stats", "az_chess_timer_enable",
    "az_chess_tree_reset",
    "az_chess_tree_release", "az_chess_tree_search", "az_chess_tree_search_noise", "az_chess_tree_play", "az_chess_tree_info",
    "az_chess_tree_export", "az_chess_trainer_create",
    "az_chess_replay_create", "az_chess_replay_destroy", "az_chess_replay_push", "az_chess_replay_size",
    "az_chess_replay_clear", "az_chess_replay_gather", "az_trainer_step_replay",
    # the exact Connect-N solver (include/az.h)
    "az_solver_create", "az_solver_destroy", "az_solver_clear", "az_solver_configure", "az_solver_solve",
    "az_solver_book_begin", "az_solver_book_solve", "az_solver_book_finish", "az_solver_book_save",
    "az_solver_book_load", "az_solver_book_info", "az_solver_book_level",
)

_lib = None


def load_library():
    """Load libaz.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("AZ_LIB_PATH", LIB_PATH)  # A/B builds (profiles/); default in-tree lib
    if not os.path.exists(path):
        raise AzError(f"libaz.so not built at {path}; run __graft_entry__.build()")
    # One HIP runtime per process: torch's wheel bundles its own libamdhip64 /
    # libhsa-runtime64 with the same SONAMEs as /opt/rocm's.  Loading torch
    # first makes libaz bind to that already-loaded runtime (SONAME match);
    # the reverse order leaves two runtimes and torch then sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sig = {
        "az_abi_version": (ctypes.c_int, []),
        "az_last_error": (ctypes.c_char_p, []),
        "az_build_id": (ctypes.c_char_p, []),
        "az_build_flags": (ctypes.c_char_p, []),
        "az_engine_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Config), ctypes.POINTER(P)]),
        "az_engine_destroy": (ctypes.c_int, [P]),
        "az_engine_lanes": (ctypes.c_int, [P]),
        "az_engine_set_weights": (ctypes.c_int, [P, ctypes.POINTER(Tensor), ctypes.c_int]),
        "az_encode": (ctypes.c_int, [P, P, ctypes.c_int, P, P]),
        "az_forward": (ctypes.c_int, [P, P, ctypes.c_int, P, P]),
        "az_selfplay_begin": (ctypes.c_int, [P, I64, I64, ctypes.c_uint32]),
        "az_selfplay_step": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(Stats)]),
        "az_selfplay_run": (ctypes.c_int, [P, I64, I64, ctypes.c_uint32, ctypes.POINTER(Stats)]),
        "az_selfplay_results": (ctypes.c_int, [P, P, P, P, P, P, P]),
        "az_selfplay_drain": (ctypes.c_int, [P, I64, P, P, P, P, P, P, P, P]),
        "az_tree_reset": (ctypes.c_int, [P, ctypes.c_int, P, P]),
        "az_tree_release": (ctypes.c_int, [P, ctypes.c_int, P]),
        "az_tree_search": (ctypes.c_int, [P, ctypes.c_int]),
        "az_tree_search_noise": (ctypes.c_int, [P, ctypes.c_int, P, ctypes.c_int]),
        "az_tree_play": (ctypes.c_int, [P, P, ctypes.c_int, ctypes.c_int, P, P, P]),
        "az_tree_info": (ctypes.c_int, [P, ctypes.c_int, P, P]),
        "az_tree_export": (ctypes.c_int, [P, ctypes.c_int, P, P, P, P, P, P, P]),
        "az_stats_get": (ctypes.c_int, [P, ctypes.POINTER(Stats)]),
        "az_timer_enable": (ctypes.c_int, [P, ctypes.c_int]),
        "az_pow_table": (ctypes.c_int, [P, P, I64]),
        "az_cache_clear": (ctypes.c_int, [P]),
        "az_cache_enable": (ctypes.c_int, [P, ctypes.c_int]),
        "az_engine_set_evaluator": (ctypes.c_int, [P, EVAL_FN, P]),
        "az_trainer_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Config), ctypes.c_int,
                                             ctypes.POINTER(P)]),
        "az_trainer_destroy": (ctypes.c_int, [P]),
        "az_trainer_set_weights": (ctypes.c_int, [P, ctypes.POINTER(Tensor), ctypes.c_int]),
        "az_trainer_reset_momentum": (ctypes.c_int, [P]),
        "az_trainer_read": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_char_p, P, I64]),
        "az_trainer_step": (ctypes.c_int, [P, P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double, ctypes.c_double, P]),
        "az_chess_all_moves": (ctypes.c_int, [P, ctypes.c_int]),
        "az_chess_legal": (ctypes.c_int, [ctypes.c_int, P, ctypes.c_int, P, P, P, P]),
        "az_chess_encode": (ctypes.c_int, [ctypes.c_int, P, P, ctypes.c_int, P]),
        "az_chess_play": (ctypes.c_int, [ctypes.c_int, P, P, ctypes.c_int, ctypes.c_int]),
        "az_chess_perft": (ctypes.c_int, [ctypes.c_int, P, ctypes.c_int, P]),
        "az_chess_engine_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ChessConfig),
                                                  ctypes.POINTER(P)]),
        "az_chess_engine_destroy": (ctypes.c_int, [P]),
        "az_chess_engine_set_weights": (ctypes.c_int, [P, ctypes.POINTER(Tensor), ctypes.c_int]),
        "az_chess_engine_set_evaluator": (ctypes.c_int, [P, EVAL_FN, P]),
        "az_chess_forward": (ctypes.c_int, [P, P, ctypes.c_int, P, P]),
        "az_chess_selfplay_begin": (ctypes.c_int, [P, I64, I64, ctypes.c_uint32]),
        "az_chess_selfplay_step": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(Stats)]),
        "az_chess_selfplay_run": (ctypes.c_int, [P, I64, I64, ctypes.c_uint32, ctypes.POINTER(Stats)]),
        "az_chess_selfplay_results": (ctypes.c_int, [P] + [P] * 9),
        "az_chess_selfplay_drain": (ctypes.c_int, [P, I64, P] + [P] * 10),
        "az_chess_stats": (ctypes.c_int, [P, ctypes.POINTER(Stats)]),
        "az_chess_timer_enable": (ctypes.c_int, [P, ctypes.c_int]),
        "az_chess_tree_reset": (ctypes.c_int, [P, ctypes.c_int, P, P]),
        "az_chess_tree_release": (ctypes.c_int, [P, ctypes.c_int, P]),
        "az_chess_tree_search": (ctypes.c_int, [P, ctypes.c_int]),
        "az_chess_tree_search_noise": (ctypes.c_int, [P, ctypes.c_int, P, ctypes.c_int]),
        "az_chess_tree_play": (ctypes.c_int, [P, P, ctypes.c_int, ctypes.c_int, P, P, P, P, P]),
        "az_chess_tree_info": (ctypes.c_int, [P, ctypes.c_int, P, P]),
        "az_chess_tree_export": (ctypes.c_int, [P, ctypes.c_int, P, P, P, P, P, P, P]),
        "az_chess_trainer_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ChessConfig), ctypes.c_int,
                                                   ctypes.POINTER(P)]),
        "az_chess_replay_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(P)]),
        "az_chess_replay_destroy": (ctypes.c_int, [P]),
        "az_chess_replay_push": (ctypes.c_int, [P, P, P, P, P, P, P, I64]),
        "az_chess_replay_size": (ctypes.c_int, [P, ctypes.POINTER(I64), ctypes.POINTER(I64)]),
        "az_chess_replay_clear": (ctypes.c_int, [P]),
        "az_chess_replay_gather": (ctypes.c_int, [P, P, ctypes.c_int, P, P, P]),
        "az_trainer_step_replay": (ctypes.c_int, [P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                  ctypes.c_double, ctypes.c_double, P]),
        "az_solver_create": (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(P)]),
        "az_solver_destroy": (ctypes.c_int, [P]),
        "az_solver_clear": (ctypes.c_int, [P]),
        "az_solver_configure": (ctypes.c_int, [P, ctypes.c_int, I64, ctypes.c_int]),
        "az_solver_solve": (ctypes.c_int, [P, P, I64, I64, P, P, P]),
        "az_solver_book_begin": (ctypes.c_int, [P, ctypes.c_int, P]),
        "az_solver_book_solve": (ctypes.c_int, [P, I64, I64, ctypes.POINTER(I64), ctypes.POINTER(I64)]),
        "az_solver_book_finish": (ctypes.c_int, [P]),
        "az_solver_book_save": (ctypes.c_int, [P, ctypes.c_char_p]),
        "az_solver_book_load": (ctypes.c_int, [P, ctypes.c_char_p]),
        "az_solver_book_info": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32), P]),
        "az_solver_book_level": (ctypes.c_int, [P, ctypes.c_int, I64, I64, I64, P, P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _ = I32
    _lib = L
    return L


def build_id():
    """(source hash, extra compile flags) of the loaded libaz (az_build_id /
    az_build_flags): profiles record the hash, bench.py matches it."""
    L = load_library()
    return L.az_build_id().decode(), L.az_build_flags().decode()


def _check(rc):
    if rc != 0:
        msg = load_library().az_last_error().decode("utf-8", "replace")
        raise AzError(f"libaz error {rc}: {msg}")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def tensor_array(named):
    """(name, numpy array or torch tensor) pairs -> az_tensor array; torch
    CUDA tensors are passed as device pointers (the engine copies them)."""
    keep, items = [], []
    for name, t in named:
        on_dev = 0
        if hasattr(t, "is_cuda"):
            t = t.detach().float().contiguous()
            on_dev = int(t.is_cuda)
            if not on_dev:
                t = t.numpy()
        if on_dev:
            ptr, numel = t.data_ptr(), t.numel()
        else:
            t = np.ascontiguousarray(t, np.float32)
            ptr, numel = t.ctypes.data, t.size
        keep.append(t)
        items.append(Tensor(name.encode(), ptr, numel, on_dev, 0))
    arr = (Tensor * len(items))(*items)
    if any(i.on_device for i in items):
        import torch
        torch.cuda.synchronize()
    return arr, len(items), keep


class _EngineBase:
    """What Engine and ChessEngine share: the handle's life, weights, the host
    evaluator's trampoline, the self-play calls and the chunked drain loop.
    _ABI is the class's prefix of the libaz symbols, _STATS its stats symbol."""

    _ABI = _STATS = None

    def _call(self, name, *args):
        return getattr(self._L, self._ABI + name)(self._h, *args)

    def _attach(self, handle, L):
        self._h, self._L, self._n_games = handle, L, 0
        self._host_fn = None     # the EVAL_FN object (kept alive while the engine may call it)
        self._host_error = None  # an exception the host evaluator raised inside a search

    def close(self):
        if getattr(self, "_h", None):
            self._call("engine_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter teardown
            pass

    def set_weights(self, named):
        """named: iterable of (name, array-like or torch tensor)."""
        arr, n, _keep = tensor_array(named)
        _check(self._call("engine_set_weights", arr, n))

    def _set_host_evaluator(self, fn, row_shape, actions, strict):
        """fn(x [n, *row_shape]) -> (probs [n, actions], values [n] or [n, 1]) as
        the engine's az_eval_fn.  strict: outputs of any other shape raise
        ValueError; otherwise they are reshaped."""
        A = actions

        def cb(_user, xp, n, pp, vp):
            try:
                x = np.ctypeslib.as_array(xp, shape=(n,) + row_shape).copy()
                p, v = fn(x)
                p = _as_numpy(p).astype(np.float32, copy=False)
                v = _as_numpy(v).astype(np.float32, copy=False)
                if strict and p.shape != (n, A):
                    raise ValueError(f"the host evaluator returned probs of shape {p.shape}, expected {(n, A)}")
                if strict and v.shape not in ((n,), (n, 1)):
                    raise ValueError(f"the host evaluator returned values of shape {v.shape}, "
                                     f"expected {(n,)} or {(n, 1)}")
                np.ctypeslib.as_array(pp, shape=(n, A))[:] = p.reshape(n, A)
                np.ctypeslib.as_array(vp, shape=(n,))[:] = v.reshape(n)
                return 0
            except BaseException as ex:  # noqa: BLE001 - handed back to the caller below
                self._host_error = ex
                return 1

        host_fn = EVAL_FN(cb)
        _check(self._call("engine_set_evaluator", host_fn, None))
        self._host_fn = host_fn

    def _search_call(self, rc):
        """_check for calls that can run the host evaluator: its exception first."""
        if self._host_error is not None:
            ex, self._host_error = self._host_error, None
            raise ex
        _check(rc)

    def selfplay_begin(self, first_game, n_games, base_seed):
        _check(self._call("selfplay_begin", int(first_game), int(n_games), int(base_seed) & 0xFFFFFFFF))
        self._n_games = int(n_games)

    def selfplay_step(self, n_moves=1, sync=True):
        """Enqueue n_moves moves for every slot.  sync=False returns at once
        (no stats): the moves run while the caller drains earlier ones --
        selfplay_drain then returns the games of the newest move whose
        snapshot is complete and waits at most for the move before the
        running one (*_selfplay_step with st = NULL)."""
        st = Stats() if sync else None
        self._search_call(self._call("selfplay_step", int(n_moves), ctypes.byref(st) if sync else None))
        return st.as_dict() if sync else None

    def selfplay_run(self, first_game, n_games, base_seed):
        st = Stats()
        self._search_call(self._call("selfplay_run", int(first_game), int(n_games), int(base_seed) & 0xFFFFFFFF,
                                     ctypes.byref(st)))
        self._n_games = int(n_games)
        return st.as_dict()

    def _drain(self, max_games, chunk, buffers):
        """The drain loop: buffers(G) makes the out arrays for G games, keyed in
        the order *_selfplay_drain takes them.  Drained in chunks of `chunk`
        games, so a call allocates for what it returns, not for the whole batch."""
        left = int(max_games if max_games is not None else max(self._n_games, 1))
        parts = []
        while left > 0:
            G = min(chunk, left)
            n = ctypes.c_int64(0)
            out = buffers(G)
            _check(self._call("selfplay_drain", G, ctypes.byref(n), *(_ptr(v) for v in out.values())))
            k = int(n.value)
            parts.append({key: v[:k] for key, v in out.items()} if k < G else out)
            left -= k
            if k < G:
                break
        if len(parts) == 1:
            p = parts[0]
            return {key: (v.copy() if v.base is not None else v) for key, v in p.items()}
        return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}

    def stats(self):
        st = Stats()
        _check(getattr(self._L, self._STATS)(self._h, ctypes.byref(st)))
        return st.as_dict()


class Engine(_EngineBase):
    """One libaz engine: one device, one HIP stream, `slots` concurrent trees."""

    _ABI, _STATS = "az_", "az_stats_get"

    def __init__(self, height=6, width=7, n=4, gravity=True, mcts_iterations=100, slots=1,
                 evaluator=EVAL_NETWORK, index_move_greedy=8, exploration_constant=1.5,
                 filters=128, depth=4, value_hidden=256, bn_epsilon=1e-3, arena_edges=0,
                 max_tree_visits=0, device=0, cache_log2=0, conv_algo=CONV_F16X2,
                 lanes=0, compact=False, tower_natural_order=False, dirichlet_noise=False,
                 dirichlet_alpha=0.03, dirichlet_ratio=0.25, rng_skip=None):
        """compact=True reclaims the subtrees a self-play game has left after
        every move (az_config.compact; arena_edges is then per half); keep it
        off for the tree API (az_tree_*), whose views need the whole tree.
        dirichlet_noise: ConfigMCTS.enable_dirichlet_noise (root noise,
        reference mcts.py:70-85) with dirichlet_alpha / dirichlet_ratio.
        rng_skip: MT19937 words a self-play game's stream discards after
        seeding; None = the reference play_game's model construction
        (np.random.rand(1, H, W, 4): 2 H W 4 words), so game g of a batch is
        the reference's play_game under np.random.seed(base_seed + g)."""
        L = load_library()
        self.height, self.width, self.n, self.gravity = height, width, n, bool(gravity)
        self.action_space = width if gravity else width * height
        self.slots = slots
        self.mcts_iterations = mcts_iterations
        cfg = Config(board_height=height, board_width=width, n=n, gravity=int(bool(gravity)),
                     mcts_iterations=mcts_iterations, index_move_greedy=index_move_greedy,
                     exploration_constant=exploration_constant, slots=slots, evaluator=evaluator,
                     filters=filters, depth=depth, value_hidden=value_hidden,
                     bn_epsilon=bn_epsilon, arena_edges=arena_edges,
                     max_tree_visits=max_tree_visits, cache_log2=cache_log2, conv_algo=conv_algo,
                     lanes=lanes, compact=int(bool(compact)),
                     tower_natural_order=int(bool(tower_natural_order)),
                     dirichlet_noise=int(bool(dirichlet_noise)), dirichlet_alpha=float(dirichlet_alpha),
                     dirichlet_ratio=float(dirichlet_ratio),
                     rng_skip=2 * height * width * 4 if rng_skip is None else int(rng_skip))
        handle = ctypes.c_void_p()
        _check(L.az_engine_create(int(device), ctypes.byref(cfg), ctypes.byref(handle)))
        self._attach(handle, L)

    @property
    def lanes(self):
        """The slot groups (streams) the engine runs (az_engine_lanes)."""
        return int(self._L.az_engine_lanes(self._h))

    def set_host_evaluator(self, fn):
        """EVAL_HOST engines: fn(x) with x [n, H, W, 4] float32 full_state planes
        returns (probs [n, A], values [n] or [n, 1]) -- the reference's
        self.model(x) call (mcts.py:130-137), here once per simulation over
        every leaf that needs an evaluation.  Outputs may be numpy arrays or
        torch / TF tensors.  An exception inside fn ends the search and is
        re-raised by the call that ran it."""
        self._set_host_evaluator(fn, (self.height, self.width, 4), self.action_space, strict=False)

    # ------------------------------------------------------------- eval
    def encode(self, boards):
        b = np.ascontiguousarray(boards, np.int8).reshape(-1, self.height, self.width)
        state = np.zeros(b.shape + (4,), np.float32)
        mask = np.zeros((len(b), self.action_space), np.uint8)
        _check(self._L.az_encode(self._h, _ptr(b), len(b), _ptr(state), _ptr(mask)))
        return state, mask.astype(bool)

    def forward(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.height, self.width, 4)
        probs = np.zeros((len(x), self.action_space), np.float32)
        values = np.zeros(len(x), np.float32)
        _check(self._L.az_forward(self._h, _ptr(x), len(x), _ptr(probs), _ptr(values)))
        return probs, values

    # ------------------------------------------------------------- self-play
    def selfplay_results(self):
        G, P, A = self._n_games, self.height * self.width, self.action_space
        lengths = np.zeros(G, np.int32)
        results = np.zeros(G, np.int32)
        expansions = np.zeros(G, np.int32)
        boards = np.zeros((G, P, self.height, self.width), np.int8)
        policies = np.zeros((G, P, A), np.float64)
        moves = np.zeros((G, P), np.int32)
        _check(self._L.az_selfplay_results(self._h, _ptr(lengths), _ptr(results), _ptr(expansions),
                                           _ptr(boards), _ptr(policies), _ptr(moves)))
        return dict(lengths=lengths, results=results, expansions=expansions, boards=boards,
                    policies=policies, moves=moves)

    def selfplay_drain(self, max_games=None, chunk=4096):
        """Games finished since the previous drain, copied to the host (the
        samples of a running batch, az_selfplay_drain): dict of arrays with
        a leading game axis plus `game_ids` (finish order), in chunks of
        `chunk` games."""
        P, A = self.height * self.width, self.action_space
        return self._drain(max_games, chunk, lambda G: dict(
            game_ids=np.zeros(G, np.int64), lengths=np.zeros(G, np.int32),
            results=np.zeros(G, np.int32), expansions=np.zeros(G, np.int32),
            boards=np.zeros((G, P, self.height, self.width), np.int8),
            policies=np.zeros((G, P, A), np.float64), moves=np.zeros((G, P), np.int32)))

    # ------------------------------------------------------------- tree API
    def tree_reset(self, slots, boards):
        slots = np.ascontiguousarray(slots, np.int32)
        b = np.ascontiguousarray(boards, np.int8).reshape(len(slots), self.height, self.width)
        _check(self._L.az_tree_reset(self._h, len(slots), _ptr(slots), _ptr(b)))

    def tree_release(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        _check(self._L.az_tree_release(self._h, len(slots), _ptr(slots)))

    def tree_search(self, n_sims, noise=None):
        """noise (engines made with dirichlet_noise): [slots, rows, A] float64,
        row r of slot s the np.random.dirichlet vector its r-th root selection
        mixes in (az_tree_search_noise)."""
        if noise is None:
            self._search_call(self._L.az_tree_search(self._h, int(n_sims)))
            return
        noise = np.ascontiguousarray(noise, np.float64)
        if noise.ndim != 3 or noise.shape[0] != self.slots or noise.shape[2] != self.action_space:
            raise ValueError(f"noise must be [slots={self.slots}, rows, A={self.action_space}], got {noise.shape}")
        self._search_call(self._L.az_tree_search_noise(self._h, int(n_sims), _ptr(noise), int(noise.shape[1])))

    def tree_play(self, uniforms=None, greedy=False, deterministic=False):
        S, A = self.slots, self.action_space
        u = None if deterministic else np.ascontiguousarray(uniforms, np.float64).reshape(S)
        moves = np.zeros(S, np.int32)
        status = np.zeros(S, np.int32)
        policy = np.zeros((S, A), np.float64)
        _check(self._L.az_tree_play(self._h, _ptr(u), int(bool(greedy)), int(bool(deterministic)),
                                    _ptr(moves), _ptr(status), _ptr(policy)))
        return moves, status, policy

    def tree_info(self, slot):
        """The slot's tree header alone (az_tree_info: no edge copy)."""
        info = np.zeros(5, np.int64)
        rv = np.zeros(1, np.float32)
        _check(self._L.az_tree_info(self._h, int(slot), _ptr(info), _ptr(rv)))
        return dict(arena_top=int(info[0]), root_first=int(info[1]), root_n=int(info[2]), ply=int(info[3]),
                    active=bool(info[4]), root_value=float(rv[0]))

    def tree_export(self, slot):
        info = np.zeros(5, np.int64)
        rv = np.zeros(1, np.float32)
        _check(self._L.az_tree_info(self._h, int(slot), _ptr(info), _ptr(rv)))
        n = int(info[0])
        out = {
            "prior": np.zeros(n, np.float64), "w": np.zeros(n, np.float64),
            "n": np.zeros(n, np.int32), "child": np.zeros(n, np.int32),
            "child_n": np.zeros(n, np.int32), "action": np.zeros(n, np.int32),
            "child_value": np.zeros(n, np.float32),
        }
        _check(self._L.az_tree_export(self._h, int(slot), _ptr(out["prior"]), _ptr(out["w"]),
                                      _ptr(out["n"]), _ptr(out["child"]), _ptr(out["child_n"]),
                                      _ptr(out["action"]), _ptr(out["child_value"])))
        out.update(arena_top=n, root_first=int(info[1]), root_n=int(info[2]), ply=int(info[3]),
                   active=bool(info[4]), root_value=float(rv[0]))
        return out

    # ------------------------------------------------------------- misc
    def cache_clear(self):
        _check(self._L.az_cache_clear(self._h))

    def cache_enable(self, on=True):
        _check(self._L.az_cache_enable(self._h, int(bool(on))))

    def timer(self, on, tree=False, every=1):
        """HIP-event timing of the network launches (az_stats conv_*); tree:
        the select and expand launches too; every >= 3: every `every`-th
        network launch of each lane only (conv_launches counts those)."""
        if every not in (1,) and every < 3:
            raise ValueError("every: 1 or >= 3")
        _check(self._L.az_timer_enable(self._h, (every if every >= 3 else 2 if tree else 1) if on else 0))

    def pow_table(self, n):
        out = np.zeros(int(n), np.float64)
        _check(self._L.az_pow_table(self._h, _ptr(out), int(n)))
        return out


TRAIN_WEIGHT, TRAIN_GRAD, TRAIN_MOMENTUM = 0, 1, 2  # include/az.h AZ_TRAIN_*


class Trainer:
    """One libaz trainer (az_trainer_*, csrc/az_train.hip): the training step
    of the policy/value network -- forward with batch statistics, backward,
    SGD with momentum -- on one device and a stream of its own.  It owns its
    weights, gradients and momentum; tensors go in and out by their
    weights.weight_spec names in Keras layout.  This class is the Connect-N
    network's (4 input planes); ChessTrainer below is the chess network's."""

    planes = 4

    def __init__(self, height=6, width=7, gravity=True, max_batch=256, filters=128, depth=4,
                 value_hidden=256, bn_epsilon=1e-3, device=0):
        from custom_alphazero.model.weights import weight_spec
        L = load_library()
        self.height, self.width, self.gravity = int(height), int(width), bool(gravity)
        self.action_space = self.width if self.gravity else self.width * self.height
        self.max_batch = int(max_batch)
        self.spec = weight_spec(self.height, self.width, self.action_space, filters, max(int(depth), 0),
                                value_hidden, self.planes)
        cfg = Config(board_height=self.height, board_width=self.width, n=min(4, self.height, self.width),
                     gravity=int(self.gravity), filters=filters, depth=depth, value_hidden=value_hidden,
                     bn_epsilon=bn_epsilon)
        handle = ctypes.c_void_p()
        _check(L.az_trainer_create(int(device), ctypes.byref(cfg), self.max_batch, ctypes.byref(handle)))
        self._h = handle
        self._L = L

    def close(self):
        if getattr(self, "_h", None):
            self._L.az_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter teardown
            pass

    def set_weights(self, named):
        """named: iterable of (name, array-like or torch tensor), every tensor
        of the spec.  Momentum is left as it is (zero at creation)."""
        arr, n, _keep = tensor_array(named)
        _check(self._L.az_trainer_set_weights(self._h, arr, n))

    def reset_momentum(self):
        _check(self._L.az_trainer_reset_momentum(self._h))

    def read(self, name, what=TRAIN_WEIGHT):
        """One tensor (Keras layout) as a float32 numpy array: the weight, or
        the last step's gradient of the total loss, or the momentum buffer."""
        shape = dict(self.spec).get(name)
        out = np.zeros(shape if shape is not None else (1,), np.float32)
        _check(self._L.az_trainer_read(self._h, int(what), name.encode(), _ptr(out), out.size))
        return out

    def read_all(self, what=TRAIN_WEIGHT):
        names = [n for n, _ in self.spec
                 if what == TRAIN_WEIGHT or n.rsplit(".", 1)[1] not in ("mean", "var")]
        return {n: self.read(n, what) for n in names}

    def step(self, x, pi, z, lr, momentum=0.9, l2=1e-4, bn_momentum=0.99):
        """One SGD step on the batch x [n, H, W, planes], pi [n, A], z [n]; returns
        (total, policy, value) losses of the weights before the update."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.height, self.width, self.planes)
        n = len(x)
        pi = np.ascontiguousarray(pi, np.float32).reshape(n, self.action_space)
        z = np.ascontiguousarray(z, np.float32).reshape(n)
        losses = np.zeros(3, np.float32)
        _check(self._L.az_trainer_step(self._h, _ptr(x), _ptr(pi), _ptr(z), n, float(lr), float(momentum),
                                       float(l2), float(bn_momentum), _ptr(losses)))
        return float(losses[0]), float(losses[1]), float(losses[2])

    def step_replay(self, replay, idx, lr, momentum=0.9, l2=1e-4, bn_momentum=0.99):
        """step on the samples idx of a ChessReplay window, gathered on the
        device into the step's own input buffers (az_trainer_step_replay):
        returns what step(*replay.gather(idx), ...) returns, bit for bit.
        The chess trainer's; on this Connect-N class the library refuses."""
        idx = np.ascontiguousarray(idx, np.int64).reshape(-1)
        losses = np.zeros(3, np.float32)
        _check(self._L.az_trainer_step_replay(self._h, replay._h, _ptr(idx), len(idx), float(lr),
                                              float(momentum), float(l2), float(bn_momentum), _ptr(losses)))
        return float(losses[0]), float(losses[1]), float(losses[2])


class ChessTrainer(Trainer):
    """The trainer of the chess network (az_chess_trainer_create): the
    (8, 8, 118) Board.full_state planes and the 1880-move action space, with
    Trainer's methods.  step takes x [n, 8, 8, 118], pi [n, 1880], z [n]."""

    planes = 118

    def __init__(self, max_batch=256, filters=128, depth=4, value_hidden=256, bn_epsilon=1e-3, device=0):
        from custom_alphazero.model.weights import weight_spec
        L = load_library()
        self.height = self.width = 8
        self.gravity = False
        self.action_space = ChessEngine.ACTIONS
        self.max_batch = int(max_batch)
        self.spec = weight_spec(8, 8, self.action_space, filters, max(int(depth), 0), value_hidden, self.planes)
        cfg = ChessConfig(filters=filters, depth=depth, value_hidden=value_hidden, bn_epsilon=bn_epsilon)
        handle = ctypes.c_void_p()
        _check(L.az_chess_trainer_create(int(device), ctypes.byref(cfg), self.max_batch, ctypes.byref(handle)))
        self._h = handle
        self._L = L


def chess_replay_records(results, start=None):
    """The samples of finished chess games as ChessReplay.push takes them, from
    the dict of ChessEngine.selfplay_results() or selfplay_drain(): every ply
    of every game, in game order, with the history self_play.play_chess gives
    it -- [0 x 7, pos] for a game's first ply, [0 x 6, start, pos] afterwards
    (start: the start position's record, default Board()'s) -- its sparse
    policy row, and z = self_play.alternating_rewards(result, T) as float32.
    Host bookkeeping only: no device work."""
    from custom_alphazero.chess import kernels as K
    from custom_alphazero.self_play import alternating_rewards
    if start is None:
        from custom_alphazero.chess.board import Board as ChessBoard
        start = ChessBoard()._pos
    lengths = np.asarray(results["lengths"]).astype(np.int64)
    hist, valid, z, rows = [], [], [], []
    for g, T in enumerate(lengths):
        T = int(T)
        h = np.zeros((T, K.HISTORY), K.POS_DTYPE)
        v = np.zeros((T, K.HISTORY), np.uint8)
        h[:, 7], v[:, 7] = results["positions"][g, :T], 1
        h[1:, 6], v[1:, 6] = start, 1
        hist.append(h)
        valid.append(v)
        z.append(np.asarray(alternating_rewards(int(results["results"][g]), T), np.float64).astype(np.float32))
        rows.append((np.full(T, g), np.arange(T)))
    gi = np.concatenate([r[0] for r in rows]) if rows else np.zeros(0, np.int64)
    ti = np.concatenate([r[1] for r in rows]) if rows else np.zeros(0, np.int64)
    M = ChessEngine.MAX_MOVES
    return dict(
        hist=np.concatenate(hist) if hist else np.zeros((0, K.HISTORY), K.POS_DTYPE),
        valid=np.concatenate(valid) if valid else np.zeros((0, K.HISTORY), np.uint8),
        policy_n=np.ascontiguousarray(np.asarray(results["policy_n"])[gi, ti], np.int32).reshape(-1),
        policy_actions=np.ascontiguousarray(np.asarray(results["policy_actions"])[gi, ti], np.int16).reshape(-1, M),
        policy_probs=np.ascontiguousarray(np.asarray(results["policy_probs"])[gi, ti], np.float64).reshape(-1, M),
        z=np.concatenate(z) if z else np.zeros(0, np.float32))


class ChessReplay:
    """The chess replay window on the device (az_chess_replay_*,
    csrc/az_replay.hip): a ring of the newest `capacity` samples in the compact
    form self-play produces (8 history positions, the sparse policy, the value;
    about 3.2 KB a sample), from which ChessTrainer.step_replay trains without
    a dense state ever being built on the host.  Index 0 is the oldest sample
    held, len(replay) - 1 the newest: the row order of train.training_loop's
    host window, so the same np.random.choice indices name the same samples.
    One thread drives a replay and the trainer stepping from it."""

    KEYS = ("hist", "valid", "policy_n", "policy_actions", "policy_probs", "z")

    def __init__(self, capacity, device=0):
        L = load_library()
        handle = ctypes.c_void_p()
        _check(L.az_chess_replay_create(int(device), int(capacity), ctypes.byref(handle)))
        self._h, self._L = handle, L
        self.capacity = int(capacity)

    def close(self):
        if getattr(self, "_h", None):
            self._L.az_chess_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter teardown
            pass

    def __len__(self):
        size = ctypes.c_int64(0)
        _check(self._L.az_chess_replay_size(self._h, ctypes.byref(size), None))
        return int(size.value)

    def push(self, hist, valid, policy_n, policy_actions, policy_probs, z):
        """Append n samples in order: hist [n, 8] positions (POS_DTYPE) oldest
        first and valid [n, 8] as chess.kernels.encode takes them, policy_n [n],
        policy_actions [n, 256], policy_probs [n, 256] float64, z [n].  A row
        with policy_n outside 0..256, a used action outside 0..1879 or an
        action used twice raises AzError and leaves the window unchanged."""
        from custom_alphazero.chess.kernels import HISTORY, POS_DTYPE
        M = ChessEngine.MAX_MOVES
        pn = np.ascontiguousarray(policy_n, np.int32).reshape(-1)
        n = len(pn)
        h = np.ascontiguousarray(hist, POS_DTYPE).reshape(n, HISTORY)
        v = np.ascontiguousarray(valid, np.uint8).reshape(n, HISTORY)
        pa = np.ascontiguousarray(policy_actions, np.int16).reshape(n, M)
        pp = np.ascontiguousarray(policy_probs, np.float64).reshape(n, M)
        zz = np.ascontiguousarray(z, np.float32).reshape(n)
        _check(self._L.az_chess_replay_push(self._h, _ptr(h), _ptr(v), _ptr(pn), _ptr(pa), _ptr(pp), _ptr(zz), n))

    def push_games(self, results, start=None):
        """Push every ply of the finished games in `results` (the dict of
        ChessEngine.selfplay_results() or selfplay_drain()), in game order, as
        self_play.play_chess builds its samples (chess_replay_records)."""
        self.push(**chess_replay_records(results, start))

    def gather(self, idx):
        """-> (x [n, 8, 8, 118], pi [n, 1880], z [n]) float32: the samples idx in
        the dense form Trainer.step takes (az_chess_replay_gather)."""
        idx = np.ascontiguousarray(idx, np.int64).reshape(-1)
        n = len(idx)
        x = np.zeros((n, 8, 8, 118), np.float32)
        pi = np.zeros((n, ChessEngine.ACTIONS), np.float32)
        z = np.zeros(n, np.float32)
        _check(self._L.az_chess_replay_gather(self._h, _ptr(idx), n, _ptr(x), _ptr(pi), _ptr(z)))
        return x, pi, z

    def clear(self):
        _check(self._L.az_chess_replay_clear(self._h))


SOLVER_SOLVED, SOLVER_UNSOLVED = 0, 1
BOOK_NONE, BOOK_BUILDING, BOOK_FINISHED = 0, 1, 2
BOOK_NO_SCORE = -128


class Solver:
    """The exact Connect-N solver on the device (az_solver_*, csrc/az_solver.hip):
    alpha-beta over bitboards, one search per GPU lane, a batch of positions
    per call.  Gravity boards with W <= 16 and W * (H + 1) <= 56.  The
    transposition table (2^tt_log2 words of 8 bytes) lives as long as the
    handle; clear() empties it."""

    def __init__(self, height=6, width=7, n=4, tt_log2=24, device=0):
        L = load_library()
        handle = ctypes.c_void_p()
        _check(L.az_solver_create(int(device), int(height), int(width), int(n), int(tt_log2), ctypes.byref(handle)))
        self._h, self._L = handle, L
        self.height, self.width, self.n = int(height), int(width), int(n)

    def close(self):
        if getattr(self, "_h", None):
            self._L.az_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter teardown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def configure(self, split_stones=0, max_jobs=0, steps_per_launch=0):
        """split_stones: positions with fewer stones are expanded on the host to
        those with that many and backed up (a frontier over max_jobs comes back
        unsolved); steps_per_launch: search steps per kernel launch.  0 keeps a value."""
        _check(self._L.az_solver_configure(self._h, int(split_stones), int(max_jobs), int(steps_per_launch)))

    def clear(self):
        _check(self._L.az_solver_clear(self._h))

    def solve(self, boards, node_budget):
        """boards [count, H, W] int8 as Board.array, +1 the side to move's stones
        (negate the array when black is to move) -> (scores int32, status uint8,
        nodes int64), each [count].  status SOLVER_UNSOLVED: the position's search
        passed node_budget nodes (or its split passed max_jobs); its score is not valid."""
        b = np.ascontiguousarray(boards, np.int8).reshape(-1, self.height, self.width)
        count = len(b)
        scores = np.zeros(count, np.int32)
        status = np.zeros(count, np.uint8)
        nodes = np.zeros(count, np.int64)
        _check(self._L.az_solver_solve(self._h, _ptr(b), count, int(node_budget), _ptr(scores), _ptr(status),
                                       _ptr(nodes)))
        return scores, status, nodes

    # ---- the opening book (az_solver_book_*, csrc/az_book.hip)
    def book_begin(self, depth):
        """Enumerates every reachable unfinished position with 0..depth stones,
        reduced by the left-right mirror, on the device; replaces any book the
        solver had.  -> the level counts, int64 [depth + 1]."""
        counts = np.zeros(int(depth) + 1 if depth >= 0 else 1, np.int64)
        _check(self._L.az_solver_book_begin(self._h, int(depth), _ptr(counts)))
        return counts

    def book_solve(self, max_positions, node_budget):
        """Searches up to max_positions deepest-level positions that have no score
        yet -> (remaining, unsolved): positions still without a score, and those of
        this call whose search passed node_budget (they are tried again later)."""
        remaining, unsolved = ctypes.c_int64(), ctypes.c_int64()
        _check(self._L.az_solver_book_solve(self._h, int(max_positions), int(node_budget), ctypes.byref(remaining),
                                            ctypes.byref(unsolved)))
        return remaining.value, unsolved.value

    def book_finish(self):
        """Backs the scores up to the empty board; from here on solve() answers
        the book's positions without a search.  AzError while positions remain."""
        _check(self._L.az_solver_book_finish(self._h))

    def book_save(self, path):
        _check(self._L.az_solver_book_save(self._h, os.fsencode(path)))

    def book_load(self, path):
        """Replaces the solver's book by the file's; AzError naming the reason for
        a file that is no book, of another geometry, cut short or damaged."""
        _check(self._L.az_solver_book_load(self._h, os.fsencode(path)))

    def book_info(self):
        """-> (depth, state, level counts [depth + 1]); depth -1 and BOOK_NONE without a book."""
        depth, state = ctypes.c_int32(), ctypes.c_int32()
        counts = np.zeros(self.height * self.width, np.int64)
        _check(self._L.az_solver_book_info(self._h, ctypes.byref(depth), ctypes.byref(state), _ptr(counts)))
        return depth.value, state.value, counts[:depth.value + 1].copy()

    def book_level(self, stones, first=0, count=None, stride=1):
        """Entries first, first + stride, ... of the level with `stones` stones ->
        (boards [count, H, W] int8, +1 the side to move; scores int8,
        BOOK_NO_SCORE where there is none yet).  count=None: to the level's end."""
        if count is None:
            n = int(self.book_info()[2][stones])
            count = max(0, (n - int(first) + int(stride) - 1) // int(stride))
        boards = np.zeros((int(count), self.height, self.width), np.int8)
        scores = np.zeros(int(count), np.int8)
        _check(self._L.az_solver_book_level(self._h, int(stones), int(first), int(count), int(stride), _ptr(boards),
                                            _ptr(scores)))
        return boards, scores

    def build_book(self, depth, node_budget, chunk=1 << 16, path=None, seconds=None, report=None):
        """Builds the book of `depth`, or goes on with the one the solver holds
        (book_load) when it has that depth: book_solve in chunks of `chunk`
        positions, saved to `path` after each, then book_finish.  Stops after
        `seconds` (checked between chunks), or when a whole pass over the
        unsolved positions solves none of them.  report(done, remaining,
        unsolved) is called per chunk.  -> True when the book is finished."""
        t0 = time.perf_counter()
        have, state, counts = self.book_info()
        if have != depth or state == BOOK_NONE:
            counts = self.book_begin(depth)
            state = BOOK_BUILDING
        if state == BOOK_FINISHED:
            return True
        total = int(counts[depth])
        remaining, failed_in_a_row = None, 0
        while remaining != 0:
            if seconds is not None and time.perf_counter() - t0 >= seconds:
                return False
            before = remaining
            remaining, unsolved = self.book_solve(chunk, node_budget)
            if path is not None:
                self.book_save(path)
            if report is not None:
                report(total - remaining, remaining, unsolved)
            # every position left has gone over the budget since the last one was scored: give up
            failed_in_a_row = failed_in_a_row + unsolved if before == remaining else unsolved
            if remaining and failed_in_a_row >= remaining:
                return False
        self.book_finish()
        if path is not None:
            self.book_save(path)
        return True


class ChessEngine(_EngineBase):
    """libaz chess self-play engine (include/az_chess.h): `slots` concurrent
    chess games on one device, MCTS with the policy/value network on the
    (8, 8, 118) Board.full_state planes and the 1880-move action space -- or,
    with evaluator=EVAL_HOST, with any Python callable (set_host_evaluator).

    dirichlet_noise: ConfigMCTS.enable_dirichlet_noise (root noise, reference
    mcts.py:70-85) with dirichlet_alpha / dirichlet_ratio.  Self-play draws
    it on the device from each game's MT19937 stream, bit for bit numpy's
    legacy RandomState.dirichlet; tree_search takes the caller's draws."""

    ACTIONS = 1880
    MAX_MOVES = 256
    _ABI, _STATS = "az_chess_", "az_chess_stats"

    def __init__(self, mcts_iterations=800, slots=256, evaluator=EVAL_NETWORK, max_plies=512,
                 index_move_greedy=8, exploration_constant=1.5, filters=128, depth=4,
                 value_hidden=256, bn_epsilon=1e-3, arena_edges=0, conv_algo=CONV_F16X2,
                 device=0, lanes=0, cache_log2=0, dirichlet_noise=False, dirichlet_alpha=0.03,
                 dirichlet_ratio=0.25):
        L = load_library()
        self.slots, self.mcts_iterations = slots, mcts_iterations
        self.max_plies = max_plies if max_plies > 0 else 512
        cfg = ChessConfig(mcts_iterations=mcts_iterations, index_move_greedy=index_move_greedy,
                          exploration_constant=exploration_constant, slots=slots,
                          evaluator=evaluator, filters=filters, depth=depth,
                          value_hidden=value_hidden, max_plies=max_plies, bn_epsilon=bn_epsilon,
                          arena_edges=arena_edges, conv_algo=conv_algo, lanes=lanes, cache_log2=cache_log2,
                          dirichlet_noise=int(bool(dirichlet_noise)), dirichlet_alpha=float(dirichlet_alpha),
                          dirichlet_ratio=float(dirichlet_ratio))
        handle = ctypes.c_void_p()
        _check(L.az_chess_engine_create(int(device), ctypes.byref(cfg), ctypes.byref(handle)))
        self._attach(handle, L)

    def set_host_evaluator(self, fn):
        """EVAL_HOST engines: fn(x) with x [n, 8, 8, 118] float32 (Board.full_state
        of each leaf, every plane) returns (probs [n, 1880], values [n] or
        [n, 1]) -- the reference's self.model(x) call (mcts.py:130-137), here
        once per simulation and lane over every leaf that needs an evaluation
        (az_chess_engine_set_evaluator).  Outputs may be numpy arrays or torch
        / TF tensors; a wrong shape raises ValueError.  An exception inside fn
        ends the search and is re-raised by the call that ran it."""
        self._set_host_evaluator(fn, (8, 8, 118), self.ACTIONS, strict=True)

    def forward(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 8, 8, 118)
        probs = np.zeros((len(x), self.ACTIONS), np.float32)
        values = np.zeros(len(x), np.float32)
        _check(self._L.az_chess_forward(self._h, _ptr(x), len(x), _ptr(probs), _ptr(values)))
        return probs, values

    def selfplay_drain(self, max_games=None, chunk=64):
        """Games finished since the previous drain (az_chess_selfplay_drain):
        the arrays of selfplay_results with a leading axis over the drained
        games in finish order, plus `game_ids`.  Chunked: a chess game's dense
        rows are ~1.3 MB (max_plies x 256 policy entries)."""
        from custom_alphazero.chess.kernels import POS_DTYPE
        P, M = self.max_plies, self.MAX_MOVES
        return self._drain(max_games, chunk, lambda G: dict(
            game_ids=np.zeros(G, np.int64), lengths=np.zeros(G, np.int32),
            results=np.zeros(G, np.int32), terminations=np.zeros(G, np.int32),
            expansions=np.zeros(G, np.int32), positions=np.zeros((G, P), POS_DTYPE),
            moves=np.zeros((G, P), np.uint16), policy_n=np.zeros((G, P), np.int32),
            policy_actions=np.zeros((G, P, M), np.int16), policy_probs=np.zeros((G, P, M), np.float64)))

    def selfplay_results(self, with_samples=True):
        from custom_alphazero.chess.kernels import POS_DTYPE
        G, P, M = self._n_games, self.max_plies, self.MAX_MOVES
        out = {k: np.zeros(G, np.int32) for k in ("lengths", "results", "terminations", "expansions")}
        if with_samples:
            out["positions"] = np.zeros((G, P), POS_DTYPE)
            out["moves"] = np.zeros((G, P), np.uint16)
            out["policy_n"] = np.zeros((G, P), np.int32)
            out["policy_actions"] = np.zeros((G, P, M), np.int16)
            out["policy_probs"] = np.zeros((G, P, M), np.float64)
        g = out.get
        _check(self._L.az_chess_selfplay_results(
            self._h, _ptr(g("lengths")), _ptr(g("results")), _ptr(g("terminations")),
            _ptr(g("expansions")), _ptr(g("positions")), _ptr(g("moves")), _ptr(g("policy_n")),
            _ptr(g("policy_actions")), _ptr(g("policy_probs"))))
        return out

    def timer(self, on):
        _check(self._L.az_chess_timer_enable(self._h, int(bool(on))))

    # ------------------------------------------------------------- tree API
    def tree_reset(self, slots, roots):
        from custom_alphazero.chess.kernels import POS_DTYPE
        slots = np.ascontiguousarray(slots, np.int32)
        roots = np.ascontiguousarray(roots, POS_DTYPE).reshape(len(slots))
        _check(self._L.az_chess_tree_reset(self._h, len(slots), _ptr(slots), _ptr(roots)))

    def tree_release(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        _check(self._L.az_chess_tree_release(self._h, len(slots), _ptr(slots)))

    def tree_search(self, n_sims, noise=None):
        """noise (engines made with dirichlet_noise): [slots, rows, 256] float64,
        row r of slot s the np.random.dirichlet vector its r-th root selection
        mixes in, entry i for root edge i (az_chess_tree_search_noise)."""
        if noise is None:
            self._search_call(self._L.az_chess_tree_search(self._h, int(n_sims)))
            return
        noise = np.ascontiguousarray(noise, np.float64)
        if noise.ndim != 3 or noise.shape[0] != self.slots or noise.shape[2] != self.MAX_MOVES:
            raise ValueError(f"noise must be [slots={self.slots}, rows, {self.MAX_MOVES}], got {noise.shape}")
        self._search_call(self._L.az_chess_tree_search_noise(self._h, int(n_sims), _ptr(noise),
                                                             int(noise.shape[1])))

    def tree_play(self, uniforms=None, greedy=False, deterministic=False):
        """-> moves [S] (move codes, -1 idle), status [S] (AZ_CHESS_* of the new
        root), policy_n [S], policy_actions [S, 256], policy_probs [S, 256]."""
        S, M = self.slots, self.MAX_MOVES
        u = None if deterministic else np.ascontiguousarray(uniforms, np.float64).reshape(S)
        out = dict(moves=np.zeros(S, np.int32), status=np.zeros(S, np.int32),
                   policy_n=np.zeros(S, np.int32), policy_actions=np.zeros((S, M), np.int16),
                   policy_probs=np.zeros((S, M), np.float64))
        _check(self._L.az_chess_tree_play(self._h, _ptr(u), int(bool(greedy)), int(bool(deterministic)),
                                          *(_ptr(out[k]) for k in ("moves", "status", "policy_n",
                                                                   "policy_actions", "policy_probs"))))
        return out

    def tree_export(self, slot):
        info = np.zeros(5, np.int64)
        rv = np.zeros(1, np.float32)
        _check(self._L.az_chess_tree_info(self._h, int(slot), _ptr(info), _ptr(rv)))
        n = int(info[0])
        out = dict(prior=np.zeros(n, np.float64), w=np.zeros(n, np.float64), n=np.zeros(n, np.int32),
                   child=np.zeros(n, np.int32), child_n=np.zeros(n, np.int32),
                   moves=np.zeros(n, np.int32), child_value=np.zeros(n, np.float32))
        _check(self._L.az_chess_tree_export(self._h, int(slot), *(_ptr(out[k]) for k in (
            "prior", "w", "n", "child", "child_n", "moves", "child_value"))))
        out.update(arena_top=n, root_first=int(info[1]), root_n=int(info[2]), ply=int(info[3]),
                   active=bool(info[4]), root_value=float(rv[0]))
        return out
