/*
 * az_chess.h -- C ABI of libaz's chess board kernels (gfx950).
 *
 * Replaces the reference's chess board seam (custom_alphazero/chess/), which
 * is a subclass of python-chess 1.9.4 (poetry.lock:227-228): the hot path's
 * "board-tensor encode + legal-move mask" for chess.
 * Each call below is batched over n positions and runs on the GPU; the Python
 * drop-in (custom_alphazero/chess/board.py) binds them with ctypes.
 *
 * Conventions as in az.h: 0 or a negative AZ_E* code, az_last_error() holds
 * the message; host buffers owned by the caller; synchronous.  `device` is a
 * HIP device ordinal; each call uses a per-device stream and scratch of the
 * library's own.
 *
 * Squares are python-chess's (A1 = 0 .. H8 = 63).  A move is a uint16:
 * from | to << 6 | promotion << 12, promotion = python-chess piece type
 * (0 none, 2 knight, 3 bishop, 4 rook, 5 queen).
 */
#ifndef AZ_CHESS_H_
#define AZ_CHESS_H_

#include <stdint.h>

#include "az.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_CHESS_MAX_MOVES 256  /* > 218, the most legal moves of any position */
#define AZ_CHESS_ACTIONS 1880   /* len(get_all_possible_moves()) (chess/utils.py:11-32) */
#define AZ_CHESS_HISTORY 8      /* Board(history_size=8) (chess/board.py:17) */
#define AZ_CHESS_PLANES 118     /* 8 x (13 one-hot + repetition) + 6 (chess/board.py:55-73) */

/* A python-chess Board's position state (80 bytes).  The repetition flag is
 * the value Board.state's last plane carries (is_repetition()). */
typedef struct az_chess_pos {
    uint64_t pieces[6];        /* pawns, knights, bishops, rooks, queens, kings */
    uint64_t occupied_co[2];   /* [0] BLACK, [1] WHITE */
    uint64_t castling_rights;  /* rook squares (python-chess Board.castling_rights) */
    int16_t ep_square;         /* -1 = None */
    uint8_t turn;              /* 1 = WHITE */
    uint8_t repetition;
    uint16_t halfmove_clock;
    uint16_t fullmove_number;
} az_chess_pos;

/* Termination codes of python-chess Board.outcome() (checked in this order) */
#define AZ_CHESS_ONGOING 0
#define AZ_CHESS_CHECKMATE 1
#define AZ_CHESS_INSUFFICIENT 2
#define AZ_CHESS_STALEMATE 3
#define AZ_CHESS_SEVENTYFIVE 4

/* get_all_possible_moves() (chess/utils.py:11-32): the action list, sorted by
 * Move.__lt__ (chess/move.py:33-37).  cap >= AZ_CHESS_ACTIONS; returns the
 * count (host-side table, no device work). */
int az_chess_all_moves(uint16_t* out, int cap);

/* Board.moves (chess/board.py:46-48: python-chess legal_moves, generation
 * order), Board.legal_moves_mask(all_possible_moves) (:111-112) and
 * is_game_over()/outcome() for n positions: moves [n][AZ_CHESS_MAX_MOVES],
 * counts [n], mask [n][AZ_CHESS_ACTIONS] u8, outcome [n].  Any output except
 * counts may be NULL. */
int az_chess_legal(int device, const az_chess_pos* pos, int n, uint16_t* moves, int32_t* counts,
                   uint8_t* mask, int32_t* outcome);

/* Board.full_state (chess/board.py:55-73) for n boards: hist [n][8] oldest
 * first (the state_history deque), valid [n][8] (0 = a zero-filled entry),
 * the board itself is hist[i][7] (castling planes, fullmove, halfmove) ->
 * state [n][8][8][118] f32, rows = ranks 8..1 as Board.array (every value is
 * a small integer: exact in f32; the reference's float64 casts exactly). */
int az_chess_encode(int device, const az_chess_pos* hist, const uint8_t* valid, int n,
                    float* state);

/* Board.play(move, keep_same_player=...) (chess/board.py:162-173) in place on
 * n positions: push, then (keep_same_player) mirror + turn = WHITE. */
int az_chess_play(int device, az_chess_pos* pos, const uint16_t* moves, int n,
                  int keep_same_player);

/* perft(depth) node count (legal move generation + push, breadth first on the
 * device): the size-independent check of the move generator. */
int az_chess_perft(int device, const az_chess_pos* pos, int depth, uint64_t* nodes);


/* ------------------------------------------------------------ self-play
 * Chess self-play (BASELINE configs[4]): the batched
 * replacement of self_play.play_game / MCTS on chess boards
 * (self_play.py:37-82, mcts/mcts.py:88-222, chess/board.py).  Same tree
 * arithmetic as the Connect-N engine (f64 PUCT, libm pow, first-max argmax,
 * float32 pairwise prior normalisation with the reference's positional
 * prior/move zip, np.random.choice on MT19937); subtrees are reused across
 * moves (current_root = edge.child) and compacted into the other half of the
 * slot's edge arena.  The reference's chess path cannot finish a game under
 * MCTS (get_result() takes no keep_same_player, chess/board.py:178 vs
 * mcts.py:179); here a terminal board scores as get_result does in the
 * canonical form: 1 for checkmate (a win for the side that just moved), 0 for
 * every draw. */
typedef struct az_chess_engine az_chess_engine;

typedef struct az_chess_config {
    int32_t mcts_iterations;      /* sims per move (ConfigSelfPlay.mcts_iterations) */
    int32_t index_move_greedy;    /* greedy once fullmove_number >= this (self_play.py:62) */
    double exploration_constant;  /* ConfigMCTS.exploration_constant */
    int32_t slots;                /* concurrent games on this device */
    int32_t evaluator;            /* AZ_EVAL_NETWORK, AZ_EVAL_SYNTHETIC or AZ_EVAL_HOST (a host
                                     callback: az_chess_engine_set_evaluator) */
    int32_t filters, depth, value_hidden;  /* ConfigModel (filters must be 128) */
    int32_t max_plies;            /* addition: games stop (as draws) after this many plies;
                                     the reference has no cap (0 = 512) */
    double bn_epsilon;
    int64_t arena_edges;          /* edges per arena half per slot (0 = 96 * mcts_iterations) */
    int32_t conv_algo;            /* AZ_CONV_F16X2 (default) / AZ_CONV_DIRECT: the tower and the
                                     stem over the 118 planes zero-padded to 128; AZ_CONV_F16 (3):
                                     the one-launch tower's one-term fp16 arithmetic (az.h; opt-in,
                                     1 <= depth <= 16) */
    int32_t lanes;                /* slot groups searched on separate HIP streams (0 = auto: 2 from
                                     128 slots, else 1); results do not depend on it */
    int32_t cache_log2;           /* ABI 10: transposition cache entries = 2^cache_log2, the
                                     reference's plays_inferences on chess boards (mcts.py:122-143):
                                     key = the leaf position + its history form, ~1.1 KB per entry
                                     (the masked priors, up to 256, and the value); identical leaves
                                     of one simulation share a network row.  0 = off, else 4..28;
                                     results are identical either way */
    int32_t dirichlet_noise;      /* ConfigMCTS.enable_dirichlet_noise (mcts.py:70-85, 113-116); the
                                     three fields took the place of reserved[5] (all zero = off, as
                                     every earlier caller passed), so the ABI version did not move */
    double dirichlet_alpha;       /* ConfigMCTS.dirichlet_noise_value (0.03); 0 < alpha <= 1 */
    double dirichlet_ratio;       /* ConfigMCTS.dirichlet_noise_ratio (0.25) */
} az_chess_config;
/* Dirichlet root noise (dirichlet_noise = 1): every selection at the current
 * root of a tree that has edges draws np.random.dirichlet(alpha * ones(k)), k
 * the root's edge count, and takes np.argmax (NaN first) of the UCB over
 * (1 - ratio) * priors + ratio * noise, computed as numpy does (the first
 * product in the priors' dtype: float32, or float64 after
 * normalize_probabilities' uniform branch).  The reference's chess MCTS cannot
 * run a search (chess/board.py:178's get_result signature vs mcts.py:179), but
 * this behaviour is its game-agnostic code's.  Self-play draws on the device
 * from the game's stream, MT19937(base_seed + game_id), bit for bit numpy's
 * legacy RandomState.dirichlet: all of a move's root-noise vectors in
 * simulation order, then MCTS.play's one random_sample.  The tree API takes
 * the caller's draws (az_chess_tree_search_noise).  The Python MCTS class on a
 * chess Board and the chess arena still refuse the flag
 * (config.check_mcts_config("chess")).
 * Evaluators: the network (AZ_EVAL_NETWORK), the oracle's synthetic function
 * (AZ_EVAL_SYNTHETIC) or a host callback (AZ_EVAL_HOST,
 * az_chess_engine_set_evaluator): self-play, the tree API and, in Python,
 * MCTS on a chess Board and the two-model arena run with any of them. */

/* Termination of a finished self-play game: AZ_CHESS_* above, or this */
#define AZ_CHESS_MAX_PLIES 5

int az_chess_engine_create(int device, const az_chess_config* cfg, az_chess_engine** out);
int az_chess_engine_destroy(az_chess_engine* eng);
/* PolicyValueModel weights for input_dim (8, 8, 118), action_space 1880
 * (model/tensorflow/model.py:152-188; names of custom_alphazero/model/weights.py);
 * AZ_EVAL_NETWORK engines only */
int az_chess_engine_set_weights(az_chess_engine* eng, const az_tensor* tensors, int n);
/* AZ_EVAL_HOST (added after ABI 10 without a version bump: the change only
 * adds): the evaluator of an engine created with AZ_EVAL_HOST, az.h's
 * az_eval_fn -- the reference's duck-typed self.model(x) seam
 * (mcts/mcts.py:130-137) for chess boards.  AZ_E_STATE on an engine created
 * with another evaluator.  The search calls it once per simulation and lane
 * with the leaves that need an evaluation -- after the transposition cache
 * and, where the cache is on, after the per-simulation sharing of identical
 * leaves -- as x [n][8][8][118] f32, contiguous: exactly Board.full_state of
 * each leaf, all 118 planes (the history planes 0-83 the self-play tower
 * skips included), in the history form of the tree API below: [0 x 7, start]
 * for a root set by reset or a game's first board, [0 x 6, start, board]
 * otherwise.  It writes the model's raw outputs probs [n][1880] (before the
 * legal-move mask and renormalisation, mcts.py:147-150) and values [n], and
 * returns 0; n <= 0 makes no call.  Host buffers, valid during the call.  A
 * nonzero return fails the search with AZ_E_CALLBACK, and the simulation it
 * interrupted leaves the trees incomplete: az_chess_selfplay_step,
 * az_chess_selfplay_run's steps, az_chess_tree_search and az_chess_tree_play
 * then fail with AZ_E_STATE until az_chess_selfplay_begin or
 * az_chess_tree_reset.  Searching before a callback is set is AZ_E_STATE.
 * The outputs must be a deterministic function of x (the cache relies on it,
 * as the reference's plays_inferences dict does); results are identical with
 * the cache on or off.  They may be any float32, non-finite included; nothing
 * is rejected, as in the reference: the search follows the reference's
 * arithmetic and np.argmax's order for the best edge, the first NaN first
 * (az.h, az_eval_fn).  az_chess_forward and az_chess_engine_set_weights on
 * such an engine answer AZ_E_STATE.  Every simulation waits for its callback,
 * so az_chess_selfplay_step with st = NULL is effectively synchronous here. */
int az_chess_engine_set_evaluator(az_chess_engine* eng, az_eval_fn fn, void* user);
/* PolicyValueModel.__call__ on chess states: x [n][8][8][118] f32 (Board.full_state)
 * -> probs [n][1880] f32, values [n] f32 */
int az_chess_forward(az_chess_engine* eng, const float* x, int n, float* probs, float* values);
/* Games first_game .. first_game + n_games - 1 from the start position, game g
 * seeded with MT19937(base_seed + g); slots refilled as games end. */
int az_chess_selfplay_begin(az_chess_engine* eng, int64_t first_game, int64_t n_games,
                            uint32_t base_seed);
/* With st = NULL the moves are only enqueued (ABI 10): the call returns at once
 * and device errors surface at the next synchronizing call; with st it waits
 * for them and fills the stats.  Only this call and az_chess_selfplay_drain
 * run beside the queued moves: every other call on the engine, az_chess_forward
 * included, first waits for them. */
int az_chess_selfplay_step(az_chess_engine* eng, int n_moves, az_stats* st);
int az_chess_selfplay_run(az_chess_engine* eng, int64_t first_game, int64_t n_games,
                          uint32_t base_seed, az_stats* st);
/* Per game g (P = max_plies): lengths[g] plies; results[g] (1 checkmate, 0
 * draw or cap); terminations[g] (AZ_CHESS_*); expansions[g]; positions
 * [g][P] (canonical root before each move, MCTS.play's parent board); moves
 * [g][P]; the MCTS.play policy sparsely: policy_n [g][P] root edges,
 * policy_actions [g][P][AZ_CHESS_MAX_MOVES] action indices (edge order),
 * policy_probs [g][P][AZ_CHESS_MAX_MOVES] f64.  Any pointer may be NULL. */
int az_chess_selfplay_results(az_chess_engine* eng, int32_t* lengths, int32_t* results,
                              int32_t* terminations, int32_t* expansions, az_chess_pos* positions,
                              uint16_t* moves, int32_t* policy_n, int16_t* policy_actions,
                              double* policy_probs);
/* The games that finished since the previous drain (ABI 10; at most
 * max_games, in the order they finished) while self-play runs on: the
 * reference's result return (self_play.py:112-118), one step at a time, as
 * az_selfplay_drain does for Connect-N.  *n_out = games copied; per game i:
 * game_ids[i], lengths/results/terminations/expansions[i], and its rows as
 * az_chess_selfplay_results: positions [i][P], moves [i][P], policy_n
 * [i][P], policy_actions [i][P][AZ_CHESS_MAX_MOVES], policy_probs
 * [i][P][AZ_CHESS_MAX_MOVES] (P = max_plies; rows past the game's length are
 * zero).  "Finished" = by the end of the newest move whose games-finished
 * snapshot is complete: the drain never waits for a running move.  Any
 * output but n_out may be NULL. */
int az_chess_selfplay_drain(az_chess_engine* eng, int64_t max_games, int64_t* n_out, int64_t* game_ids,
                            int32_t* lengths, int32_t* results, int32_t* terminations, int32_t* expansions,
                            az_chess_pos* positions, uint16_t* moves, int32_t* policy_n,
                            int16_t* policy_actions, double* policy_probs);
int az_chess_stats(az_chess_engine* eng, az_stats* st);

/* MCTS tree API on chess boards (mcts/mcts.py:86-222 with a chess Board):
 * replaces the per-object UCTNode/UCTEdge tree of one MCTS instance with a
 * slot of the engine.  A reset root evaluates with the history of a board
 * made by deepcopy (python-chess copy() re-runs the subclass __init__:
 * [0 x 7, start-position state], whatever the position); every board after
 * play() holds [0 x 6, start state, board].  Positions are canonical
 * (Board.play(keep_same_player=True) form). */
int az_chess_tree_reset(az_chess_engine* eng, int n, const int32_t* slots, const az_chess_pos* roots);
/* Idle the given slots (search and play skip them) until the next reset. */
int az_chess_tree_release(az_chess_engine* eng, int n, const int32_t* slots);
/* MCTS.search(n_sims) on every active slot.  AZ_E_INVALID on an engine
 * created with dirichlet_noise (its searches need the caller's draws). */
int az_chess_tree_search(az_chess_engine* eng, int n_sims);
/* The same on an engine created with dirichlet_noise = 1 (AZ_E_INVALID on any
 * other): noise [slots][rows][AZ_CHESS_MAX_MOVES] f64, row r of slot s the
 * np.random.dirichlet vector that slot's r-th root selection of this search
 * mixes in; entry i of a row belongs to root edge i (python-chess move order),
 * entries past the root's edge count are ignored.  One row is consumed per
 * simulation whose root has edges (the first simulation after a reset expands
 * the root and consumes none); a slot that runs out of rows fails the search
 * with AZ_E_DEVICE (root-noise-rows-exhausted).  Added without a version bump:
 * the change only adds. */
int az_chess_tree_search_noise(az_chess_engine* eng, int n_sims, const double* noise, int rows);
/* MCTS.play(greedy, deterministic) on every active slot: uniforms [slots] are
 * the np.random.random_sample draws np.random.choice consumes (ignored when
 * deterministic).  Per slot: moves (move code, -1 idle), status (AZ_CHESS_*
 * outcome of the new root), the policy sparsely as in
 * az_chess_selfplay_results (policy_n, policy_actions [slots][256], policy_probs
 * [slots][256]).  The chosen child's subtree becomes the tree (mcts.py:212);
 * siblings are dropped.  Any output pointer may be NULL. */
int az_chess_tree_play(az_chess_engine* eng, const double* uniforms, int greedy, int deterministic,
                       int32_t* moves, int32_t* status, int32_t* policy_n, int16_t* policy_actions,
                       double* policy_probs);
/* Tree snapshot of one slot: info = {edges, root_first, root_n, ply,
 * active}, root_value = the root's evaluated_value (0 before expansion);
 * then the edge arrays (length info[0]); moves are move codes, child the
 * first edge of the child's expansion or -1. */
int az_chess_tree_info(az_chess_engine* eng, int slot, int64_t* info, float* root_value);
int az_chess_tree_export(az_chess_engine* eng, int slot, double* prior, double* w, int32_t* n,
                         int32_t* child, int32_t* child_n, int32_t* moves, float* child_value);

/* HIP-event timing of the residual-tower conv launches (bench.py roofline) */
int az_chess_timer_enable(az_chess_engine* eng, int on);

/* The training step of the chess network (8x8x118 planes, 1880 actions): an az_trainer
 * (include/az.h) that every az_trainer_* call accepts.  Reads cfg->filters, depth,
 * value_hidden, bn_epsilon; the rest of cfg is ignored.  filters must be 128, depth 1..16,
 * value_hidden 1..1024, bn_epsilon > 0, max_batch >= 1 and max_batch*64*128 < 2^31.
 * az_trainer_step then takes x [n][8][8][118] (Board.full_state), pi [n][1880], z [n]; tensor
 * names and layouts are weights.weight_spec(8, 8, 1880, 128, depth, value_hidden, 118)'s, the
 * spec az_chess_engine_set_weights loads.  Added without a version bump: the change only adds. */
int az_chess_trainer_create(int device, const az_chess_config* cfg, int max_batch, az_trainer** out);

/* ------------------------------------------------------------ replay window
 * The chess replay window on the device: the samples the training loop draws
 * its batches from (the reference's local_*_queue arrays, train.py:16-40), held
 * as self-play hands them over -- each sample the board's 8 history positions
 * and their valid flags (az_chess_encode's form), the MCTS.play policy sparsely
 * (az_chess_selfplay_results' policy_n / policy_actions / policy_probs row) and
 * the value: about 3.2 KB against 45 KB in dense form.  Storage is a structure
 * of arrays: hist [cap][8] az_chess_pos, valid [cap][8] u8, policy_n [cap] i32,
 * policy_actions [cap][256] i16, policy_probs [cap][256] f64, z [cap] f32.  One
 * kernel gathers a batch by index, encodes the planes and scatters the policy
 * to dense rows.  Every call is synchronous.  One thread drives a replay and the
 * trainer that steps from it: no call on either runs beside another.  Added
 * without a version bump: the change only adds. */
typedef struct az_chess_replay az_chess_replay;

/* capacity >= 1 samples on `device`. */
int az_chess_replay_create(int device, int64_t capacity, az_chess_replay** out);
int az_chess_replay_destroy(az_chess_replay* rp);
/* Appends n samples, in order, from host buffers: hist [n][8] oldest first and
 * valid [n][8] as az_chess_encode takes them, policy_n [n], policy_actions
 * [n][AZ_CHESS_MAX_MOVES], policy_probs [n][AZ_CHESS_MAX_MOVES] f64 (entries
 * past policy_n are ignored), z [n].  The window is a ring that keeps the newest
 * `capacity` samples; a push of n > capacity keeps its last `capacity`.
 * Checked on the host before anything is copied: 0 <= policy_n <= 256, every
 * used action in 0..1879, and no action twice in a row of the policy (the
 * host's dense assignment is last-wins, a parallel scatter is not).  A violation
 * is AZ_E_INVALID and leaves the window as it was. */
int az_chess_replay_push(az_chess_replay* rp, const az_chess_pos* hist, const uint8_t* valid,
                         const int32_t* policy_n, const int16_t* policy_actions, const double* policy_probs,
                         const float* z, int64_t n);
/* Samples held, and the capacity; either pointer may be NULL. */
int az_chess_replay_size(az_chess_replay* rp, int64_t* size, int64_t* capacity);
/* Empties the window: the next push starts at index 0. */
int az_chess_replay_clear(az_chess_replay* rp);
/* The samples idx [n] in dense form, to host buffers: x [n][8][8][118]
 * (Board.full_state, bitwise az_chess_encode's), pi [n][1880] f32 (zeros, then
 * pi[action] = (float)prob: round to nearest, numpy's astype(float32)), z [n].
 * Any output may be NULL.  Index 0 is the oldest sample held and size - 1 the
 * newest: the row order of the reference's window np.vstack(...)[-size:], so the
 * same np.random.choice indices name the same samples.  Indices may repeat and
 * come in any order.  AZ_E_INVALID for an index outside 0..size-1, AZ_E_STATE on
 * an empty window. */
int az_chess_replay_gather(az_chess_replay* rp, const int64_t* idx, int n, float* x, float* pi, float* z);
/* az_trainer_step (include/az.h) on the samples idx [n] of the window, for a
 * trainer made by az_chess_trainer_create: the batch is gathered on the device
 * straight into the step's input buffers, on the trainer's stream, and no dense
 * state crosses the host.  The step itself, its preconditions and its results
 * are az_trainer_step's on az_chess_replay_gather's arrays, bit for bit.
 * AZ_E_INVALID for a Connect-N trainer, a replay on another device than the
 * trainer, n outside 1..max_batch or an index outside the window; AZ_E_STATE
 * before az_trainer_set_weights or on an empty window.  Waits for the step. */
int az_trainer_step_replay(az_trainer* tr, az_chess_replay* rp, const int64_t* idx, int n, double lr,
                           double momentum, double l2, double bn_momentum, float* losses);

#ifdef __cplusplus
}
#endif
#endif
