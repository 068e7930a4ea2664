// az_tree.h -- device-resident MCTS forest: one tree per game slot.
#pragma once
#include "az_cache.h"
#include "az_device.h"

namespace az {

// One tree edge (reference UCTEdge, mcts/mcts.py:22-33) = 32 bytes.  A node
// is implicit: the contiguous run of edges its expansion allocated.  Child
// boards are not stored; select() replays the path's moves from the root
// board (board rules are cheap, HBM bytes are not).
struct Edge {
  double W;           // total_action_value (float64, += in path order)
  double prior;       // float32 prior widened exactly, or the float64 1/n uniform
  int32_t N;          // visit_count
  int32_t child;      // first edge of the child's expansion, kNoChild if leaf
  int16_t child_n;    // child's edge count (0 = unexpanded or terminal)
  int16_t action;     // index into all_possible_moves
  float child_value;  // child's evaluated_value (tree export only)
};
static_assert(sizeof(Edge) == 32, "Edge must stay 32 bytes");

// Counters/stat words (unsigned long long, device), each on a 128-byte line
// of its own (kStatStride words apart): every wave of every lane adds to them
// (wave-aggregated atomics), and counters sharing a line serialised in its
// L2 channel (round 6).  An index below is the word offset of its counter.
constexpr int kStatStride = 16;
enum : int {
  kStatExpansions = 0 * kStatStride,   // evaluate_and_expand calls
  kStatTerminal = 1 * kStatStride,     // terminal leaf visits
  kStatGamesDone = 2 * kStatStride,
  kStatErrors = 3 * kStatStride,       // bit flags below
  kStatSims = 4 * kStatStride,         // per-slot simulations
  kStatPlies = 5 * kStatStride,
  kStatNextGame = 6 * kStatStride,     // next game id to hand to a free slot
  kStatCacheHits = 7 * kStatStride,    // expansions served by the transposition cache
  kStatNNEvals = 8 * kStatStride,      // boards the evaluator actually computed
  kStatCacheInserts = 9 * kStatStride,
  kStatPathEdges = 10 * kStatStride,   // edges on the selected paths (sum of select depths)
  kStatMaxRetained = 11 * kStatStride, // compaction: most edges kept (atomicMax)
  kStatPoolHigh = 12 * kStatStride,    // pooled arenas: most edges a lane's half held at a move's end (atomicMax)
  kStatCount = 13 * kStatStride        // words (kStatCacheInserts counts since engine creation; CacheDev::ctl since a clear)
};
// a lane's per-simulation queue counters (eval, miss, nn; the block's fourth
// counter went with the per-simulation dedup), one block per simulation
// parity, each counter on a 128-byte line of its own
constexpr int kCountStride = 32;
constexpr int kCountWords = 2 * 4 * kCountStride;
enum : unsigned long long {
  kErrArena = 1, kErrPow = 2, kErrPath = 4, kErrIllegal = 8, kErrNoRoot = 16,
  kErrActRange = 32,  // a conv16 activation beyond the split16 range (|x| > 32752)
  kErrNoise = 64,     // the tree API's host-drawn root noise ran out of rows
  kErrDraw = 128      // the wave-parallel Dirichlet draw hit its round cap (az_dirichlet_wave.h)
};

// All device state of a forest (struct of arrays over slots).
//
// Arenas.  halves == 1 (the tree API, uncompacted self-play): slot s owns the
// static run edges[s * arena_cap, (s + 1) * arena_cap); edge indices are
// relative to it.  halves == 2 (compacted self-play): every lane owns a POOL
// of two halves of pool_cap edges; a move's search allocates from the
// current half (`edges`, bump counter `pool_top`) in chunks of kPoolChunkA * A
// edges per slot, and compaction copies each slot's kept subtree into the
// other half (`dst_edges`, `dst_top`), reserving the slot's live edge count
// there in one bump.  After a lane's compaction the current half is empty:
// its counter resets and the halves swap (host side, the next launches'
// views).  Edge indices are pool-half indices.  The pool is shared by the
// lane's slots, so one game whose kept subtree grows large (a peaked
// network) borrows what other slots do not use; overflow raises kErrArena.
constexpr int kPoolChunkA = 16;
struct TreeDev {
  Edge* edges;                 // halves == 1: [slots][arena_cap]; 2: the lane's current pool half
  int32_t* arena_end;          // [slots] pool: end of the slot's current chunk
  int32_t* slot_live;          // [slots] pool: edges of the slot's tree in the current half
  unsigned long long* pool_top;  // pool: the current half's bump counter
  Edge* dst_edges;             // pool: the other half (compaction target) ...
  unsigned long long* dst_top;   // ... and its counter
  int32_t pool_cap;            // pool: edges per half
  Board* root_board;           // [slots]
  int32_t* root_first;         // [slots]
  int32_t* root_n;             // [slots]
  float* root_value;           // [slots]
  int32_t* arena_top;          // [slots] next free edge (static: of the slot's run; pool: of the half)
  int32_t* ply;                // [slots] (Board.fullmove_number)
  int64_t* game_id;            // [slots], -1 = idle
  int32_t* path;               // [slots][max_depth]
  int32_t* path_len;           // [slots]
  int32_t* slot_expansions;    // [slots], this game's expansions so far
  uint32_t* mt;                // [625][mt_stride], word-major MT19937 state (+ index)
  int32_t mt_stride;           // slots of the whole engine (a lane view offsets mt)
  // the slot's leaf of this simulation, read by the expand launch (one
  // thread per slot): (leaf_epoch << 32) | src, src >= 0 a cache entry, < 0
  // -(evaluator row + 1); another simulation's tag: no leaf (idle, terminal)
  uint64_t* leaf_src;          // [slots]
  Board* leaf_board;           // [slots]
  uint32_t leaf_epoch;         // this simulation's tag, unique over the engine's lanes
  Board* eval_board;           // [slots] evaluator rows with the cache off (every leaf)
  int32_t* eval_count;         // [1]
  int32_t* miss_count;         // [1]
  Board* nn_board;             // [slots] evaluator rows with the cache on (the misses)
  int32_t* nn_count;           // [1]
  // eval/miss/nn counts (and a spare word) are one block of 4; two blocks
  // alternate by simulation (epoch parity): the select kernel zeroes the
  // other block, the next simulation's, so no memset launch sits between
  int32_t* next_counts;        // [4 * kCountStride] the block the next simulation uses
  uint32_t epoch;              // the lane's simulation counter (its parity picks the block)
  unsigned long long* stats;   // [kStatCount]
  const double* powtab;        // [pow_len]: libm pow(n, 0.5), host-built
  // per-move outputs (MCTS API play())
  int32_t* last_move;          // [slots] action played (-1 none)
  int32_t* last_status;        // [slots] 0 ongoing / 1 win / 2 draw
  double* last_policy;         // [slots][A]
  // tree API root noise drawn by the host (az_tree_search_noise): slot s's
  // r-th root selection of the search mixes noise_in[(s * noise_rows + r) * A + i]
  // into edge i's prior; null: self-play draws on the device from the slot's MT19937
  const double* noise_in;
  int32_t* noise_cur;          // [slots] rows consumed
  int32_t noise_rows;
};

// The transposition cache (az_cache.h) keyed by boards; a payload is [A+1]
// floats: probs then value.
using CacheDev = Cache<Board>;

// Self-play sample sink, indexed by game id - first_game.
struct SampleDev {
  int64_t first_game = 0, n_games = 0;
  uint32_t base_seed = 0;
  Board* boards = nullptr;     // [n_games][max_plies]: root board before each move
  double* policy = nullptr;    // [n_games][max_plies][A]
  int16_t* moves = nullptr;    // [n_games][max_plies]
  int32_t* length = nullptr;   // [n_games]
  int32_t* result = nullptr;   // [n_games]: get_result(keep_same_player=True)
  int32_t* expansions = nullptr;  // [n_games]
  int64_t* done_ids = nullptr;    // [n_games] game ids in the order they finished
  unsigned long long* done_count = nullptr;  // [1]
};

// Finished games [from, from + n) of smp.done_ids packed for one D2H copy
// (az_selfplay_drain): ids, lengths, results, expansions, then per game
// HW plies of int8 cells (row-major, canonical), f64 policies [HW][A] and
// int16 moves.  Layout of one record: drain_record_bytes().
size_t drain_record_bytes(const GameCfg& g);
void launch_drain_pack(const GameCfg& g, const SampleDev& smp, int64_t from, int n, uint8_t* out,
                       hipStream_t s);

// the base edge indices of slot s are relative to
AZ_HD Edge* slot_edges(const GameCfg& g, const TreeDev& t, int s) {
  return g.halves > 1 ? t.edges : t.edges + (size_t)s * g.arena_cap;
}

void launch_select(const GameCfg& g, const TreeDev& t, const CacheDev& c, hipStream_t s);
// self-play tree reuse (halves == 2): the new root's subtree into the other
// pool half; then the current half's counter is reset (its high-water mark to
// kStatPoolHigh) -- the host swaps the halves for the next move
void launch_compact(const GameCfg& g, const TreeDev& t, hipStream_t s);
// end of a lane's move: the last of n_lanes lanes to arrive stores the
// games-finished count into *snap (pinned host memory) and resets *arrive
void launch_move_end(int32_t* arrive, int n_lanes, const unsigned long long* done_count,
                     unsigned long long* snap, hipStream_t s);
// the synthetic evaluator on the queued boards (cache on: the misses' rows,
// one per missing slot -- two slots that miss on one board each take a row)
void launch_synth_eval(const GameCfg& g, const Board* boards, const int32_t* count, float* probs,
                       float* values, hipStream_t s);
void launch_expand(const GameCfg& g, const TreeDev& t, const CacheDev& c, const float* probs,
                   const float* values, hipStream_t s);
// uniforms: device [slots] draws for play (MCTS API), or null -> per-slot MT19937;
// greedy_mode -1 = by ply (self-play), 0/1 = caller's flag
void launch_play(const GameCfg& g, const TreeDev& t, const SampleDev& smp, const double* uniforms,
                 int greedy_mode, int deterministic, int refill, hipStream_t s);
void launch_slot_init(const GameCfg& g, const TreeDev& t, const SampleDev& smp, int64_t n_first,
                      hipStream_t s);
void launch_slot_release(const TreeDev& t, const int32_t* slots, int n, hipStream_t s);
void launch_slot_set_root(const GameCfg& g, const TreeDev& t, const int32_t* slots,
                          const Board* boards, int n, hipStream_t s);

}  // namespace az
