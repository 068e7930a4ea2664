// az_engine.hip -- host side of libaz: the Connect-N C ABI (include/az.h),
// device buffers, and the lockstep self-play driver.
#include <math.h>
#include <string.h>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/az.h"
#include "az_session.h"
#include "az_mt.h"
#include "az_nn.h"
#include "az_tree.h"

namespace {

constexpr auto& fail = az::fail_abi;

// HIP hardware queues of this process (GPU_MAX_HW_QUEUES, HIP's default 4),
// read once when the library loads -- HIP reads the variable at its own
// initialisation, so a value set later would not describe the queues HIP
// made; the lane rule (az_engine_lanes) uses this snapshot.  The Python
// package sets 8 at import before anything initialises HIP.
int read_hw_queues() {
  const char* q = getenv("GPU_MAX_HW_QUEUES");
  const int v = q && *q ? atoi(q) : 0;
  return v > 0 ? v : 4;
}
const int g_hw_queues_at_load = read_hw_queues();

}  // namespace

// A lane = a contiguous group of slots searched on its own HIP stream.  Lanes
// share the network, the transposition cache, the sample sink and the
// counters; each owns its eval queues and slices of the activation
// buffers.  Two lanes keep the GPU busy across each
// other's launch tails and small latency-bound kernels; results do not
// depend on the lane count (each game's search only reads its own tree and
// the evaluator is deterministic per board).
struct Lane : az::EvalLane {  // counts: [2][4][kCountStride], a block of eval/miss/nn counts per simulation parity
  az::GameCfg g{};
  az::TreeDev t{};
  az::ConvTimer tree_timer;  // select and expand launches (bench.py roofline_tree)
  int64_t pool_cap = 0;        // compacted self-play: edges per pool half (TreeDev::pool_cap)
};

// The session's streams: `stream`, the lanes' own when there is more than one
// lane, and the drain's pack stream.  The pack has no stream of its own with
// two or more lanes: HIP maps streams onto 4 hardware queues per process
// (GPU_MAX_HW_QUEUES), and a snapshot or pack stream sharing a lane's queue
// runs behind that lane's queued moves -- it uses `stream`, idle while moves run.
struct az_engine : az::Session {
  Lane whole;                // every slot on `stream` (tree API; self-play with one lane)
  std::vector<Lane*> lanes;  // self-play lanes (just &whole when there is one)
  az_config cfg{};
  az::GameCfg g{};
  az::TreeDev t{};
  az::SampleDev smp{};
  az::CacheDev cache{};
  az::NetDev net{};
  az::ConvTimer timer;
  double* uniforms = nullptr;
  double* noise_buf = nullptr;  // az_tree_search_noise: the caller's root-noise rows
  size_t noise_cap = 0;
  int32_t* dev_i32 = nullptr;  // scratch for az_tree_reset
  az::Board* dev_boards = nullptr;
  uint32_t leaf_epoch = 0;         // simulations enqueued, every lane's (TreeDev::leaf_epoch)
  uint8_t* drain_dev = nullptr;    // packed records (device) and their pinned host copy
  uint8_t* drain_host = nullptr;
  size_t drain_cap = 0;            // records the two buffers hold
};

namespace {

int check_device_errors(az_engine* e) {
  return az::device_error_status(e->t.stats, {"(raise az_config.arena_edges)", "(raise az_config.max_tree_visits)"});
}

az::Board board_from_cells(const int8_t* cells, int HW) {
  az::Board b;
  b.own[0] = b.own[1] = b.opp[0] = b.opp[1] = 0;
  for (int c = 0; c < HW; ++c) {
    if (cells[c] == 1) az::set_bit(b.own, c);
    else if (cells[c] == -1) az::set_bit(b.opp, c);
  }
  return b;
}

// point a tree view's four counters at parity p of the [2][4] block at base
void set_counts(az::TreeDev& t, int32_t* base, int p) {
  constexpr int K = az::kCountStride;
  t.eval_count = base + 4 * K * p;
  t.miss_count = t.eval_count + K;
  t.nn_count = t.eval_count + 2 * K;
  t.next_counts = base + 4 * K * (p ^ 1);
}

void cells_from_board(const az::Board& b, int HW, int8_t* cells) {
  for (int c = 0; c < HW; ++c)
    cells[c] = az::bit(b.own, c) ? 1 : (az::bit(b.opp, c) ? -1 : 0);
}

// AZ_EVAL_HOST: the leaves' full_state planes to the host, the callback (the
// reference's self.model(np.expand_dims(board.full_state, 0)), mcts.py:130-137,
// here over every leaf of the simulation at once), its outputs back to the
// lane's evaluator slices; synchronous on the lane's stream
int host_evaluate(az_engine* e, Lane& L, const az::Board* rows, const int32_t* n_rows) {
  az::launch_encode(rows, n_rows, L.n, L.g.HW, L.x, L.stream);
  AZ_HIP(hipGetLastError());
  return e->host.run(L.stream, L.x, n_rows, L.n, (size_t)L.g.HW * 4, L.g.A, L.probs, L.values);
}

// one simulation for every active slot of a lane (MCTS.search body,
// mcts.py:171-180), enqueued on the lane's stream
int simulate(az_engine* e, Lane& L) {
  hipStream_t s = L.stream;
  L.t.epoch += 1;
  // leaf records of any other simulation read as absent: the tag is unique
  // over the engine's lanes; when it wraps (2^32 simulations) the records are
  // cleared first, so none written 2^32 simulations ago can match
  if (++e->leaf_epoch == 0) {
    AZ_TRY(e->sync_all());
    AZ_HIP(hipMemset(e->t.leaf_src, 0, (size_t)e->g.slots * sizeof(uint64_t)));
    e->leaf_epoch = 1;
  }
  L.t.leaf_epoch = e->leaf_epoch;
  // eval_count, miss_count, nn_count: the epoch parity's block of
  // four (zeroed by the previous simulation's select kernel, or at creation)
  set_counts(L.t, L.counts, L.t.epoch & 1);
  if (L.tree_timer.enabled) L.tree_timer.begin(s);
  az::launch_select(L.g, L.t, e->cache, s);
  if (L.tree_timer.enabled) L.tree_timer.end(s, 1);
  const az::Board* rows = L.t.eval_board;
  const int32_t* n_rows = L.t.eval_count;
  if (e->cache.enabled) {  // the misses' rows (a board two slots miss on in one simulation has two)
    rows = L.t.nn_board;
    n_rows = L.t.nn_count;
  }
  if (e->cfg.evaluator == AZ_EVAL_NETWORK) {
    // the stem reads the queued boards straight (no encode pass; bitwise the same outputs)
    az::launch_forward(e->net, L.x, n_rows, L.n, L.g.H, L.g.W, L.g.A, L.act[0], L.act[1], L.act[2],
                       L.probs, L.values, s, L.timer.enabled ? &L.timer : nullptr, rows);
  } else if (e->cfg.evaluator == AZ_EVAL_HOST) {
    if (int rc = host_evaluate(e, L, rows, n_rows)) {
      e->broken = true;
      return rc;
    }
  } else {
    az::launch_synth_eval(L.g, rows, n_rows, L.probs, L.values, s);
  }
  if (L.tree_timer.enabled) L.tree_timer.begin(s);
  az::launch_expand(L.g, L.t, e->cache, L.probs, L.values, s);
  if (L.tree_timer.enabled) L.tree_timer.end(s, 1);
  AZ_HIP(hipGetLastError());
  return 0;
}

// the tree API never compacts (its views are the whole tree, like the
// reference's object graph): an engine created with compact = 1 sizes each
// arena half for one move, which a reused tree outgrows
int tree_api_ok(az_engine* e) {
  if (e->g.halves > 1)
    return fail(AZ_E_INVALID, "the tree API (az_tree_*) needs an engine created with compact = 0");
  return 0;
}

// (the caller has entered: no move is running)
int cache_clear(az_engine* e) {
  if (!e->cache.state) return 0;
  AZ_TRY(az::cache_clear(e->cache, e->stream));
  AZ_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

int ready_to_search(az_engine* e) { return e->ready_to_search(e->cfg.evaluator, e->net.ready, "az_"); }

// Lane views: per-slot arrays offset to the lane's first slot; with more than
// one lane each gets its own eval-queue counters.
int make_lane(az_engine* e, Lane* L, int first, int n, bool own_queue) {
  const az::GameCfg& g = e->g;
  L->g = g;
  L->g.slots = n;
  az::TreeDev t = e->t;
  const size_t f = (size_t)first;
  if (g.halves == 1) t.edges += f * g.arena_cap;  // pooled: the lane's own pool (alloc_pool)
  if (t.arena_end) t.arena_end += f;
  if (t.slot_live) t.slot_live += f;
  t.root_board += f;
  t.root_first += f;
  t.root_n += f;
  t.root_value += f;
  t.arena_top += f;
  t.ply += f;
  t.game_id += f;
  t.path += f * g.max_depth;
  t.path_len += f;
  t.slot_expansions += f;
  t.mt += f;  // word-major: stride stays the whole engine's slot count
  t.leaf_src += f;
  t.leaf_board += f;
  t.eval_board += f;

  t.nn_board += f;
  t.last_move += f;
  t.last_status += f;
  t.last_policy += f * g.A;
  if (own_queue) {
    int rc;
    if ((rc = e->mem.alloc(&t.eval_count, az::kCountWords, false))) return rc;
    AZ_HIP(hipMemset(t.eval_count, 0, az::kCountWords * sizeof(int32_t)));
    set_counts(t, t.eval_count, 0);
    t.epoch = 0;
  }
  L->counts = t.eval_count;
  L->t = t;
  e->slice(*L, first, n, (size_t)g.HW * 4, (size_t)g.HW * 128, g.A);
  return 0;
}

// compacted self-play: the lane's two pool halves of `cap` edges and their counters
int alloc_pool(az_engine* e, Lane* L, int64_t cap) {
  int rc;
  az::Edge* halves = nullptr;
  unsigned long long* tops = nullptr;
  if ((rc = e->mem.alloc(&halves, 2 * (size_t)cap, false)) || (rc = e->mem.alloc(&tops, 2, false))) return rc;
  AZ_HIP(hipMemset(tops, 0, 2 * sizeof(unsigned long long)));
  L->pool_cap = cap;
  L->t.pool_cap = (int32_t)cap;
  L->t.edges = halves;
  L->t.dst_edges = halves + cap;
  L->t.pool_top = tops;
  L->t.dst_top = tops + 1;
  return 0;
}

}  // namespace

extern "C" {

int az_abi_version(void) { return AZ_ABI_VERSION; }
#ifndef AZ_SRC_HASH
#define AZ_SRC_HASH "unknown"
#endif
#ifndef AZ_BUILD_EXTRA
#define AZ_BUILD_EXTRA "unknown"
#endif
const char* az_build_id(void) { return AZ_SRC_HASH; }
const char* az_build_flags(void) { return AZ_BUILD_EXTRA; }
const char* az_last_error(void) { return az::g_last_error.c_str(); }

int az_engine_create(int device, const az_config* cfg, az_engine** out) {
  if (!cfg || !out) return fail(AZ_E_INVALID, "null argument");
  const az_config& c = *cfg;
  if (c.board_height < 2 || c.board_width < 2 || c.board_height * c.board_width > az::kMaxCells)
    return fail(AZ_E_INVALID, "board must have 4..128 cells");
  if (c.n < 2 || c.n > std::min(c.board_height, c.board_width))
    return fail(AZ_E_INVALID, "need 2 <= n <= min(width, height) (connect_n/board.py:14-18)");
  const int A = c.gravity ? c.board_width : c.board_width * c.board_height;
  if (A > az::kMaxActions) return fail(AZ_E_INVALID, "action space too large");
  if (c.slots < 1 || c.mcts_iterations < 1) return fail(AZ_E_INVALID, "slots and mcts_iterations must be >= 1");
  az::NetRequest req;  // (its lanes: below, once they exist)
  req.conv_algo = c.conv_algo;
  req.H = c.board_height, req.W = c.board_width, req.A = A;
  req.depth = c.depth, req.hidden = c.value_hidden;
  req.natural_order = c.tower_natural_order != 0;
  req.network_evaluator = c.evaluator == AZ_EVAL_NETWORK;
  if (const az::NetStatus bad = az::check_net_request(req); bad.code != AZ_OK) return fail(bad.code, bad.message);
  if (c.depth < 0 || c.depth > 1024 || c.value_hidden < 1) return fail(AZ_E_INVALID, "need 0 <= depth and value_hidden >= 1");
  if (c.evaluator == AZ_EVAL_NETWORK && (int64_t)c.slots * c.board_height * c.board_width * 512 >= (1ll << 31))
    return fail(AZ_E_INVALID, "slots * H * W * 512 must stay below 2^31 (32-bit activation byte offsets)");
  if (c.evaluator != AZ_EVAL_NETWORK && c.evaluator != AZ_EVAL_SYNTHETIC && c.evaluator != AZ_EVAL_HOST)
    return fail(AZ_E_INVALID, "unknown evaluator");
  if (c.evaluator == AZ_EVAL_NETWORK && c.filters != 128)
    return fail(AZ_E_INVALID, "network evaluator supports filters == 128 (ConfigModel.filters)");
  AZ_TRY(az::open_device(device));

  az_engine* e = new az_engine();
  e->device = device;
  e->cfg = c;
  az::GameCfg& g = e->g;
  g.H = c.board_height;
  g.W = c.board_width;
  g.HW = g.H * g.W;
  g.n = c.n;
  g.gravity = c.gravity ? 1 : 0;
  g.A = A;
  g.sims = c.mcts_iterations;
  g.greedy_ply = c.index_move_greedy;
  g.c_puct = c.exploration_constant;
  g.slots = c.slots;
  g.max_depth = g.HW + 1;
  g.noise = c.dirichlet_noise != 0;
  g.noise_alpha = c.dirichlet_alpha;
  g.noise_ratio = c.dirichlet_ratio;
  g.rng_skip = c.rng_skip;
  if (c.rng_skip < 0) {
    delete e;
    return fail(AZ_E_INVALID, "rng_skip must be >= 0");
  }
  if (g.noise && !(c.dirichlet_alpha > 0.0 && c.dirichlet_alpha <= 1.0 && std::isfinite(c.dirichlet_ratio))) {
    delete e;
    return fail(AZ_E_INVALID, "Dirichlet noise needs 0 < dirichlet_alpha <= 1 (the reference's 0.03) and a "
                              "finite dirichlet_ratio");
  }
  const int64_t visits = c.max_tree_visits > 0 ? c.max_tree_visits : (int64_t)c.mcts_iterations * g.HW + 2;
  // a slot's tree holds at most mcts_iterations * H*W expansions of <= A edges
  // (one game): `safe` edges per slot can never overflow.
  //  * uncompacted (tree API): a static run of arena_edges (default safe) per slot;
  //  * compacted self-play (az_config.compact): pooled arenas (az_tree.h) -- per
  //    lane two halves of arena_edges x the lane's slots, arena_edges (an
  //    average per slot) defaulting to safe when two such halves per slot fit
  //    in 40% of the free HBM, else the most that does (at least 8 S A + H W A).
  //    A slot holds what it uses -- one move's search plus its kept subtree,
  //    a few thousand edges at configs[1] -- so the pool is shared: a game
  //    whose kept subtree grows toward the whole game's search (a peaked
  //    network) takes the room other slots leave.  Overflow is kErrArena,
  //    never an overrun.
  g.halves = c.compact ? 2 : 1;
  const int64_t safe = (int64_t)c.mcts_iterations * g.HW * A + A;
  int64_t arena = c.arena_edges > 0 ? c.arena_edges : safe;
  if (c.arena_edges <= 0 && c.compact) {
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const int64_t fit = (int64_t)(0.4 * (double)free_b / ((double)c.slots * 2.0 * sizeof(az::Edge)));
      arena = std::min(safe, std::max(fit, (int64_t)8 * c.mcts_iterations * A + (int64_t)g.HW * A));
    }
  }
  if (visits > (1 << 30) || arena > (1 << 30) || (c.compact && arena < 2 * az::kPoolChunkA * A)) {
    delete e;
    return fail(AZ_E_INVALID, "tree bounds too large (or a pooled arena below two chunks per slot)");
  }
  g.pow_len = (int)visits;
  g.arena_cap = (int)arena;

  auto cleanup = [&](int rc) {
    az_engine_destroy(e);
    return rc;
  };
  int rc;
  if ((rc = e->new_stream(&e->stream))) return cleanup(rc);
  if (c.lanes < 0) return cleanup(fail(AZ_E_INVALID, "lanes must be >= 0"));
  const size_t S = (size_t)g.slots;
  az::TreeDev& t = e->t;
  t.edges = nullptr;
  t.arena_end = t.slot_live = nullptr;
  if (g.halves == 1 && (rc = e->mem.alloc(&t.edges, S * (size_t)g.arena_cap, false))) return cleanup(rc);
  if (g.halves > 1 && ((rc = e->mem.alloc(&t.arena_end, S, false)) || (rc = e->mem.alloc(&t.slot_live, S, false)))) return cleanup(rc);
  if ((rc = e->mem.alloc(&t.root_board, S, false)) ||
      (rc = e->mem.alloc(&t.root_first, S, false)) || (rc = e->mem.alloc(&t.root_n, S, false)) ||
      (rc = e->mem.alloc(&t.root_value, S, false)) || (rc = e->mem.alloc(&t.arena_top, S, false)) ||
      (rc = e->mem.alloc(&t.ply, S, false)) || (rc = e->mem.alloc(&t.game_id, S, false)) ||
      (rc = e->mem.alloc(&t.path, S * g.max_depth, false)) || (rc = e->mem.alloc(&t.path_len, S, false)) ||
      (rc = e->mem.alloc(&t.slot_expansions, S, false)) || (rc = e->mem.alloc(&t.mt, S * (az::kMtN + 1), false)) ||
      (rc = e->mem.alloc(&t.leaf_src, S, false)) || (rc = e->mem.alloc(&t.leaf_board, S, false)) ||
      (rc = e->mem.alloc(&t.eval_board, S, false)) || (rc = e->mem.alloc(&t.nn_board, S, false)) ||
      (rc = e->mem.alloc(&t.eval_count, az::kCountWords, false)) || (rc = e->mem.alloc(&t.stats, az::kStatCount, false)) ||
      (rc = e->mem.alloc(&t.last_move, S, false)) || (rc = e->mem.alloc(&t.last_status, S, false)) ||
      (rc = e->mem.alloc(&t.last_policy, S * A, false)))
    return cleanup(rc);
  double* powtab = nullptr;
  if ((rc = e->mem.alloc(&powtab, g.pow_len, false))) return cleanup(rc);
  {
    const std::vector<double> h = az::sqrt_pow_table(g.pow_len);
    if (hipMemcpy(powtab, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      return cleanup(fail(AZ_E_HIP, "pow table upload failed"));
  }
  t.powtab = powtab;
  t.mt_stride = g.slots;
  set_counts(t, t.eval_count, 0);
  t.epoch = 0;
  // leaf records start untagged (leaf_epoch counts from 1)
  if (hipMemset(t.leaf_src, 0, S * sizeof(uint64_t)) != hipSuccess)
    return cleanup(fail(AZ_E_HIP, "memset failed"));
  // LRU eviction by generations of cap/kCacheGenDiv inserts -- or, for a
  // larger batch, of more than three moves of every slot's inserts: select
  // finds an entry and expand reads its payload one launch later, on lanes
  // that move events keep within two moves of each other (configs[2]'s 8192 x
  // S=200 and configs[3]'s 4096 x S=400 need it at 2^26 entries)
  if ((rc = az::cache_create(e->mem, e->cache, c.cache_log2, 30, A + 1,
                             3ull * (unsigned long long)g.slots * (unsigned long long)g.sims)))
    return cleanup(rc);
  if (hipMemset(t.stats, 0, az::kStatCount * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(t.eval_count, 0, az::kCountWords * sizeof(int32_t)) != hipSuccess ||

      hipMemset(t.game_id, 0xff, S * sizeof(int64_t)) != hipSuccess)
    return cleanup(fail(AZ_E_HIP, "memset failed"));
  // evaluator buffers (batch = slots)
  if ((rc = e->mem.alloc(&e->probs, S * A, false)) || (rc = e->mem.alloc(&e->values, S, false)) ||
      (rc = e->mem.alloc(&e->uniforms, S, false)) || (rc = e->mem.alloc(&e->dev_i32, S, false)) ||
      (rc = e->mem.alloc(&e->dev_boards, S, false)))
    return cleanup(rc);
  if ((rc = e->mem.alloc(&e->x, S * g.HW * 4, false))) return cleanup(rc);
  if (c.evaluator == AZ_EVAL_HOST && (rc = e->host.create(S, (size_t)g.HW * 4, A))) return cleanup(rc);
  if (c.evaluator == AZ_EVAL_NETWORK) {
    const size_t act = S * g.HW * 128;
    for (int i = 0; i < 3; ++i)
      if ((rc = e->mem.alloc(&e->act[i], act, false))) return cleanup(rc);
  }
  e->net.req = req;  // the forward's form: load_network, once the weights and the device are known
  e->net.err = e->t.stats + az::kStatErrors;
  // lanes: 0 = auto (two streams once each lane still holds a few hundred
  // games; three for 1536-4096 slots when HIP gives the process a hardware
  // queue per stream -- with 4 a third lane shares one and loses 27%:
  // profiles/r5/ab_queues_lanes.txt; larger launches keep two)
  int nl = c.lanes;
  if (nl <= 0) {
    const int queues = g_hw_queues_at_load;
    nl = g.slots < 512 ? 1 : (queues >= 8 && g.slots >= 1536 && g.slots <= 4096) ? 3 : 2;
  }
  nl = std::min(nl, std::min(g.slots, 8));
  if ((rc = make_lane(e, &e->whole, 0, g.slots, false))) return cleanup(rc);
  e->whole.stream = e->stream;
  if (nl == 1) {
    e->lanes.push_back(&e->whole);
  } else {
    for (int l = 0; l < nl; ++l) {
      Lane* L = new Lane();
      e->lanes.push_back(L);
      const int lo = (int)((int64_t)g.slots * l / nl), hi = (int)((int64_t)g.slots * (l + 1) / nl);
      if ((rc = make_lane(e, L, lo, hi - lo, true)) || (rc = e->new_lane_stream(&L->stream))) return cleanup(rc);
    }
  }
  e->net.req.lanes = (int)e->lanes.size();  // (the tower's dual-launch threshold)
  if (g.halves > 1)  // pooled arenas, one pool per lane (whose indices stay below 2^31)
    for (Lane* L : e->lanes)
      if ((rc = alloc_pool(e, L, std::min<int64_t>((int64_t)g.arena_cap * L->n, (1ll << 31) - 1))))
        return cleanup(rc);
  // drain: one lane runs on `stream`, so the pack needs a stream of its own;
  // with more lanes `stream` is idle while moves run
  e->own_pack_stream = nl == 1;
  e->pack_stream = e->stream;
  if (e->own_pack_stream && (rc = e->new_stream(&e->pack_stream))) return cleanup(rc);
  if ((rc = e->clock.create(e->mem, nl, "drain snapshot setup failed"))) return cleanup(rc);
  *out = e;
  return 0;
}

int az_engine_lanes(const az_engine* eng) { return eng ? (int)eng->lanes.size() : 0; }

int az_engine_destroy(az_engine* eng) {
  if (!eng) return 0;
  eng->destroy();
  for (Lane* L : eng->lanes)
    if (L != &eng->whole) delete L;
  if (eng->drain_dev) (void)hipFree(eng->drain_dev);
  if (eng->drain_host) (void)hipHostFree(eng->drain_host);
  delete eng;
  return 0;
}

int az_engine_set_evaluator(az_engine* e, az_eval_fn fn, void* user) {
  if (!e || !fn) return fail(AZ_E_INVALID, "null argument");
  if (e->cfg.evaluator != AZ_EVAL_HOST) return fail(AZ_E_STATE, "the engine was not created with AZ_EVAL_HOST");
  AZ_TRY(e->enter());
  e->host.fn = fn;
  e->host.user = user;
  return cache_clear(e);  // cached outputs belong to the previous evaluator
}

int az_engine_set_weights(az_engine* e, const az_tensor* tensors, int n) {
  if (!e || (!tensors && n)) return fail(AZ_E_INVALID, "null argument");
  AZ_TRY(e->enter());
  int rc;
  if ((rc = az::load_network(e->net, tensors, n, e->cfg.bn_epsilon, e->mem))) return rc;
  return cache_clear(e);  // cached outputs belong to the previous weights
}

int az_encode(az_engine* e, const int8_t* boards, int n, float* state, uint8_t* mask) {
  if (!e || n < 0 || (n && !boards)) return fail(AZ_E_INVALID, "bad arguments");
  AZ_TRY(e->enter());
  const int HW = e->g.HW, A = e->g.A;
  const int chunk = e->g.slots;
  std::vector<az::Board> hb(std::min(n, chunk));
  uint8_t* dmask = reinterpret_cast<uint8_t*>(e->probs);  // slots*A floats >= slots*A bytes
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    for (int i = 0; i < m; ++i) hb[i] = board_from_cells(boards + (size_t)(off + i) * HW, HW);
    AZ_HIP(hipMemcpyAsync(e->dev_boards, hb.data(), m * sizeof(az::Board), hipMemcpyHostToDevice, e->stream));
    if (state) {
      az::launch_encode(e->dev_boards, nullptr, m, HW, e->x, e->stream);
      AZ_HIP(hipMemcpyAsync(state + (size_t)off * HW * 4, e->x, (size_t)m * HW * 4 * sizeof(float),
                            hipMemcpyDeviceToHost, e->stream));
    }
    if (mask) {
      az::launch_legal_mask(e->dev_boards, m, e->g, dmask, e->stream);
      AZ_HIP(hipMemcpyAsync(mask + (size_t)off * A, dmask, (size_t)m * A, hipMemcpyDeviceToHost, e->stream));
    }
    AZ_HIP(hipStreamSynchronize(e->stream));
  }
  return 0;
}

int az_forward(az_engine* e, const float* x, int n, float* probs, float* values) {
  if (!e || n < 0 || (n && (!x || !probs || !values))) return fail(AZ_E_INVALID, "bad arguments");
  if (!e->net.ready) return fail(AZ_E_STATE, "az_engine_set_weights was not called");
  AZ_TRY(e->enter());
  const int HW = e->g.HW, A = e->g.A, chunk = e->g.slots;
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    AZ_HIP(hipMemcpyAsync(e->x, x + (size_t)off * HW * 4, (size_t)m * HW * 4 * sizeof(float),
                          hipMemcpyHostToDevice, e->stream));
    az::launch_forward(e->net, e->x, nullptr, m, e->g.H, e->g.W, A, e->act[0], e->act[1], e->act[2],
                       e->probs, e->values, e->stream, e->timer.enabled ? &e->timer : nullptr);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(probs + (size_t)off * A, e->probs, (size_t)m * A * sizeof(float),
                          hipMemcpyDeviceToHost, e->stream));
    AZ_HIP(hipMemcpyAsync(values + off, e->values, (size_t)m * sizeof(float), hipMemcpyDeviceToHost,
                          e->stream));
    AZ_HIP(hipStreamSynchronize(e->stream));
  }
  return 0;
}

int az_stats_get(az_engine* e, az_stats* st) {
  if (!e || !st) return fail(AZ_E_INVALID, "null argument");
  AZ_TRY(e->enter());
  int rc;
  unsigned long long h[az::kStatCount];
  if ((rc = az::read_common_stats(st, h, e->t.stats, e->t.game_id, e->g.slots, e->cache)))
    return rc;
  std::vector<az::ConvTimer*> timers = {&e->timer, &e->whole.timer};
  for (Lane* L : e->lanes)
    if (L != &e->whole) timers.push_back(&L->timer);
  az::conv_busy_union(timers, st);
  std::vector<az::ConvTimer*> ttimers = {&e->whole.tree_timer};
  for (Lane* L : e->lanes)
    if (L != &e->whole) ttimers.push_back(&L->tree_timer);
  for (az::ConvTimer* tm : ttimers) {
    tm->flush();
    st->tree_ms += tm->total_ms;
    st->tree_launches += tm->launches;
  }
  st->path_edges = (int64_t)h[az::kStatPathEdges];
  st->max_retained = (int64_t)h[az::kStatMaxRetained];
  st->games_drained = e->clock.drained;
  st->arena_edges = e->g.arena_cap;
  if (e->g.halves > 1) {
    st->arena_pool_edges = 0;
    for (Lane* L : e->lanes) st->arena_pool_edges += 2 * L->pool_cap;
    st->arena_pool_high = (int64_t)h[az::kStatPoolHigh];
  }
  const az::IssuedFlop flop = az::issued_flop_per_board(e->net.form, e->net.terms, e->net.layout);
  st->issued_flop_per_board = flop.main;
  st->issued_flop_per_board_small = flop.alt;
  st->tower_small_max_boards = e->net.layout.alt_max_boards;  // (-1: no alt tiles, or no tower)
  return 0;
}

int az_cache_enable(az_engine* e, int on) {
  if (!e) return fail(AZ_E_INVALID, "null engine");
  if (!e->cache.state) return on ? fail(AZ_E_STATE, "engine created with cache_log2 = 0") : 0;
  AZ_TRY(e->enter());
  e->cache.enabled = on != 0;
  return 0;
}

int az_cache_clear(az_engine* e) {
  if (!e) return fail(AZ_E_INVALID, "null engine");
  AZ_TRY(e->enter());
  return cache_clear(e);
}

int az_timer_enable(az_engine* e, int on) {
  if (!e) return fail(AZ_E_INVALID, "null engine");
  AZ_TRY(e->enter());
  // on: 1 = conv launches, 2 = conv + select/expand launches (more events per
  // simulation: bench.py times the tree kernels in a window of their own),
  // k >= 3 = every k-th conv launch of each lane (sampled)
  std::vector<az::ConvTimer*> timers = {&e->timer, &e->whole.timer}, ttimers = {&e->whole.tree_timer};
  for (Lane* L : e->lanes)
    if (L != &e->whole) {
      timers.push_back(&L->timer);
      ttimers.push_back(&L->tree_timer);
    }
  // (both lists share the origin; the second call records it again, on streams still idle)
  AZ_TRY(az::arm_timers(&e->timer_ref, e->stream, timers, on != 0, on >= 3 ? on : 1));
  return az::arm_timers(&e->timer_ref, e->stream, ttimers, on >= 2, 1);
}

int az_pow_table(az_engine* e, double* out, int64_t n) {
  if (!e || !out || n < 0 || n > e->g.pow_len) return fail(AZ_E_INVALID, "bad arguments");
  AZ_TRY(e->enter());
  AZ_HIP(hipMemcpy(out, e->t.powtab, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------ self-play
int az_selfplay_begin(az_engine* e, int64_t first_game, int64_t n_games, uint32_t base_seed) {
  if (!e || n_games < 0 || first_game < 0) return fail(AZ_E_INVALID, "bad arguments");
  int rc;
  e->broken = false;  // every slot starts a fresh game
  if ((rc = ready_to_search(e))) return rc;
  AZ_TRY(e->enter());  // moves of an earlier batch may still be running (async steps)
  e->samples.free_all();
  az::SampleDev& smp = e->smp;
  smp = az::SampleDev{};
  smp.first_game = first_game;
  smp.n_games = n_games;
  smp.base_seed = base_seed;
  const size_t G = (size_t)std::max<int64_t>(n_games, 1), P = (size_t)e->g.HW, A = (size_t)e->g.A;
  az::DeviceAllocs& sb = e->samples;
  hipStream_t s = e->stream;
  if ((rc = sb.alloc_zeroed_async(&smp.boards, G * P, s)) || (rc = sb.alloc_zeroed_async(&smp.policy, G * P * A, s)) ||
      (rc = sb.alloc_zeroed_async(&smp.moves, G * P, s)) || (rc = sb.alloc_zeroed_async(&smp.length, G, s)) ||
      (rc = sb.alloc_zeroed_async(&smp.result, G, s)) || (rc = sb.alloc_zeroed_async(&smp.expansions, G, s)) ||
      (rc = sb.alloc_zeroed_async(&smp.done_ids, G, s)) || (rc = sb.alloc_zeroed_async(&smp.done_count, 1, s)))
    return rc;
  return e->begin_batch(e->t.stats, e->g.slots, first_game, n_games, [&](int64_t first_wave) {
    az::launch_slot_init(e->g, e->t, smp, first_wave, e->stream);
    AZ_HIP(hipGetLastError());
    if (e->g.halves > 1)  // every slot starts with no chunk: the pools are empty
      for (Lane* L : e->lanes) {
        AZ_HIP(hipMemsetAsync(L->t.pool_top, 0, sizeof(unsigned long long), e->stream));
        AZ_HIP(hipMemsetAsync(L->t.dst_top, 0, sizeof(unsigned long long), e->stream));
      }
    return 0;
  });
}

int az_selfplay_step(az_engine* e, int n_moves, az_stats* st) {
  if (!e || n_moves < 0) return fail(AZ_E_INVALID, "bad arguments");
  int rc;
  if ((rc = ready_to_search(e))) return rc;
  rc = e->step_moves(
      n_moves, e->g.sims, e->lanes, e->smp.done_count, [&](Lane& L) { return simulate(e, L); },
      [](Lane&) { return 0; },
      [&](Lane& L) {
        az::launch_play(L.g, L.t, e->smp, nullptr, -1, 0, 1, L.stream);
        az::launch_compact(L.g, L.t, L.stream);
        if (L.g.halves > 1) {  // the kept trees are in the other half now: it is the current one
          std::swap(L.t.edges, L.t.dst_edges);
          std::swap(L.t.pool_top, L.t.dst_top);
        }
      });
  if (rc || !st) return rc;  // st = NULL, asynchronous: the moves run on while the caller drains earlier ones
  if ((rc = e->sync_all())) return rc;
  if ((rc = check_device_errors(e))) return rc;
  return az_stats_get(e, st);
}

int az_selfplay_run(az_engine* e, int64_t first_game, int64_t n_games, uint32_t base_seed,
                    az_stats* st) {
  return az::run_to_end(
      st, [&] { return az_selfplay_begin(e, first_game, n_games, base_seed); },
      [&](az_stats* now) { return az_selfplay_step(e, 1, now); });
}

int az_selfplay_results(az_engine* e, int32_t* lengths, int32_t* results, int32_t* expansions,
                        int8_t* boards, double* policies, int32_t* moves) {
  if (!e) return fail(AZ_E_INVALID, "null engine");
  AZ_TRY(e->enter());
  const size_t G = (size_t)e->sp_n, P = (size_t)e->g.HW, A = (size_t)e->g.A, HW = (size_t)e->g.HW;
  if (G == 0) return 0;
  const az::SampleDev& smp = e->smp;
  if (lengths) AZ_HIP(hipMemcpy(lengths, smp.length, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (results) AZ_HIP(hipMemcpy(results, smp.result, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (expansions) AZ_HIP(hipMemcpy(expansions, smp.expansions, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (policies) AZ_HIP(hipMemcpy(policies, smp.policy, G * P * A * sizeof(double), hipMemcpyDeviceToHost));
  if (boards) {
    std::vector<az::Board> hb(G * P);
    AZ_HIP(hipMemcpy(hb.data(), smp.boards, hb.size() * sizeof(az::Board), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hb.size(); ++i) cells_from_board(hb[i], (int)HW, boards + i * HW);
  }
  if (moves) {
    std::vector<int16_t> hm(G * P);
    AZ_HIP(hipMemcpy(hm.data(), smp.moves, hm.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hm.size(); ++i) moves[i] = hm[i];
  }
  return 0;
}

int az_selfplay_drain(az_engine* e, int64_t max_games, int64_t* n_out, int64_t* game_ids, int32_t* lengths,
                      int32_t* results, int32_t* expansions, int8_t* boards, double* policies,
                      int32_t* moves) {
  if (!e || !n_out || max_games < 0) return fail(AZ_E_INVALID, "bad arguments");
  *n_out = 0;
  if (!e->smp.done_count) return 0;  // no self-play batch begun
  AZ_HIP(hipSetDevice(e->device));
  int64_t n = 0;
  if (int rc = e->clock.drainable(max_games, &n)) return rc;
  if (n <= 0) return 0;
  const size_t rec = az::drain_record_bytes(e->g);
  if ((size_t)n > e->drain_cap) {
    if (e->drain_dev) AZ_HIP(hipFree(e->drain_dev));
    if (e->drain_host) AZ_HIP(hipHostFree(e->drain_host));
    e->drain_dev = nullptr;
    e->drain_host = nullptr;
    e->drain_cap = 0;
    const size_t cap = std::max<size_t>((size_t)n, 1024);
    AZ_HIP(hipMalloc(&e->drain_dev, cap * rec));
    AZ_HIP(hipHostMalloc(&e->drain_host, cap * rec, hipHostMallocDefault));
    e->drain_cap = cap;
  }
  // pack_stream (nothing else queued on it; the host has seen the snapshot's
  // move finish on every lane): the games it counts are complete
  az::launch_drain_pack(e->g, e->smp, e->clock.drained, (int)n, e->drain_dev, e->pack_stream);
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipMemcpyAsync(e->drain_host, e->drain_dev, (size_t)n * rec, hipMemcpyDeviceToHost, e->pack_stream));
  AZ_HIP(hipStreamSynchronize(e->pack_stream));
  const size_t HW = (size_t)e->g.HW, A = (size_t)e->g.A;
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t* r = e->drain_host + (size_t)i * rec;
    const int32_t* h = reinterpret_cast<const int32_t*>(r + 8);
    if (game_ids) memcpy(game_ids + i, r, sizeof(int64_t));
    if (lengths) lengths[i] = h[0];
    if (results) results[i] = h[1];
    if (expansions) expansions[i] = h[2];
    if (policies) memcpy(policies + i * HW * A, r + 24, HW * A * sizeof(double));
    const int16_t* mv = reinterpret_cast<const int16_t*>(r + 24 + 8 * HW * A);
    if (moves)
      for (size_t p = 0; p < HW; ++p) moves[i * HW + p] = mv[p];
    if (boards) memcpy(boards + i * HW * HW, mv + HW, HW * HW);
  }
  e->clock.drained += n;
  *n_out = n;
  return 0;
}

// ------------------------------------------------------------------ tree API
int az_tree_reset(az_engine* e, int n, const int32_t* slots, const int8_t* boards) {
  if (!e || n < 0 || n > e->g.slots || (n && (!slots || !boards))) return fail(AZ_E_INVALID, "bad arguments");
  AZ_TRY(e->enter());
  if (int rc_ = tree_api_ok(e)) return rc_;
  std::vector<az::Board> hb(n);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= e->g.slots) return fail(AZ_E_INVALID, "slot out of range");
    hb[i] = board_from_cells(boards + (size_t)i * e->g.HW, e->g.HW);
  }
  e->smp = az::SampleDev{};
  AZ_HIP(hipMemcpyAsync(e->dev_i32, slots, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  AZ_HIP(hipMemcpyAsync(e->dev_boards, hb.data(), n * sizeof(az::Board), hipMemcpyHostToDevice, e->stream));
  az::launch_slot_set_root(e->g, e->t, e->dev_i32, e->dev_boards, n, e->stream);
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipStreamSynchronize(e->stream));
  e->broken = false;
  return 0;
}

int az_tree_release(az_engine* e, int n, const int32_t* slots) {
  if (!e || n < 0 || n > e->g.slots || (n && !slots)) return fail(AZ_E_INVALID, "bad arguments");
  AZ_TRY(e->enter());
  for (int i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= e->g.slots) return fail(AZ_E_INVALID, "slot out of range");
  AZ_HIP(hipMemcpyAsync(e->dev_i32, slots, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  az::launch_slot_release(e->t, e->dev_i32, n, e->stream);
  AZ_HIP(hipGetLastError());
  AZ_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

int az_tree_search(az_engine* e, int n_sims) {
  if (!e || n_sims < 0) return fail(AZ_E_INVALID, "bad arguments");
  if (e->g.noise)  // the tree API's noise is drawn by the caller from numpy's global stream
    return fail(AZ_E_INVALID, "this engine mixes Dirichlet root noise: search it with az_tree_search_noise "
                              "(the caller's np.random.dirichlet draws)");
  int rc;
  if ((rc = ready_to_search(e))) return rc;
  AZ_TRY(e->enter());
  if (int rc_ = tree_api_ok(e)) return rc_;
  for (int s = 0; s < n_sims; ++s)
    if ((rc = simulate(e, e->whole))) return rc;
  AZ_HIP(hipStreamSynchronize(e->stream));
  return check_device_errors(e);
}

int az_tree_search_noise(az_engine* e, int n_sims, const double* noise, int rows) {
  if (!e || n_sims < 0 || rows < 0 || (rows > 0 && !noise)) return fail(AZ_E_INVALID, "bad arguments");
  if (!e->g.noise)
    return fail(AZ_E_INVALID, "az_tree_search_noise needs an engine created with dirichlet_noise = 1");
  int rc;
  if ((rc = ready_to_search(e))) return rc;
  AZ_TRY(e->enter());
  if (int rc_ = tree_api_ok(e)) return rc_;
  const size_t S = (size_t)e->g.slots, n = S * (size_t)std::max(rows, 1) * e->g.A;
  az::TreeDev& t = e->whole.t;
  if (n > e->noise_cap) {  // grown on demand, kept for the next searches
    double* buf = nullptr;
    if ((rc = e->mem.alloc(&buf, n, false))) return rc;
    e->noise_buf = buf;
    e->noise_cap = n;
  }
  if (!t.noise_cur && (rc = e->mem.alloc(&t.noise_cur, S, false))) return rc;
  if (rows) AZ_HIP(hipMemcpyAsync(e->noise_buf, noise, S * rows * e->g.A * sizeof(double), hipMemcpyHostToDevice,
                                  e->stream));
  AZ_HIP(hipMemsetAsync(t.noise_cur, 0, S * sizeof(int32_t), e->stream));
  t.noise_in = e->noise_buf;
  t.noise_rows = rows;
  rc = 0;
  for (int s = 0; s < n_sims && !rc; ++s) rc = simulate(e, e->whole);
  t.noise_in = nullptr;  // self-play keeps drawing on the device
  t.noise_rows = 0;
  if (rc) return rc;
  AZ_HIP(hipStreamSynchronize(e->stream));
  return check_device_errors(e);
}

int az_tree_play(az_engine* e, const double* uniforms, int greedy, int deterministic,
                 int32_t* moves, int32_t* status, double* policy) {
  if (!e || (!deterministic && !uniforms)) return fail(AZ_E_INVALID, "bad arguments");
  if (e->broken) return ready_to_search(e);
  AZ_TRY(e->enter());
  if (int rc_ = tree_api_ok(e)) return rc_;
  const size_t S = (size_t)e->g.slots;
  if (!deterministic)
    AZ_HIP(hipMemcpyAsync(e->uniforms, uniforms, S * sizeof(double), hipMemcpyHostToDevice, e->stream));
  AZ_HIP(hipMemsetAsync(e->t.last_move, 0xff, S * sizeof(int32_t), e->stream));
  az::SampleDev none{};
  az::launch_play(e->g, e->t, none, deterministic ? nullptr : e->uniforms, greedy ? 1 : 0,
                  deterministic, 0, e->stream);
  AZ_HIP(hipGetLastError());
  if (moves) AZ_HIP(hipMemcpyAsync(moves, e->t.last_move, S * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (status) AZ_HIP(hipMemcpyAsync(status, e->t.last_status, S * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (policy)
    AZ_HIP(hipMemcpyAsync(policy, e->t.last_policy, S * e->g.A * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  AZ_HIP(hipStreamSynchronize(e->stream));
  return check_device_errors(e);
}

int az_tree_info(az_engine* e, int slot, int64_t* info, float* root_value) {
  if (!e || !info || slot < 0 || slot >= e->g.slots) return fail(AZ_E_INVALID, "bad arguments");
  AZ_TRY(e->enter());
  int32_t top, first, cnt, ply;
  int64_t gid;
  AZ_HIP(hipMemcpy(&top, e->t.arena_top + slot, 4, hipMemcpyDeviceToHost));
  AZ_HIP(hipMemcpy(&first, e->t.root_first + slot, 4, hipMemcpyDeviceToHost));
  AZ_HIP(hipMemcpy(&cnt, e->t.root_n + slot, 4, hipMemcpyDeviceToHost));
  AZ_HIP(hipMemcpy(&ply, e->t.ply + slot, 4, hipMemcpyDeviceToHost));
  AZ_HIP(hipMemcpy(&gid, e->t.game_id + slot, 8, hipMemcpyDeviceToHost));
  if (root_value) AZ_HIP(hipMemcpy(root_value, e->t.root_value + slot, 4, hipMemcpyDeviceToHost));
  info[0] = top;
  info[1] = first;
  info[2] = cnt;
  info[3] = ply;
  info[4] = gid >= 0;
  return 0;
}

int az_tree_export(az_engine* e, int slot, double* prior, double* w, int32_t* n, int32_t* child,
                   int32_t* child_n, int32_t* action, float* child_value) {
  if (!e || slot < 0 || slot >= e->g.slots) return fail(AZ_E_INVALID, "bad arguments");
  AZ_TRY(e->enter());
  if (int rc_ = tree_api_ok(e)) return rc_;
  int32_t top;
  AZ_HIP(hipMemcpy(&top, e->t.arena_top + slot, 4, hipMemcpyDeviceToHost));
  std::vector<az::Edge> h(top);
  if (top)
    AZ_HIP(hipMemcpy(h.data(), e->t.edges + (size_t)slot * e->g.arena_cap, top * sizeof(az::Edge),
                     hipMemcpyDeviceToHost));
  for (int i = 0; i < top; ++i) {
    if (prior) prior[i] = h[i].prior;
    if (w) w[i] = h[i].W;
    if (n) n[i] = h[i].N;
    if (child) child[i] = h[i].child;
    if (child_n) child_n[i] = h[i].child_n;
    if (action) action[i] = h[i].action & az::kActMask;
    if (child_value) child_value[i] = h[i].child_value;
  }
  return 0;
}

}  // extern "C"
