// az_host.h -- host code the C-ABI translation units share (az_engine.hip,
// az_chess_mcts.hip, az_chess.hip, az_train.hip): error reporting, the device
// of a handle, owned device memory, the device error flags, the move clock
// behind asynchronous self-play steps and the drain, and the stats read-out.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "../../include/az.h"
#include "az_move_clock.h"
#include "az_nn.h"
#include "az_tree.h"

namespace az {

// az_last_error's text, per thread
inline thread_local std::string g_last_error;

inline int fail_abi(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define AZ_HIP(expr)                                                                       \
  do {                                                                                     \
    hipError_t err__ = (expr);                                                             \
    if (err__ != hipSuccess)                                                               \
      return az::fail_abi(AZ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(err__)); \
  } while (0)

#define AZ_TRY(expr)                \
  do {                              \
    const int rc__ = (expr);        \
    if (rc__ != AZ_OK) return rc__; \
  } while (0)

// Makes `device` current; bad_index is the caller's wording for an ordinal past the devices.
inline int open_device(int device, const char* bad_index = "bad device index") {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail_abi(AZ_E_HIP, "no HIP device visible: libaz has no CPU fallback");
  if (device < 0 || device >= count) return fail_abi(AZ_E_INVALID, bad_index);
  AZ_HIP(hipSetDevice(device));
  return 0;
}

// Device allocations a handle frees together.
struct DeviceAllocs {
  std::vector<void*> ptrs;

  template <typename T>
  int alloc(T** p, size_t count, bool zero) {
    void* q = nullptr;
    AZ_HIP(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    ptrs.push_back(q);
    if (zero) AZ_HIP(hipMemset(q, 0, std::max<size_t>(count, 1) * sizeof(T)));
    *p = static_cast<T*>(q);
    return 0;
  }
  // at least 16 bytes, zeroed on stream s (the self-play sample buffers)
  template <typename T>
  int alloc_zeroed_async(T** p, size_t count, hipStream_t s) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    void* q = nullptr;
    AZ_HIP(hipMalloc(&q, bytes));
    ptrs.push_back(q);
    *p = static_cast<T*>(q);
    AZ_HIP(hipMemsetAsync(q, 0, bytes, s));
    return 0;
  }
  void free_all() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};

// The transposition cache of an engine (az_cache.h): 2^cache_log2 entries of
// pay_floats payload floats each, empty; cache_log2 = 0 leaves c off.  max_log2
// is the engine's limit, reader_window_inserts its cache_gen_size argument.
template <typename Key>
int cache_create(DeviceAllocs& mem, Cache<Key>& c, int cache_log2, int max_log2, size_t pay_floats,
                 unsigned long long reader_window_inserts) {
  if (cache_log2 < 0 || cache_log2 > max_log2 || (cache_log2 > 0 && cache_log2 < 4))
    return fail_abi(AZ_E_INVALID, "cache_log2 must be 0 (no cache) or 4.." + std::to_string(max_log2));
  if (cache_log2 == 0) return 0;
  const size_t cap = (size_t)1 << cache_log2;
  AZ_TRY(mem.alloc(&c.keys, cap, false));
  AZ_TRY(mem.alloc(&c.state, cap, false));
  AZ_TRY(mem.alloc(&c.pay, cap * pay_floats, false));
  AZ_TRY(mem.alloc(&c.ctl, 4, false));
  c.mask = (uint32_t)(cap - 1);
  c.enabled = 1;
  c.gen_size = cache_gen_size(cap, reader_window_inserts);
  if (hipMemset(c.state, 0, cap * sizeof(uint32_t)) != hipSuccess ||
      hipMemset(c.ctl, 0, 4 * sizeof(unsigned long long)) != hipSuccess)
    return fail_abi(AZ_E_HIP, "cache memset failed");
  return 0;
}

// Empties the cache (every state word Empty, the control words 0) on stream s;
// the caller keeps the cache's kernels away before and waits for s after.
inline int cache_clear(const CacheCore& c, hipStream_t s) {
  AZ_HIP(hipMemsetAsync(c.state, 0, ((size_t)c.mask + 1) * sizeof(uint32_t), s));
  AZ_HIP(hipMemsetAsync(c.ctl, 0, 4 * sizeof(unsigned long long), s));
  return 0;
}

// Each engine's own advice, appended to the flag's name in the message.
struct ErrorHints {
  const char* arena;   // after " arena-overflow"
  const char* visits;  // after " visit-table-overflow"
};

// The error flags kernels raised (stats[kStatErrors]): 0, or AZ_E_DEVICE with their names.
inline int device_error_status(unsigned long long* stats, const ErrorHints& hints) {
  unsigned long long err = 0;
  AZ_HIP(hipMemcpy(&err, stats + kStatErrors, sizeof(err), hipMemcpyDeviceToHost));
  if (!err) return 0;
  std::string m = "device error flags:";
  if (err & kErrArena) m += std::string(" arena-overflow") + hints.arena;
  if (err & kErrPow) m += std::string(" visit-table-overflow") + hints.visits;
  if (err & kErrPath) m += " path-overflow";
  if (err & kErrIllegal) m += " illegal-move";
  if (err & kErrNoRoot) m += " play-before-search";
  if (err & kErrNoise) m += " root-noise-rows-exhausted(pass a row per root selection)";
  if (err & kErrDraw) m += " root-noise-draw-round-cap(a defect in the device Dirichlet draw or a corrupt stream position)";
  if (err & kErrActRange)
    m += " activation-range(a non-finite activation, or |x| > 32752 in the per-layer fp16x2 convs: "
         "use conv_algo=AZ_CONV_F16X2 or AZ_CONV_DIRECT)";
  // play on a slot without a searched root changes nothing: that flag is
  // cleared once reported (the others mean a broken tree and stay)
  if (err == kErrNoRoot) AZ_HIP(hipMemset(stats + kStatErrors, 0, sizeof(err)));
  return fail_abi(AZ_E_DEVICE, m);
}

// The move clock behind asynchronous steps (*_selfplay_step without stats
// returns while the lanes' kernels run) and the drain.  Moves are numbered
// over the engine's life.  The last lane to finish move m stores the
// games-finished count into snap_host[m % 4] (launch_move_end), and a drain
// reads the newest complete snapshot (az_move_clock.h), so it never waits for
// the move that is running.  A lane plays move m only once every other lane
// has finished move m - 1: that snapshot then holds no game of move m, and the
// lanes stay within two moves of each other (the cache eviction bound, az_engine.hip).
struct MoveClock {
  int32_t* arrive = nullptr;                // device [4]: lanes done with move m, slot m % 4
  unsigned long long* snap_host = nullptr;  // [4] pinned coherent, move m in slot m % 4
  unsigned long long* snap_dev = nullptr;   // snap_host's device address
  int64_t issued = 0;                       // moves enqueued
  int64_t batch_first = 0;                  // `issued` at the batch's begin
  int64_t drained = 0;                      // finished games of the batch the drain has returned
  std::vector<std::array<hipEvent_t, 4>> done;  // [lane]: end of move m on the lane, slot m % 4

  // snapshot_error: the caller's wording for a failed snapshot setup
  int create(DeviceAllocs& mem, int lanes, const char* snapshot_error) {
    done.assign(lanes, std::array<hipEvent_t, 4>{});
    for (auto& lane : done)
      for (hipEvent_t& ev : lane)
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
          return fail_abi(AZ_E_HIP, "hipEventCreate failed");
    AZ_TRY(mem.alloc(&arrive, 4, false));
    if (hipMemset(arrive, 0, 4 * sizeof(int32_t)) != hipSuccess ||
        hipHostMalloc(&snap_host, 4 * sizeof(unsigned long long), hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&snap_dev, snap_host, 0) != hipSuccess)
      return fail_abi(AZ_E_HIP, snapshot_error);
    for (int i = 0; i < 4; ++i) snap_host[i] = 0;
    return 0;
  }
  void destroy() {
    if (snap_host) (void)hipHostFree(snap_host);
    for (auto& lane : done)
      for (hipEvent_t ev : lane)
        if (ev) (void)hipEventDestroy(ev);
  }
  void begin_batch() {
    drained = 0;
    batch_first = issued;
  }
  // a move's epilogue on `lane`'s stream s: before its play launch ...
  int before_play(int64_t m, size_t lane, hipStream_t s) {
    if (m > batch_first)
      for (size_t o = 0; o < done.size(); ++o)
        if (o != lane) AZ_HIP(hipStreamWaitEvent(s, done[o][(m - 1) % 4], 0));
    return 0;
  }
  // ... and after it (and whatever else of the move follows the play)
  int after_play(int64_t m, size_t lane, hipStream_t s, const unsigned long long* done_count) {
    launch_move_end(arrive + m % 4, (int)done.size(), done_count, snap_dev + m % 4, s);
    AZ_HIP(hipEventRecord(done[lane][m % 4], s));
    return 0;
  }
  // *n: finished games a drain may return now, at most max_games (they start at `drained`)
  int drainable(int64_t max_games, int64_t* n) {
    *n = 0;
    const int64_t last = issued - 1;
    bool last_done = last >= batch_first;
    if (last_done)
      for (auto& lane : done) last_done = last_done && hipEventQuery(lane[last % 4]) == hipSuccess;
    const DrainMove k = drainable_move(last, batch_first, last_done);
    if (k.move < 0) return 0;
    if (k.wait)
      for (auto& lane : done) AZ_HIP(hipEventSynchronize(lane[k.move % 4]));
    const unsigned long long finished = __atomic_load_n(snap_host + k.move % 4, __ATOMIC_ACQUIRE);
    *n = std::max<int64_t>(std::min<int64_t>((int64_t)finished - drained, max_games), 0);
    return 0;
  }
};

// What both engines report alike: the device counter block (also left in h
// for the caller's own fields), the cache control words, the slots holding a
// game.  Clears *st first.
inline int read_common_stats(az_stats* st, unsigned long long (&h)[kStatCount], const unsigned long long* stats,
                             const int64_t* game_id, int slots, const CacheCore& cache) {
  AZ_HIP(hipMemcpy(h, stats, sizeof(h), hipMemcpyDeviceToHost));
  std::vector<int64_t> gid(slots);
  AZ_HIP(hipMemcpy(gid.data(), game_id, gid.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  memset(st, 0, sizeof(*st));
  st->expansions = (int64_t)h[kStatExpansions];
  st->terminal_visits = (int64_t)h[kStatTerminal];
  st->games_done = (int64_t)h[kStatGamesDone];
  st->simulations = (int64_t)h[kStatSims];
  st->plies = (int64_t)h[kStatPlies];
  st->errors = (int64_t)h[kStatErrors];
  st->cache_hits = (int64_t)h[kStatCacheHits];
  st->evaluations = (int64_t)h[kStatNNEvals];
  st->active_slots = std::count_if(gid.begin(), gid.end(), [](int64_t v) { return v >= 0; });
  if (cache.ctl) {
    unsigned long long ctl[3];
    AZ_HIP(hipMemcpy(ctl, cache.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    st->cache_generation = (int64_t)ctl[0];
    st->cache_inserts = (int64_t)ctl[1];
    st->cache_gen_size = (int64_t)cache.gen_size;
    st->cache_entries = (int64_t)ctl[2];
    st->cache_capacity = (int64_t)cache.mask + 1;
  }
  return 0;
}

// Flushes the timers (call after their streams' synchronize) into conv_ms and
// conv_launches; conv_busy_ms = the union of their intervals over all lanes.
inline void conv_busy_union(const std::vector<ConvTimer*>& timers, az_stats* st) {
  std::vector<std::pair<double, double>> iv;
  for (ConvTimer* tm : timers) {
    tm->flush();
    st->conv_ms += tm->total_ms;
    st->conv_launches += tm->launches;
    iv.insert(iv.end(), tm->intervals.begin(), tm->intervals.end());
  }
  std::sort(iv.begin(), iv.end());
  double busy = 0.0, lo = 0.0, hi = -1.0;
  for (const auto& x : iv) {
    if (x.first > hi) {
      if (hi > lo) busy += hi - lo;
      lo = x.first;
      hi = x.second;
    } else {
      hi = std::max(hi, x.second);
    }
  }
  if (hi > lo) busy += hi - lo;
  st->conv_busy_ms = busy;
}

// A fresh common origin (*ref, recorded on the idle `stream`) for the timers'
// intervals, and the timers cleared and switched; every stride-th launch is timed.
inline int arm_timers(hipEvent_t* ref, hipStream_t stream, const std::vector<ConvTimer*>& timers, bool enabled,
                      int stride) {
  if (!*ref) AZ_HIP(hipEventCreate(ref));
  AZ_HIP(hipEventRecord(*ref, stream));
  AZ_HIP(hipStreamSynchronize(stream));
  for (ConvTimer* tm : timers) {
    tm->flush();
    tm->reset();
    tm->ref = ref;
    tm->enabled = enabled;
    tm->stride = stride;
  }
  return 0;
}

// [0, libm pow(k, 0.5) for k = 1 .. len - 1]: Python's `int ** 0.5`
// (mcts.py:50) is float_pow -> pow(n, 0.5), which is NOT sqrt for 1,638
// n <= 2e6; through a volatile pointer, so no compiler folds it into sqrt.
inline std::vector<double> sqrt_pow_table(int len) {
  double (*volatile libm_pow)(double, double) = pow;
  std::vector<double> t(len);
  for (int k = 0; k < len; ++k) t[k] = k == 0 ? 0.0 : libm_pow((double)k, 0.5);
  return t;
}

}  // namespace az
