// az_session.h -- the host session both engine handles (az_engine,
// az_chess_engine) extend: the device, the streams, the move clock, owned
// memory, the evaluator buffers and the host evaluator's staging; the entry
// guard of the ABI calls; the lanes' evaluator slices; the self-play loop.
// The engines decide which streams exist (their lane rules); the session
// records them and which of them it owns.
#pragma once
#include "az_host.h"

namespace az {

// AZ_EVAL_HOST: the callback and its pinned staging buffers (one engine batch).
struct HostEval {
  az_eval_fn fn = nullptr;
  void* user = nullptr;
  float *x = nullptr, *p = nullptr, *v = nullptr;
  int32_t* n = nullptr;

  int create(size_t slots, size_t row_floats, size_t actions) {
    if (hipHostMalloc(&x, slots * row_floats * sizeof(float), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&p, slots * actions * sizeof(float), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&v, slots * sizeof(float), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&n, sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
      return fail_abi(AZ_E_HIP, "host evaluator staging allocation failed");
    return 0;
  }
  void destroy() {
    for (void* q : {(void*)x, (void*)p, (void*)v, (void*)n})
      if (q) (void)hipHostFree(q);
  }
  // The rows the caller's encode launch queued on s (dev_x, *dev_count of them)
  // to the host, the callback, its outputs back to dev_probs / dev_values.
  // Synchronous on s: after the first wait the count and the rows are final;
  // after the last one the staging buffers are free for the next lane.
  int run(hipStream_t s, const float* dev_x, const int32_t* dev_count, int max_rows, size_t row_floats,
          size_t actions, float* dev_probs, float* dev_values) {
    AZ_HIP(hipMemcpyAsync(n, dev_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    AZ_HIP(hipStreamSynchronize(s));
    const int rows = *n;
    if (rows <= 0) return 0;
    if (rows > max_rows) return fail_abi(AZ_E_DEVICE, "host evaluator: leaf count past the lane's slots");
    AZ_HIP(hipMemcpyAsync(x, dev_x, (size_t)rows * row_floats * sizeof(float), hipMemcpyDeviceToHost, s));
    AZ_HIP(hipStreamSynchronize(s));
    if (fn(user, x, rows, p, v) != 0) return fail_abi(AZ_E_CALLBACK, "the host evaluator returned an error");
    AZ_HIP(hipMemcpyAsync(dev_probs, p, (size_t)rows * actions * sizeof(float), hipMemcpyHostToDevice, s));
    AZ_HIP(hipMemcpyAsync(dev_values, v, (size_t)rows * sizeof(float), hipMemcpyHostToDevice, s));
    AZ_HIP(hipStreamSynchronize(s));
    return 0;
  }
};

// A lane's slot range, its stream and its slices of the evaluator buffers.
struct EvalLane {
  int first = 0, n = 0;
  hipStream_t stream = nullptr;
  float* x = nullptr;
  float* act[3] = {nullptr, nullptr, nullptr};
  float* probs = nullptr;
  float* values = nullptr;
  ConvTimer timer;
  int32_t* counts = nullptr;  // the lane's eval queue counters, alternating by simulation
};

struct Session {
  int device = 0;
  hipStream_t stream = nullptr;           // the ABI calls' own work; owned
  std::vector<hipStream_t> lane_streams;  // the lanes' streams other than `stream`; owned
  hipStream_t pack_stream = nullptr;      // the drain's copies
  bool own_pack_stream = false;           // (else pack_stream is `stream`)
  MoveClock clock;
  DeviceAllocs mem;
  DeviceAllocs samples;  // the self-play sample buffers, re-made at every *_selfplay_begin
  hipEvent_t timer_ref = nullptr;  // common origin of every ConvTimer's intervals
  // evaluator buffers, one engine batch (slots rows); the lanes hold slices
  float* x = nullptr;
  float* act[3] = {nullptr, nullptr, nullptr};
  float* probs = nullptr;
  float* values = nullptr;
  HostEval host;
  // a host evaluator failed mid-simulation (AZ_E_CALLBACK): the leaves it
  // selected were never expanded, so the trees are one simulation short;
  // searching refuses until *_selfplay_begin or *_tree_reset starts over
  bool broken = false;
  int64_t sp_n = 0;  // games of the batch *_selfplay_begin started

  int new_stream(hipStream_t* s) {
    if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess)
      return fail_abi(AZ_E_HIP, "hipStreamCreate failed");
    return 0;
  }
  int new_lane_stream(hipStream_t* s) {
    AZ_TRY(new_stream(s));
    lane_streams.push_back(*s);
    return 0;
  }

  int sync_all() {
    AZ_HIP(hipStreamSynchronize(stream));
    for (hipStream_t s : lane_streams) AZ_HIP(hipStreamSynchronize(s));
    if (own_pack_stream) AZ_HIP(hipStreamSynchronize(pack_stream));
    return 0;
  }

  // The entry rule.  Every ABI call on an engine handle checks its arguments,
  // then calls enter(): the device, then every queued move finished.
  // (*_selfplay_step without stats returns while the lanes' kernels run on
  // non-blocking streams; their samples, trees and evaluator slices must not
  // be read or overwritten under them.)  The exceptions: *_selfplay_step and
  // *_selfplay_drain, which must not wait (they set the device only); getters
  // of host fields (az_engine_lanes); and a state check that an ABI call has
  // always made before touching the device keeps its place in front of enter().
  int enter() {
    AZ_HIP(hipSetDevice(device));
    return sync_all();
  }

  // The three refusals of a search; `abi` is the engine's symbol prefix ("az_", "az_chess_").
  int ready_to_search(int evaluator, bool net_ready, const char* abi) const {
    const std::string p = abi;
    if (broken)
      return fail_abi(AZ_E_STATE, "a host evaluator error interrupted a simulation: the trees are incomplete "
                                  "until " + p + "selfplay_begin or " + p + "tree_reset");
    if (evaluator == AZ_EVAL_NETWORK && !net_ready)
      return fail_abi(AZ_E_STATE, "network evaluator selected but " + p + "engine_set_weights was not called");
    if (evaluator == AZ_EVAL_HOST && !host.fn)
      return fail_abi(AZ_E_STATE, "host evaluator selected but " + p + "engine_set_evaluator was not called");
    return 0;
  }

  // L's range and its slices of the evaluator buffers, rows of x_row_floats /
  // act_row_floats / actions floats (a buffer the engine did not allocate stays null)
  void slice(EvalLane& L, int first, int n, size_t x_row_floats, size_t act_row_floats, size_t actions) const {
    const size_t f = (size_t)first;
    L.first = first;
    L.n = n;
    L.x = x ? x + f * x_row_floats : nullptr;
    for (int i = 0; i < 3; ++i) L.act[i] = act[i] ? act[i] + f * act_row_floats : nullptr;
    L.probs = probs + f * actions;
    L.values = values + f;
  }

  // The end of *_selfplay_begin, once the caller has entered, freed `samples`
  // and made the batch's own: the clock's batch, the counter block with the
  // next game to hand out, and slot_init(first_wave) -- the engine's launch
  // that seats the first wave of games -- finished on `stream`.
  template <typename SlotInit>
  int begin_batch(unsigned long long* stats, int slots, int64_t first_game, int64_t n_games, SlotInit slot_init) {
    clock.begin_batch();
    unsigned long long st[kStatCount] = {0};
    const int64_t first_wave = std::min<int64_t>(n_games, slots);
    st[kStatNextGame] = (unsigned long long)(first_game + first_wave);
    AZ_HIP(hipMemcpyAsync(stats, st, sizeof(st), hipMemcpyHostToDevice, stream));
    AZ_TRY(slot_init(first_wave));
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(stream));
    sp_n = n_games;
    return 0;
  }

  // n_moves moves enqueued for every lane, without waiting: per move `sims`
  // simulations, the lanes interleaved per simulation so every stream always
  // has work queued; finish_search(lane) (what a search owes after its last
  // simulation); then per lane the clock's epilogue around play(lane).
  template <typename LaneT, typename Simulate, typename Finish, typename Play>
  int step_moves(int n_moves, int sims, const std::vector<LaneT*>& lanes, const unsigned long long* done_count,
                 Simulate simulate, Finish finish_search, Play play) {
    AZ_HIP(hipSetDevice(device));
    for (int mv = 0; mv < n_moves; ++mv) {
      const int64_t m = clock.issued++;
      for (int s = 0; s < sims; ++s)
        for (LaneT* L : lanes) AZ_TRY(simulate(*L));
      for (LaneT* L : lanes) AZ_TRY(finish_search(*L));
      for (size_t l = 0; l < lanes.size(); ++l) {
        LaneT& L = *lanes[l];
        AZ_TRY(clock.before_play(m, l, L.stream));
        play(L);
        AZ_TRY(clock.after_play(m, l, L.stream, done_count));
      }
      AZ_HIP(hipGetLastError());
    }
    return 0;
  }

  // Everything the session owns, after its work has finished (a handle's destroy).
  void destroy() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipStream_t s : lane_streams) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
    if (own_pack_stream && pack_stream) {
      (void)hipStreamSynchronize(pack_stream);
      (void)hipStreamDestroy(pack_stream);
    }
    clock.destroy();
    samples.free_all();
    mem.free_all();
    if (timer_ref) (void)hipEventDestroy(timer_ref);
    host.destroy();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// *_selfplay_run: begin(), then step(&stats) move by move until no slot holds a game.
template <typename Begin, typename Step>
int run_to_end(az_stats* st, Begin begin, Step step) {
  AZ_TRY(begin());
  az_stats tmp;
  do {
    AZ_TRY(step(&tmp));
  } while (tmp.active_slots != 0);
  if (st) *st = tmp;
  return 0;
}

}  // namespace az
